"""GPU tests of the host layer over the time-domain entries: the CLI programs jdsp_pitch2 / jdsp_pitch3 / jdsp_lpc
(compat/drivers.cpp) and the reference-signature wrapper LPCEstimation (compat/jeicyboo_compat.h), the latter through
compat_selftest's "lpc" mode, which runs the reference's main() loop."""
import os
import re
import subprocess

import numpy as np
import pytest

import timedomain_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "jeicyboodsp_amd", "compat")
LINE = re.compile(r"Estimation arg (-?\d+) , dMin (\S+) pitch (\S+)")


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def write_wav(path, pcm):
    with open(path, "wb") as f:
        f.write(b"\0" * 44)
        f.write(np.asarray(pcm, "<i2").tobytes())


@pytest.mark.parametrize("method", [2, 3])
def test_pitch_programs_print_the_reference_lags(golden_dir, tmp_path, method):
    g = np.load(os.path.join(golden_dir, "timedomain.npz"))
    for name in ("mixed", "full_scale", "silence", "zero_keep"):
        wav = tmp_path / ("%s.wav" % name)
        write_wav(wav, g["pcm_" + name])
        out = subprocess.run([os.path.join(COMPAT, "jdsp_pitch%d" % method), str(wav)], check=True, timeout=120,
                             capture_output=True, text=True).stdout
        rows = LINE.findall(out)
        g_arg, g_val = g["arg%d_%s" % (method, name)], g["val%d_%s" % (method, name)]
        assert [int(a) for a, _, _ in rows] == g_arg.tolist(), name
        assert [v for _, v, _ in rows] == ["%f" % v for v in g_val], name          # the same digits as the reference
        assert [p for _, _, p in rows] == ["%f" % (16000.0 / a) for a in g_arg], name
        assert out.rstrip().endswith("Processing End")


def test_lpc_program_and_compat_wrapper(eng, tmp_path):
    pcm = np.concatenate([R.voiced(41, 9, 256), R.silence(2, 256), R.white(42, 6, 256)])
    want = eng.lpc(pcm, 256, 12)
    assert want.shape == (17, 12)
    write_wav(tmp_path / "in.wav", pcm)
    subprocess.run([os.path.join(COMPAT, "jdsp_lpc"), str(tmp_path / "in.wav"), str(tmp_path / "out.lpc")], check=True,
                   timeout=120, stdout=subprocess.DEVNULL)
    got = np.fromfile(tmp_path / "out.lpc", np.float64).reshape(-1, 12)
    assert got.shape == (16, 12)                                                   # n - 1 vectors
    assert np.array_equal(got, want[1:], equal_nan=True)
    # bool LPCEstimation(short*, double*): one block per call, static keep buffer, first call returns false
    pcm.tofile(tmp_path / "in.raw")
    subprocess.run([os.path.join(COMPAT, "compat_selftest"), "lpc", str(tmp_path / "in.raw"), str(tmp_path / "out.bin")],
                   check=True, timeout=120, stdout=subprocess.DEVNULL)
    got = np.fromfile(tmp_path / "out.bin", np.float64).reshape(-1, 12)
    assert got.shape == (16, 12)
    assert np.array_equal(got, want[1:], equal_nan=True)
    assert np.all(np.isnan(want[10])) and np.all(np.isfinite(want[[9, 11]]))       # frame 10 = [silence, silence]
