"""GPU tests of the host layer over the stream filters: the CLI programs jdsp_geq / jdsp_nlms (compat/drivers.cpp) on
files built from the golden streams, byte for byte against the compiled reference's output files, and the
reference-signature wrappers CalcCoefficient / ApplyIirGEQ / LMSFilter (compat/jeicyboo_compat.h) through
compat_selftest's "geq" and "nlms" modes, which run the reference's main() loops."""
import os
import subprocess

import numpy as np
import pytest

import streamfilter_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "jeicyboodsp_amd", "compat")


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "streamfilter.npz"))


def write_wav(path, pcm):
    with open(path, "wb") as f:
        f.write(b"\1" * 44)                     # a header that would be heard if it were not skipped
        f.write(np.asarray(pcm, "<i2").tobytes())


def run(*args):
    subprocess.run([str(a) for a in args], check=True, timeout=120, stdout=subprocess.DEVNULL)


def test_geq_program_writes_the_reference_files(gold, tmp_path):
    for name in ("white", "loud", "impulse"):
        write_wav(tmp_path / "in.wav", gold["geq_pcm_" + name])
        run(os.path.join(COMPAT, "jdsp_geq"), tmp_path / "in.wav", tmp_path / "out.raw")
        assert (tmp_path / "out.raw").read_bytes() == gold["geq_out_" + name].tobytes(), name
    # a length that is no multiple of the block: the last fread() is short and the block is completed with the stale
    # tail of the one before, so the file equals that of the stream so completed -- whose head is the golden's
    pcm = gold["geq_pcm_loud"]
    n = 3 * 512 + 200
    write_wav(tmp_path / "in.wav", pcm[:n])
    run(os.path.join(COMPAT, "jdsp_geq"), tmp_path / "in.wav", tmp_path / "out.raw")
    got = np.fromfile(tmp_path / "out.raw", "<i2")
    assert len(got) == 4 * 512
    assert got[:n].tobytes() == gold["geq_out_loud"][:n].tobytes()
    completed = np.concatenate([pcm[:n], pcm[2 * 512 + 200:3 * 512]])
    assert np.array_equal(got, R.geq(completed, gold["geq_coeff"])[0])


def test_nlms_program_writes_the_reference_files(gold, tmp_path):
    for name in ("echo", "full_scale"):
        write_wav(tmp_path / "in.wav", gold["nlms_in_" + name])
        gold["nlms_ref_" + name].astype("<i2").tofile(tmp_path / "ref.raw")
        run(os.path.join(COMPAT, "jdsp_nlms"), tmp_path / "in.wav", tmp_path / "ref.raw", tmp_path / "est.raw",
            tmp_path / "err.raw")
        assert (tmp_path / "est.raw").read_bytes() == gold["nlms_est_" + name].tobytes(), name
        assert (tmp_path / "err.raw").read_bytes() == gold["nlms_err_" + name].tobytes(), name


def test_compat_wrappers_agree_with_the_engine(eng, gold, tmp_path):
    pcm = gold["geq_pcm_loud"][:5 * 512]
    pcm.tofile(tmp_path / "in.raw")
    run(os.path.join(COMPAT, "compat_selftest"), "geq", tmp_path / "in.raw", tmp_path / "out.bin")
    g = eng.geq(1)
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.int16), g.process(pcm)[0])
    g.close()
    x, ref = gold["nlms_in_echo"][:3 * 1024], gold["nlms_ref_echo"][:3 * 1024]
    x.tofile(tmp_path / "in.raw")
    ref.tofile(tmp_path / "ref.raw")
    run(os.path.join(COMPAT, "compat_selftest"), "nlms", tmp_path / "in.raw", tmp_path / "out.bin", tmp_path / "ref.raw")
    got = np.fromfile(tmp_path / "out.bin", np.int16).reshape(2, 2, 1024)      # blocks 1 and 2: est, err
    f = eng.nlms(1)
    est, err = f.process(x, ref)
    assert np.array_equal(got[:, 0].reshape(-1), est[0, 1024:]) and np.array_equal(got[:, 1].reshape(-1), err[0, 1024:])
    f.close()
