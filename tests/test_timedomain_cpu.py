"""CPU tests of the time-domain pitch (AMDF, autocorrelation) and LPC feature:
  - the numpy restatements (tests/timedomain_ref.py) against what the reference's own programs printed
    (tests/golden/timedomain.npz, made by tests/golden/make_golden_timedomain.py);
  - the new entries are declared in include/jdsp.h, exported by libjdsp.so and prototyped by _lib.py;
  - K_ref: the forward error of the FP64 LU-inverse solve against an extended-precision solve, the unit of the
    device solve's bound in test_timedomain_gpu.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import timedomain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["jdsp_pitch_lag_dev", "jdsp_pitch_lag", "jdsp_lpc_dev", "jdsp_lpc"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "timedomain.npz"))


def stream_names(golden):
    return sorted(k[4:] for k in golden.files if k.startswith("pcm_"))


def test_golden_covers_the_families(golden):
    names = stream_names(golden)
    assert {"mixed", "voiced", "white", "silence", "constant", "full_scale", "zero_keep"} <= set(names)
    for n in names:
        assert golden["pcm_" + n].dtype == np.int16
        for m in (2, 3):
            assert len(golden["arg%d_%s" % (m, n)]) == len(golden["pcm_" + n]) // 512


@pytest.mark.parametrize("method", [2, 3])
def test_restatement_equals_reference_prints(golden, method):
    """lag equal on every block; value within the %f print precision, 5e-7 + 2^-52 |value|"""
    n_blocks = 0
    for name in stream_names(golden):
        arg, val, curve = R.pitch_stream(golden["pcm_" + name], method)
        g_arg, g_val = golden["arg%d_%s" % (method, name)], golden["val%d_%s" % (method, name)]
        assert np.array_equal(arg, g_arg), (name, np.flatnonzero(arg != g_arg))
        assert np.all(np.abs(val - g_val) <= 5e-7 + 2.0 ** -52 * np.abs(val)), name
        assert np.all((arg > 100) & (arg < 512))
        n_blocks += len(arg)
    assert n_blocks >= 80


def test_restatement_silence_and_ties():
    for method in (2, 3):
        arg, val, curve = R.pitch_stream(R.silence(3), method)
        assert arg.tolist() == [101, 101, 101] and np.all(val == 0) and np.all(curve == 0)
    # a period-128 square wave: the AMDF is exactly 0 at lags 128, 256 and 384, and the smallest lag wins the tie
    x = np.tile(np.r_[np.full(64, 1000), np.full(64, -1000)], 8).astype(np.int16)
    arg, val, _ = R.pitch_stream(np.r_[x[:512], x[:512]], 2)
    assert arg[1] == 128 and val[1] == 0


def test_sums_exceed_32_bits(golden):
    """the exactness argument needs more than an int32: the full-scale family's sums pass 2^32"""
    _, _, curve = R.pitch_stream(golden["pcm_full_scale"], 3)
    sums = np.abs(curve * (1024 - np.arange(512)))
    assert 2.0 ** 32 < sums.max() < 2.0 ** 40


def test_new_entries_declared_exported_and_prototyped():
    """fails before the feature: the header, the library and the ctypes table all carry the four entries"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jdsp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(jdsp_[a-z0-9_]+)\s*\(", txt))
    assert set(NEW_ENTRIES) <= declared
    assert re.search(r"JDSP_PITCH_AMDF\s*=\s*2\b", txt) and re.search(r"JDSP_PITCH_ACF\s*=\s*3\b", txt)
    lib_path = os.path.join(ROOT, "jeicyboodsp_amd", "libjdsp.so")
    if not os.path.exists(lib_path):
        import __graft_entry__
        __graft_entry__.build_hip()
    lib = C.CDLL(lib_path)
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    lib.jdsp_abi_version.restype = C.c_int
    assert lib.jdsp_abi_version() == 2
    # NULL handle: an error code, not a crash
    lib.jdsp_pitch_lag.restype = C.c_int
    lib.jdsp_pitch_lag.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long] + [C.c_void_p] * 4
    assert lib.jdsp_pitch_lag(None, 2, None, 0, None, None, None, None) == -1
    from jeicyboodsp_amd import _lib
    vp, i, l = C.c_void_p, C.c_int, C.c_long
    assert _lib.lib.jdsp_pitch_lag_dev.argtypes == [vp, i, vp, l, vp, vp, vp, vp]
    assert _lib.lib.jdsp_pitch_lag.argtypes == [vp, i, vp, l, vp, vp, vp, vp]
    assert _lib.lib.jdsp_lpc_dev.argtypes == [vp, vp, l, i, i, vp, vp, vp]
    assert _lib.lib.jdsp_lpc.argtypes == [vp, vp, l, i, i, vp, vp, vp]
    assert (_lib.PITCH_AMDF, _lib.PITCH_ACF) == (2, 3)
    import jeicyboodsp_amd
    assert callable(jeicyboodsp_amd.Engine.pitch_lag) and callable(jeicyboodsp_amd.Engine.lpc)


def test_lpc_restatement_shapes_and_silence():
    a, r = R.lpc_stream(R.white(5, 6, 256), 256, 12)
    assert a.shape == (6, 12) and r.shape == (6, 13) and np.all(np.isfinite(a))
    T, v = R.toeplitz_system(r[3])
    assert np.abs(T @ a[3] - v).max() <= 1e-9 * np.abs(v).max()
    a, r = R.lpc_stream(R.silence(2, 256), 256, 12)
    assert np.all(np.isnan(a)) and np.all(r == 0)
    # the frame that follows silence has a zero first half and is solvable
    a, _ = R.lpc_stream(np.r_[R.silence(1, 256), R.white(6, 1, 256)], 256, 12)
    assert np.all(np.isnan(a[0])) and np.all(np.isfinite(a[1]))


def test_lpc_k_ref_is_finite():
    """K_ref = worst forward error of the FP64 LU-inverse solve, in units of eps * cond_2(T) * |a|_inf, against the
    extended-precision solve, over every frame of lpc_families() x LPC_CASES (DESIGN.md section 3.8 records it)."""
    k_ref, worst_cond = R.measure_k_ref()
    print("K_ref = %.4f   largest cond_2(T) = %.3e" % (k_ref, worst_cond))
    assert math.isfinite(k_ref) and k_ref > 0
    assert math.isfinite(worst_cond)
