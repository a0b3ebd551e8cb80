"""CPU tests of the stream filters: the coefficient design through the C ABI (no GPU), the restatements
(tests/streamfilter_ref.py) against what the compiled reference wrote (tests/golden/streamfilter.npz, made by
tests/golden/make_golden_streamfilter.py), stream sharding, and the argument errors that need no device.
Every comparison is bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import streamfilter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jeicyboodsp_amd", "libjdsp.so")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build_hip()
    return C.CDLL(LIB)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "streamfilter.npz"))


def design(lib, gains):
    out = np.full((7, 2, 3), np.nan)
    g = None if gains is None else np.asarray(gains, np.float64)
    rc = lib.jdsp_geq_design(g.ctypes.data_as(C.c_void_p) if g is not None else None, out.ctypes.data_as(C.c_void_p))
    return rc, out


def test_design_equals_the_compiled_reference_and_the_restatement(lib, gold):
    rc, got = design(lib, None)
    assert rc == 0
    assert got.tobytes() == gold["geq_coeff"].tobytes()                      # all 42 doubles of rgdBandCoeff
    assert R.geq_design().tobytes() == gold["geq_coeff"].tobytes()
    assert np.array_equal(design(lib, R.GAINS)[1], got)
    # the other branches: band 1 cut, band 7 boost, a peaking cut
    for gains in [(-12.0, 12.0, 0.0, 0.0, 3.0, 0.0, -12.0), (12.0, 12.0, 0.0, 0.0, 3.0, 0.0, 9.0),
                  (12.0, -7.5, 0.0, -3.0, 3.0, 0.0, -12.0), (-4.0, -1.0, 2.0, -6.0, 0.5, -9.0, 4.0)]:
        rc, got = design(lib, gains)
        assert rc == 0 and np.array_equal(got, R.geq_design(gains)), gains
        assert np.all(np.isfinite(got)) and np.all(got[:, 1, 0] == 0.0)


def test_geq_restatement_equals_the_reference_files(gold):
    names = sorted(k[8:] for k in gold.files if k.startswith("geq_pcm_"))
    assert names == sorted(R.geq_families())
    wrapped = 0
    for name in names:
        pcm = gold["geq_pcm_" + name]
        assert np.array_equal(pcm, R.geq_families()[name]) and len(pcm) == 16 * R.GEQ_BLOCK
        out, pre, _ = R.geq(pcm, gold["geq_coeff"])
        assert out.tobytes() == gold["geq_out_" + name].tobytes(), name
        wrapped += int(np.count_nonzero(np.abs(pre) >= 32769.0)) if name == "loud" else 0
    assert wrapped > 0                                                       # the loud family does wrap
    # cut into the reference's blocks, state carried: the same bytes
    pcm, st, parts = gold["geq_pcm_loud"], None, []
    for b in range(0, len(pcm), R.GEQ_BLOCK):
        o, _, st = R.geq(pcm[b:b + R.GEQ_BLOCK], gold["geq_coeff"], st)
        parts.append(o)
    assert np.concatenate(parts).tobytes() == gold["geq_out_loud"].tobytes()


@pytest.mark.parametrize("order", ["reference", "device"])
def test_nlms_restatement_equals_the_reference_files(gold, order):
    """order="device" (the kernel's documented tree) on the SAME committed streams, no sample excluded"""
    names = sorted(k[8:] for k in gold.files if k.startswith("nlms_in_"))
    assert names == sorted(R.nlms_families())
    for name in names:
        x, ref = gold["nlms_in_" + name], gold["nlms_ref_" + name]
        assert np.array_equal(x, R.nlms_families()[name][0]) and len(x) == 8 * R.NLMS_BLOCK
        est, err, _, _ = R.nlms(x, ref, order=order)
        assert est[R.NLMS_BLOCK:].tobytes() == gold["nlms_est_" + name].tobytes(), name
        assert err[R.NLMS_BLOCK:].tobytes() == gold["nlms_err_" + name].tobytes(), name


def test_stream_shard_covers_every_stream_once():
    from jeicyboodsp_amd.sharding import stream_shard
    for n_streams in (0, 1, 5, 8, 10000, 65536):
        for world in (1, 2, 3, 8):
            seen = []
            for rank in range(world):
                first, count = stream_shard(n_streams, rank, world)
                assert count >= 0 and abs(count - n_streams / world) < 1
                seen.extend(range(first, first + count))
            assert seen == list(range(n_streams)), (n_streams, world)


def test_argument_errors_that_need_no_device(lib):
    out = np.zeros((7, 2, 3))
    assert lib.jdsp_geq_design(None, None) == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        g = np.array(R.GAINS)
        g[4] = bad
        assert lib.jdsp_geq_design(g.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == EINVAL
    h = C.c_void_p()
    lib.jdsp_geq_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.POINTER(C.c_void_p)]
    lib.jdsp_nlms_create.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_long, C.POINTER(C.c_void_p)]
    assert lib.jdsp_geq_create(None, None, 7, 1, C.byref(h)) == EINVAL and not h.value
    assert lib.jdsp_nlms_create(None, 256, 1e-4, 1e-4, 1, C.byref(h)) == EINVAL and not h.value
    for name in ("jdsp_geq_destroy", "jdsp_nlms_destroy"):
        f = getattr(lib, name)
        f.argtypes = [C.c_void_p]
        assert f(None) == 0
    for name in ("jdsp_geq_reset", "jdsp_nlms_reset"):
        f = getattr(lib, name)
        f.argtypes = [C.c_void_p]
        assert f(None) == EINVAL
    lib.jdsp_geq_process.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_void_p]
    assert lib.jdsp_geq_process(None, None, 8, 8, None, None) == EINVAL
