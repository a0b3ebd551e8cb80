"""GPU tests: time-domain pitch (jdsp_pitch_lag: AMDF, autocorrelation) and LPC (jdsp_lpc).

Pitch is bit-exact: arg, value and curve are np.array_equal to the int64 restatement (tests/timedomain_ref.py, itself
checked against the reference's prints in test_timedomain_cpu.py), tie-breaking included.

LPC is checked in two stages.  Stage 1: autocorr within 1100 eps sum_j |y_j y_{j+i}| / (N - i) of the restatement
(any order of summation costs at most 511 eps per side, the window's cos, subtraction and multiply a few eps per
product; both sides contribute).  Stage 2: lpc against the extended-precision solve of the Toeplitz system built from
the RETURNED autocorr, within 4 K_ref eps cond_2(T) |a|_inf, where K_ref is numpy's LU-inverse solve's own worst error
in those units over the same families (timedomain_ref.measure_k_ref) and 4 covers pivot and operation order."""
import numpy as np
import pytest

import timedomain_ref as R

pytestmark = pytest.mark.gpu
EINVAL = -1
METHODS = [2, 3]


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def same(got, want):
    arg, val, curve = got
    w_arg, w_val, w_curve = want
    assert arg.dtype == np.int32 and val.dtype == np.float64
    assert np.array_equal(arg, w_arg), np.flatnonzero(arg != w_arg)
    assert np.array_equal(val, w_val), np.flatnonzero(val != w_val)
    if curve is not None:
        assert curve.dtype == np.float64 and np.array_equal(curve, w_curve), np.argwhere(curve != w_curve)[:4]


def host(t):
    return [None if x is None else x.cpu().numpy() for x in t]


# ---- pitch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [1, 2, 50, 300])
@pytest.mark.parametrize("method", METHODS)
def test_pitch_lag_bit_exact_every_family(eng, method, n_blocks):
    import torch
    for name, pcm in R.pitch_families(n_blocks).items():
        want = R.pitch_stream(pcm, method)
        # host arrays, with and without the curve
        same(eng.pitch_lag(pcm, method, want_curve=True), want)
        same(eng.pitch_lag(pcm, method) + (None,), want)
        # device tensors, with and without the curve
        t = torch.from_numpy(pcm).cuda()
        got = eng.pitch_lag(t, method, want_curve=True)
        got2 = eng.pitch_lag(t, method)
        torch.cuda.synchronize()
        same(host(got), want)
        same(host(got2) + [None], want)


@pytest.mark.parametrize("method", METHODS)
def test_pitch_lag_golden_streams(eng, golden_dir, method):
    """the reference's own printed lags, and its values to the %f print precision"""
    import os
    g = np.load(os.path.join(golden_dir, "timedomain.npz"))
    for name in sorted(k[4:] for k in g.files if k.startswith("pcm_")):
        arg, val = eng.pitch_lag(g["pcm_" + name], method)
        g_val = g["val%d_%s" % (method, name)]
        assert np.array_equal(arg, g["arg%d_%s" % (method, name)]), name
        assert np.all(np.abs(val - g_val) <= 5e-7 + 2.0 ** -52 * np.abs(val)), name


@pytest.mark.parametrize("method", METHODS)
def test_pitch_lag_sliced_stream_is_bit_identical(eng, method):
    """a stream cut into 3 slices with prev_block handed over (simulated sharding) equals the whole stream"""
    import torch
    for name, pcm in R.pitch_families(50).items():
        want = R.pitch_stream(pcm, method)
        cuts = [0, 17, 18, 50]
        for on_device in (False, True):
            parts = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                sl = pcm[a * 512:b * 512]
                prev = pcm[(a - 1) * 512:a * 512] if a else None
                if on_device:
                    got = eng.pitch_lag(torch.from_numpy(sl).cuda(), method, want_curve=True,
                                        prev_block=None if prev is None else torch.from_numpy(prev.copy()).cuda())
                    torch.cuda.synchronize()
                    parts.append(host(got))
                else:
                    parts.append(eng.pitch_lag(sl, method, prev_block=prev, want_curve=True))
            same([np.concatenate([p[i] for p in parts]) for i in range(3)], want)


@pytest.mark.parametrize("method", METHODS)
def test_pitch_lag_silence_and_ties(eng, method):
    arg, val, curve = eng.pitch_lag(R.silence(4), method, want_curve=True)
    assert arg.tolist() == [101] * 4 and np.all(val == 0) and np.all(curve == 0)
    arg, val = eng.pitch_lag(R.silence(4), method)
    assert arg.tolist() == [101] * 4 and np.all(val == 0)
    # exact ties at lags 128, 256, 384 (AMDF 0 at every multiple of the period): the smallest lag wins
    x = np.tile(np.r_[np.full(64, 1000), np.full(64, -1000)], 8).astype(np.int16)
    same(eng.pitch_lag(x, method, want_curve=True), R.pitch_stream(x, method))
    if method == 2:
        assert eng.pitch_lag(x, 2)[0][1] == 128


def test_pitch_lag_optional_outputs_and_errors(eng):
    import ctypes as C
    from jeicyboodsp_amd import JdspError, _lib
    L = _lib.lib
    pcm = R.voiced(3, 5)
    want = R.pitch_stream(pcm, 2)
    arg = np.full(5, -7, np.int32)
    val = np.full(5, -7.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
    assert L.jdsp_pitch_lag(eng._h, 2, vp(pcm), 5, None, vp(arg), None, None) == 0
    assert np.array_equal(arg, want[0])
    assert L.jdsp_pitch_lag(eng._h, 2, vp(pcm), 5, None, None, vp(val), None) == 0
    assert np.array_equal(val, want[1])
    assert L.jdsp_pitch_lag(eng._h, 2, vp(pcm), 5, None, None, None, None) == 0
    assert L.jdsp_pitch_lag(eng._h, 3, None, 0, None, None, None, None) == 0          # n_blocks == 0: no-op
    for bad in (0, 1, 4, -2):
        with pytest.raises(JdspError) as ei:
            eng.pitch_lag(pcm, bad)
        assert ei.value.code == EINVAL
    assert L.jdsp_pitch_lag(eng._h, 2, vp(pcm), -1, None, vp(arg), vp(val), None) == EINVAL
    assert L.jdsp_pitch_lag(eng._h, 2, None, 5, None, vp(arg), vp(val), None) == EINVAL
    assert L.jdsp_pitch_lag_dev(eng._h, 2, C.c_void_p(8), 5, None, None, None, None) == EINVAL   # misaligned pcm
    assert L.jdsp_pitch_lag_dev(eng._h, 5, None, 0, None, None, None, None) == EINVAL


# ---- LPC ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def k_ref():
    k, worst_cond = R.measure_k_ref()
    print("K_ref = %.4f (largest cond_2 %.3e)" % (k, worst_cond))
    assert np.isfinite(k) and k > 0
    return k


@pytest.mark.parametrize("block_len,order", R.LPC_CASES)
def test_lpc_autocorr_and_solve(eng, k_ref, block_len, order):
    import torch
    worst1 = worst2 = 0.0
    for name, pcm in R.lpc_families(R.LPC_SAMPLES).items():
        lpc, ac = eng.lpc(pcm, block_len, order, want_autocorr=True)
        nb = pcm.size // block_len
        assert lpc.shape == (nb, order) and ac.shape == (nb, order + 1)
        # stage 1
        r, mag = R.lpc_autocorr(R.lpc_windowed(pcm, block_len), order)
        excess = np.abs(ac - r) / (1100 * R.EPS * mag)
        worst1 = max(worst1, float(excess.max()))
        assert np.all(np.abs(ac - r) <= 1100 * R.EPS * mag), (name, float(excess.max()))
        # stage 2: every frame
        for b in range(nb):
            assert ac[b, 0] != 0
            a_ext = R.solve_ext(ac[b])
            units = R.forward_error_units(lpc[b], a_ext, R.cond2(ac[b]))
            worst2 = max(worst2, units)
            assert units <= 4 * k_ref, (name, b, units, k_ref)
        # the device-pointer entry gives the same bits, with and without the autocorr output
        t = torch.from_numpy(pcm).cuda()
        d_lpc, d_ac = eng.lpc(t, block_len, order, want_autocorr=True)
        d_only = eng.lpc(t, block_len, order)
        torch.cuda.synchronize()
        assert np.array_equal(d_lpc.cpu().numpy(), lpc) and np.array_equal(d_ac.cpu().numpy(), ac)
        assert np.array_equal(d_only.cpu().numpy(), lpc)
    print("block %d order %d: autocorr error %.4f of its bound, solve error %.4f eps cond |a| (bound %.3f)"
          % (block_len, order, worst1, worst2, 4 * k_ref))


@pytest.mark.parametrize("block_len", [256, 512])
def test_lpc_is_independent_of_the_batch(eng, block_len):
    """a frame run alone equals the same frame inside a batch of 300, bit for bit"""
    pcm = np.concatenate([R.voiced(31, 100, block_len), R.lowpassed(32, 100, block_len), R.white(33, 100, block_len)])
    lpc, ac = eng.lpc(pcm, block_len, 12, want_autocorr=True)
    assert lpc.shape == (300, 12)
    for b in (0, 1, 99, 100, 217, 299):
        prev = pcm[(b - 1) * block_len:b * block_len] if b else None
        l1, a1 = eng.lpc(pcm[b * block_len:(b + 1) * block_len], block_len, 12, prev_block=prev, want_autocorr=True)
        assert np.array_equal(l1[0], lpc[b]) and np.array_equal(a1[0], ac[b]), b
    # three slices with the keep buffer handed over
    parts = [eng.lpc(pcm[a * block_len:b * block_len], block_len, 12,
                     prev_block=pcm[(a - 1) * block_len:a * block_len] if a else None)
             for a, b in ((0, 40), (40, 41), (41, 300))]
    assert np.array_equal(np.concatenate(parts), lpc)


def test_lpc_zero_frames_give_nan(eng, k_ref):
    for block_len in (256, 512):
        pcm = np.r_[R.silence(2, block_len), R.white(7, 2, block_len)]
        lpc, ac = eng.lpc(pcm, block_len, 12, want_autocorr=True)
        assert np.all(ac[:2] == 0) and np.all(np.isnan(lpc[:2]))            # r[0] == 0: all NaN
        assert np.all(np.isfinite(lpc[2:]))
        for b in (2, 3):                                                    # b = 2: the frame's first half is zeros
            assert R.forward_error_units(lpc[b], R.solve_ext(ac[b]), R.cond2(ac[b])) <= 4 * k_ref


def test_lpc_errors(eng):
    import ctypes as C
    from jeicyboodsp_amd import JdspError, _lib
    L = _lib.lib
    pcm = R.white(8, 4, 256)
    for kw in (dict(order=0), dict(order=17), dict(order=-1), dict(block_len=128), dict(block_len=1024)):
        with pytest.raises(JdspError) as ei:
            eng.lpc(pcm, **kw)
        assert ei.value.code == EINVAL
    out = np.zeros((4, 12))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
    assert L.jdsp_lpc(eng._h, vp(pcm), -1, 256, 12, None, None, vp(out)) == EINVAL
    assert L.jdsp_lpc(eng._h, vp(pcm), 4, 256, 12, None, None, None) == EINVAL
    assert L.jdsp_lpc(eng._h, None, 0, 256, 12, None, None, None) == 0                # n_blocks == 0: no-op
    assert L.jdsp_lpc_dev(eng._h, C.c_void_p(8), 4, 256, 12, None, None, C.c_void_p(16)) == EINVAL   # misaligned pcm
