"""GPU tests: the multi-stream IIR equaliser (jdsp_geq_*) and NLMS filter (jdsp_nlms_*).

Everything is np.array_equal: int16 outputs, the pre-cast doubles, the state.  The restatements (tests/streamfilter_ref.py)
are checked against the compiled reference's files in test_streamfilter_cpu.py; the golden tests here compare the GPU
with those files directly.  The NLMS is compared with the restatement's order="device" (the documented tree)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import streamfilter_ref as R

pytestmark = pytest.mark.gpu
EINVAL = -1
GEQ_STREAMS = [1, 7, 8, 9, 65]
GEQ_SAMPLES = [1, 6, 7, 8, 9, 511, 512, 1000]
GEQ_SECTIONS = [1, 2, 7, 8, 9, 16]
NLMS_SAMPLES = [1, 255, 256, 1024, 1025, 3000]


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def coeff_of(n_sections):
    return R.geq_design() if n_sections == 7 else R.stable_sections(n_sections)


@functools.lru_cache(maxsize=None)
def geq_pool():
    """nine distinct streams of 1000 samples, one of every family and three more"""
    n = 1000
    p = [R.white(101, n), R.white(102, n, 9000.0), R.full_scale(103, n), R.impulse(n), R.constant(n), R.silence(n),
         R.white(104, n, 400.0), R.white(105, n, 9000.0), R.full_scale(106, n)]
    return np.stack(p)


@functools.lru_cache(maxsize=None)
def geq_want(n_sections, n):
    """restatement of the pool's first n samples: (out [9, n], precast [9, n], state [9, n_sections + 1, 2])"""
    got = [R.geq(x[:n], coeff_of(n_sections)) for x in geq_pool()]
    return tuple(np.stack([g[i] for g in got]) for i in range(3))


def pick(a, n_streams):
    return a[np.arange(n_streams) % len(a)]


# ---- equaliser -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sections", GEQ_SECTIONS)
def test_geq_equals_the_restatement_at_every_shape(eng, n_sections):
    import torch
    coeff = None if n_sections == 7 else coeff_of(n_sections)
    for n_streams in GEQ_STREAMS:
        g = eng.geq(n_streams, coeff)
        for n in GEQ_SAMPLES:
            w_out, w_pre, w_state = (pick(a, n_streams) for a in geq_want(n_sections, n))
            pcm = np.ascontiguousarray(pick(geq_pool(), n_streams)[:, :n])
            # host arrays
            g.reset()
            out, pre = g.process(pcm, want_precast=True)
            assert out.dtype == np.int16 and pre.dtype == np.float64
            assert np.array_equal(out, w_out), (n_streams, n, np.argwhere(out != w_out)[:4])
            assert np.array_equal(pre, w_pre), (n_streams, n, np.argwhere(pre != w_pre)[:4])
            assert np.array_equal(g.state(), w_state), (n_streams, n)
            # device tensors, rows further apart than n_samples, without the pre-cast output
            g.reset()
            big = torch.full((n_streams, 1016), 77, dtype=torch.int16, device="cuda")
            big[:, :n] = torch.from_numpy(pcm).cuda()
            out = g.process(big[:, :n])
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), w_out), (n_streams, n)
            assert np.array_equal(g.state(), w_state), (n_streams, n)
        g.close()


def test_geq_host_entry_with_a_pitch_past_the_samples(eng):
    """the C entry itself, pitch 24 for 13 samples: what lies between the streams comes back untouched"""
    from jeicyboodsp_amd.engine import L
    n_streams, n, pitch = 9, 13, 24
    g = eng.geq(n_streams)
    pcm = np.full((n_streams, pitch), 999, np.int16)
    pcm[:, :n] = geq_pool()[:, :n]
    out = np.full((n_streams, pitch), -5, np.int16)
    pre = np.full((n_streams, pitch), -5.0, np.float64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.jdsp_geq_process(g._h, vp(pcm), n, pitch, vp(out), vp(pre)) == 0
    w_out, w_pre, _ = geq_want(7, n)
    assert np.array_equal(out[:, :n], w_out) and np.array_equal(pre[:, :n], w_pre)
    assert np.all(out[:, n:] == -5) and np.all(pre[:, n:] == -5.0)
    assert L.jdsp_geq_process(g._h, vp(pcm), 0, pitch, vp(out), None) == 0      # a successful no-op
    g.close()


def test_geq_golden_streams(eng, golden_dir):
    """the compiled reference's output files byte for byte, the wrapping family included"""
    gold = np.load(os.path.join(golden_dir, "streamfilter.npz"))
    names = sorted(k[8:] for k in gold.files if k.startswith("geq_pcm_"))
    assert "loud" in names and len(names) == 6
    pcm = np.stack([gold["geq_pcm_" + k] for k in names])
    want = np.stack([gold["geq_out_" + k] for k in names])
    g = eng.geq(len(names))
    out, pre = g.process(pcm, want_precast=True)
    for i, k in enumerate(names):
        assert out[i].tobytes() == want[i].tobytes(), k
    assert np.abs(pre[names.index("loud")]).max() > 32768            # the last section alone wraps there
    g.close()


def test_geq_call_cuts_state_and_reset(eng):
    n_streams, n = 9, 1000
    pcm = geq_pool()
    w_out, w_pre, w_state = geq_want(7, n)
    g = eng.geq(n_streams)
    cuts = [0, 1, 7, 13, 512, 513, n]
    parts = [g.process(pcm[:, a:b], want_precast=True) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1), w_out)
    assert np.array_equal(np.concatenate([p[1] for p in parts], axis=1), w_pre)
    assert np.array_equal(g.state(), w_state)
    # get_state -> new handle -> set_state continues identically
    g.reset()
    assert not g.state().any()
    head = g.process(pcm[:, :300])
    st = g.state()
    assert np.array_equal(st, geq_want(7, 300)[2])
    g2 = eng.geq(n_streams)
    g2.set_state(st)
    tail = g2.process(pcm[:, 300:])
    assert np.array_equal(np.concatenate([head, tail], axis=1), w_out)
    assert np.array_equal(g2.state(), w_state)
    # reset: the zero keep again
    g2.reset()
    assert not g2.state().any()
    assert np.array_equal(g2.process(pcm), w_out)
    g.close()
    g2.close()


def test_geq_streams_do_not_see_their_neighbours(eng):
    """the same PCM at different stream indices, beside different neighbours"""
    n = 512
    pool = geq_pool()[:, :n]
    w_out = geq_want(7, n)[0]
    order_a = [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 1]
    order_b = [8, 0, 7, 1, 0, 2, 0, 6, 1, 5, 0, 4, 3, 0, 1, 1, 2, 0]
    for order in (order_a, order_b):
        g = eng.geq(len(order))
        out = g.process(np.ascontiguousarray(pool[order]))
        assert np.array_equal(out, w_out[order])
        g.close()


# ---- NLMS ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nlms_pool():
    """five (input, reference) pairs of 3000 samples"""
    n = 3000
    z = R.white(205, n, 300.0)
    pairs = [R.echo_pair(201, n), R.echo_pair(202, n, 9000.0, noise=100.0), (R.full_scale(203, n), R.full_scale(204, n)),
             (R.impulse(n), z), R.echo_pair(206, n, 4000.0, taps=60)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@functools.lru_cache(maxsize=None)
def nlms_want(L):
    """order="device" restatement of the pool, run in segments that end at every tested length:
    (est, err, precast) [5, 3000] and {n: (coefficients [5, L], keep [5, L - 1])}"""
    x, ref = nlms_pool()
    outs, states = [], {n: [] for n in NLMS_SAMPLES}
    for s in range(len(x)):
        st, seg, a = None, [], 0
        for b in NLMS_SAMPLES:
            est, err, pre, st = R.nlms(x[s, a:b], ref[s, a:b], L, state=st, order="device")
            seg.append((est, err, pre))
            states[b].append(st)
            a = b
        outs.append([np.concatenate([p[i] for p in seg]) for i in range(3)])
    return (tuple(np.stack([o[i] for o in outs]) for i in range(3)),
            {n: (np.stack([s[0] for s in v]), np.stack([s[1] for s in v])) for n, v in states.items()})


@pytest.mark.parametrize("L", [64, 128, 256])
def test_nlms_equals_the_device_order_restatement(eng, L):
    import torch
    x, ref = nlms_pool()
    (w_est, w_err, w_pre), w_state = nlms_want(L)
    for n_streams in (1, 3, 5):
        f = eng.nlms(n_streams, L)
        for n in NLMS_SAMPLES:
            xs, rs = np.ascontiguousarray(x[:n_streams, :n]), np.ascontiguousarray(ref[:n_streams, :n])
            f.reset()
            est, err, pre = f.process(xs, rs, want_precast=True)
            assert np.array_equal(est, w_est[:n_streams, :n]), (n_streams, n, np.argwhere(est != w_est[:n_streams, :n])[:4])
            assert np.array_equal(err, w_err[:n_streams, :n]), (n_streams, n)
            assert np.array_equal(pre, w_pre[:n_streams, :n]), (n_streams, n, np.argwhere(pre != w_pre[:n_streams, :n])[:4])
            cf, kp = f.state()
            assert np.array_equal(cf, w_state[n][0][:n_streams]), (n_streams, n)
            assert np.array_equal(kp, w_state[n][1][:n_streams]), (n_streams, n)
            if n in (255, 1025):                                 # device tensors, no pre-cast output
                f.reset()
                est, err = f.process(torch.from_numpy(xs).cuda(), torch.from_numpy(rs).cuda())
                torch.cuda.synchronize()
                assert np.array_equal(est.cpu().numpy(), w_est[:n_streams, :n])
                assert np.array_equal(err.cpu().numpy(), w_err[:n_streams, :n])
                assert np.array_equal(f.state()[0], w_state[n][0][:n_streams])
        f.close()


def test_nlms_call_cuts_and_state_round_trip(eng):
    x, ref = nlms_pool()
    n = 1025
    (w_est, w_err, w_pre), w_state = nlms_want(256)
    f = eng.nlms(5)
    cuts = [0, 1, 255, 1024, n]
    parts = [f.process(x[:, a:b], ref[:, a:b], want_precast=True) for a, b in zip(cuts, cuts[1:])]
    for i, w in enumerate((w_est, w_err, w_pre)):
        assert np.array_equal(np.concatenate([p[i] for p in parts], axis=1), w[:, :n])
    cf, kp = f.state()
    assert np.array_equal(cf, w_state[n][0]) and np.array_equal(kp, w_state[n][1])
    # state -> new handle -> the stream goes on identically
    f2 = eng.nlms(5)
    f2.set_state(cf, kp)
    est, err = f2.process(x[:, n:], ref[:, n:])
    assert np.array_equal(est, w_est[:, n:]) and np.array_equal(err, w_err[:, n:])
    assert np.array_equal(f2.state()[0], w_state[3000][0])
    f2.reset()
    cf, kp = f2.state()
    assert not cf.any() and not kp.any()
    f.close()
    f2.close()


def test_nlms_golden_streams(eng, golden_dir):
    """the compiled reference's est / err files byte for byte (it writes from its second block on)"""
    gold = np.load(os.path.join(golden_dir, "streamfilter.npz"))
    names = sorted(k[8:] for k in gold.files if k.startswith("nlms_in_"))
    assert len(names) == 6
    f = eng.nlms(len(names))
    est, err = f.process(np.stack([gold["nlms_in_" + k] for k in names]), np.stack([gold["nlms_ref_" + k] for k in names]))
    for i, k in enumerate(names):
        assert est[i, R.NLMS_BLOCK:].tobytes() == gold["nlms_est_" + k].tobytes(), k
        assert err[i, R.NLMS_BLOCK:].tobytes() == gold["nlms_err_" + k].tobytes(), k
    f.close()


def test_nlms_streams_do_not_see_their_neighbours(eng):
    x, ref = nlms_pool()
    n = 600
    (w_est, w_err, _), _ = nlms_want(256)
    for order in ([0, 1, 2, 3, 4, 0], [4, 0, 0, 3, 1, 0, 2]):
        f = eng.nlms(len(order))
        est, err = f.process(np.ascontiguousarray(x[order, :n]), np.ascontiguousarray(ref[order, :n]))
        assert np.array_equal(est, w_est[order, :n]) and np.array_equal(err, w_err[order, :n])
        f.close()


# ---- errors --------------------------------------------------------------------------------------------------------
def raises_einval(fn):
    import jeicyboodsp_amd
    with pytest.raises(jeicyboodsp_amd.JdspError) as ei:
        fn()
    assert ei.value.code == EINVAL and len(str(ei.value)) > len("jdsp error -1: "), str(ei.value)


def test_bad_arguments_are_einval_with_a_message(eng):
    import torch
    from jeicyboodsp_amd.engine import L
    ok = R.geq_design()
    raises_einval(lambda: eng.geq(4, np.zeros((0, 2, 3))))
    raises_einval(lambda: eng.geq(4, R.stable_sections(17)))
    raises_einval(lambda: eng.geq(0))
    raises_einval(lambda: eng.geq(-3, ok))
    for bad in (np.nan, np.inf):
        c = ok.copy()
        c[3, 0, 1] = bad
        raises_einval(lambda: eng.geq(2, c))
    c = ok.copy()
    c[5] = [[32764.0, -1.0, 1.0], [0.0, 1.0, -1.0]]            # the five |coefficients| sum to 2^15 exactly (integers: no rounding)
    assert np.abs(c[5]).sum() == 32768.0
    raises_einval(lambda: eng.geq(2, c))
    c[5, 0, 0] = 40000.0
    raises_einval(lambda: eng.geq(2, c))
    c[5, 0, 0] = 32763.5                                       # just below the bound: accepted ([k][1][0] is not counted)
    c[5, 1, 0] = 1e9
    eng.geq(2, c).close()
    for bad_len in (0, 63, 96, 512):
        raises_einval(lambda: eng.nlms(2, bad_len))
    raises_einval(lambda: eng.nlms(0))
    raises_einval(lambda: eng.nlms(2, 256, mu=np.nan))
    raises_einval(lambda: eng.nlms(2, 256, compensation=np.inf))

    # a bad pitch or alignment: -1, a message, and nothing written
    g, f = eng.geq(2), eng.nlms(2, 64)
    buf = torch.zeros((2, 64), dtype=torch.int16, device="cuda")
    out = torch.full((2, 64), 5, dtype=torch.int16, device="cuda")
    out2 = torch.full((2, 64), 5, dtype=torch.int16, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    eng._use_torch_stream()
    geq_calls = [(p(buf), 8, 12, p(out), None), (p(buf), 16, 8, p(out), None), (p(buf), -1, 16, p(out), None),
                 (p(buf, 2), 16, 16, p(out), None), (p(buf), 16, 16, p(out, 6), None), (None, 16, 16, p(out), None)]
    for a in geq_calls:
        assert L.jdsp_geq_process_dev(g._h, *a) == EINVAL, a
        assert L.jdsp_last_error(eng._h)
    nlms_calls = [(p(buf), p(buf), 16, 20, p(out), p(out2), None), (p(buf), p(buf), 32, 24, p(out), p(out2), None),
                  (p(buf), p(buf, 2), 16, 16, p(out), p(out2), None), (p(buf), p(buf), 16, 16, p(out), p(out2, 8), None),
                  (p(buf), p(buf), 16, 16, None, p(out2), None)]
    for a in nlms_calls:
        assert L.jdsp_nlms_process_dev(f._h, *a) == EINVAL, a
        assert L.jdsp_last_error(eng._h)
    torch.cuda.synchronize()
    assert bool((out == 5).all()) and bool((out2 == 5).all())
    assert not g.state().any() and not f.state()[0].any()
    g.close()
    f.close()
