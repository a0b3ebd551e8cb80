"""GPU: the live n-microphone MVDR streams (jdsp_mvdrn_streams*, csrc/mvdrn_live_kernels.hip, mvdrn_live_api.hip) on
what the white array scene of tests/test_mvdrn_streams_gpu.py does not reach -- the scenes of tests/mvdrn_cases.py
(fractional, positive, far and absent steering, covariances near rank 1, with steep spectra, a loud bin 0 and seven
decades on the diagonal, a loud microphone beside a quiet one) at loadings 1e-3, 1e-6, 0 and 1, delivered among company
and cut where a stream carries something of its own; the carried covariance against the FP64 restatement, not only
against itself; and the loading-0 rule on 2, 5 and 8 microphones, 8 being where the carried count saturates.  The cases
are tests/mvdrn_streams_hard_cases.py's; tests/test_mvdrn_streams_hard_cpu.py shows that they are not vacuous and says
why nothing here compares the oracle's finite mask in front of the n_mics-th estimation frame.  Run with -s for the
shares of the bars (profiles/r27_mvdrn_streams_hard.txt holds them)."""
import numpy as np
import pytest

import mvdrn_batch_cases as K
import mvdrn_cases as H
import mvdrn_streams_cases as S
import mvdrn_streams_hard_cases as X
from mvdrn_batch_cases import B
from test_mvdrn_hard_gpu import batch_groups, oracle_case      # and with them its oracle cache, one per session

pytestmark = pytest.mark.gpu
HOST_GROUP = "steering_frac"                                  # the steering group that goes through the host entry


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def state(m, ids):
    seen, cov = m.streams_state(ids, want_cov=True)
    return seen.tolist(), cov.tobytes()


def alone(eng, n_mics, delays, loading, pcm):
    """(result, state) of one stream delivered alone as one chunk of all its blocks"""
    n = pcm.shape[1] // B
    m = eng.mvdr_multi(n_mics, delays, loading)
    m.open_streams(1, n)
    res = S.deliver(m, [pcm], S.plan_of([n]))[0]
    st = state(m, [0])
    m.close()
    return res, st


def batch_of(eng, n_mics, delays, loading, pcm):
    import torch
    m = eng.mvdr_multi(n_mics, delays, loading)
    res = m.process_batch(torch.from_numpy(np.array(pcm)).cuda(), [pcm.shape[1] // B], want_precast=True, want_flags=True)
    torch.cuda.synchronize()
    m.close()
    return tuple(r.cpu().numpy() for r in res)


def same_on(a, b, held):
    """out, and the finite precast samples, of two results equal as bytes on the held emitted samples"""
    fa, fb = np.isfinite(a[1][B:])[held], np.isfinite(b[1][B:])[held]
    return (a[0][B:][held].tobytes() == b[0][B:][held].tobytes() and np.array_equal(fa, fb) and
            a[1][B:][held][fa].tobytes() == b[1][B:][held][fb].tobytes())


# ---- 1. the hard scenes among company -------------------------------------------------------------------------------------
@pytest.mark.parametrize("loading", H.LOADINGS)
@pytest.mark.parametrize("n_mics", H.N_MICS)
def test_hard_scenes_as_concurrent_streams_hold_the_bar_and_their_own_bytes(eng, oracle, n_mics, loading):
    """All scenes of one steering as the live streams of one handle, dealt over six ragged calls with gaps: each against
    the oracle at the header's bars (at loading 0 from its n_mics-th estimation frame on, H.held_mask), as bytes and as
    state what it is delivered alone in one chunk, and as bytes what jdsp_mvdrn_batch makes of it as one utterance (12
    estimation frames: the header promises that up to 128)."""
    for g, names in enumerate(batch_groups(n_mics)):
        entry = "host" if HOST_GROUP in names else "dev"
        delays = H.cached_scene(names[0], n_mics)[1]
        streams = [H.cached_scene(name, n_mics)[0] for name in names]
        plan = S.random_plan(50 + 10 * g + n_mics, [X.N] * len(names), 6)
        m = eng.mvdr_multi(n_mics, delays, loading)
        m.open_streams(len(names), max(sum(n for _, n in call) for call in plan))
        got = S.deliver(m, streams, plan, entry, gaps=True)
        states = [state(m, [s]) for s in range(len(names))]
        m.close()
        for s, name in enumerate(names):
            out, pre, flags = got[s]
            o_out, o_pre, held = oracle_case(oracle, name, n_mics, loading, 1024)
            assert out.size == X.N * B and not out[:B].any() and not pre[:B].any(), name     # block 0 of its life: unwritten
            assert np.array_equal(flags, H.flags_of(oracle, streams[s], 1024)), name
            share = K.check(out[B:], pre[B:].astype(np.float64), o_out, o_pre, held)
            want, want_state = alone(eng, n_mics, delays, loading, streams[s])
            assert S.same_bytes(got[s], want), name
            assert states[s] == want_state and states[s][0] == [X.N], name
            batch = batch_of(eng, n_mics, delays, loading, streams[s])
            assert held.all() == (loading != 0), name
            assert same_on(got[s], batch, held) and flags.tobytes() == batch[2].tobytes(), name
            print("share of the bar %-16s mics %d loading %-6g live, %d streams, %s entry %.3f" % (
                name, n_mics, loading, len(names), entry, share))


# ---- 2. cuts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loading", X.CUT_LOADINGS)
@pytest.mark.parametrize("n_mics", H.N_MICS)
@pytest.mark.parametrize("name", X.CUT_SCENES)
def test_bits_and_state_do_not_depend_on_the_cuts(eng, oracle, name, n_mics, loading):
    """One block per call, X.edges (a chunk's block 0 that is the n_mics-th estimation frame, that is quiet behind a
    loud carried block, that is an estimation frame through the carried bit and block alone, that is loud behind a quiet
    one, and a chunk of 0 blocks) and random cuts against the scene in one chunk, itself held to the oracle."""
    pcm, delays, _ = H.cached_scene(name, n_mics)
    m = eng.mvdr_multi(n_mics, delays, loading)
    m.open_streams(1, X.N)
    want = S.deliver(m, [pcm], S.plan_of(X.cuts("whole", n_mics)))[0]
    want_state = state(m, [0])
    K.check(want[0][B:], want[1][B:].astype(np.float64), *oracle_case(oracle, name, n_mics, loading, 1024))
    for kind in ("each", "edges", "random"):
        m.reset_streams()
        got = S.deliver(m, [pcm], S.plan_of(X.cuts(kind, n_mics)))[0]
        assert S.same_bytes(got, want), kind
        assert state(m, [0]) == want_state, kind
    m.close()


# ---- 3. the carried covariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mics", H.N_MICS)
@pytest.mark.parametrize("name", H.SCENES)
def test_the_carried_covariance_is_ref64s(eng, name, n_mics):
    """streams_state's covariance against the FP64 restatement's R at X.cov_bar (4 x plain FP32's own figure): at the
    end of the scene in one chunk, and under X.edges after the chunk that ends with block 8 -- the first pause, the
    n_mics-th event taken from the carried block -- and at the end.  Row, column as the header says, the scale 1 / 1024,
    nothing past n_mics, real diagonals and Hermitian bit for bit (X.check_cov)."""
    pcm, delays, _ = H.cached_scene(name, n_mics)
    bar = X.cov_bar(name, n_mics)
    m = eng.mvdr_multi(n_mics, delays, 1e-3)
    m.open_streams(2, X.N)
    shares = {}
    S.deliver(m, {1: pcm}, S.plan_of(X.cuts("whole", n_mics), 1))
    seen, cov = m.streams_state([1, 0], want_cov=True)
    assert seen.tolist() == [X.N, 0] and not cov[1].any()       # the stream beside it: fresh
    shares["whole"] = X.check_cov(cov[0], X.cov_ref64(name, n_mics), n_mics, bar)
    sizes = X.edges(n_mics)
    k = X.calls_upto(sizes, X.FIRST_PAUSE - 1)
    S.deliver(m, [pcm], S.plan_of(sizes[:k]))
    seen, mid = m.streams_state([0], want_cov=True)
    assert seen.tolist() == [X.FIRST_PAUSE]
    shares["edges, after block 8"] = X.check_cov(mid[0], X.cov_ref64(name, n_mics, X.FIRST_PAUSE), n_mics, bar)
    S.deliver(m, [pcm[:, X.FIRST_PAUSE * B:]], S.plan_of(sizes[k:]))
    seen, end = m.streams_state([0], want_cov=True)
    assert seen.tolist() == [X.N]
    shares["edges, at the end"] = X.check_cov(end[0], X.cov_ref64(name, n_mics), n_mics, bar)
    assert end.tobytes() == cov[:1].tobytes()                   # and the two deliveries carry the same bytes
    m.close()
    print("share of the covariance bar %-16s mics %d bar %.3g  %s" % (
        name, n_mics, bar, "  ".join("%s %.3f" % kv for kv in shares.items())))


# ---- 4. the rule at loading 0 -------------------------------------------------------------------------------------------------
def check_rule(oracle, x, res, n_mics):
    """emitted blocks 1 .. n_mics - 1 wholly non-finite in precast and 0 in out, every later block wholly finite, and on
    those the oracle's bars.  The oracle's mask in front of the n_mics-th frame is chance and is not looked at."""
    out, pre, flags = res
    assert not out[:n_mics * B].any() and not pre[:B].any()
    assert not np.isfinite(pre[B:n_mics * B]).any() and np.isfinite(pre[n_mics * B:]).all()
    assert np.array_equal(flags, K.oracle_flags(oracle, x))
    o_out, o_pre = K.oracle_utt(oracle, x, 0.0)
    return K.check(out[B:], pre[B:].astype(np.float64), o_out, o_pre, X.rule_held(flags, n_mics))


@pytest.mark.parametrize("n_mics", X.RULE_MICS)
def test_loading_0_is_non_finite_until_the_n_mics_th_estimation_frame_however_cut(eng, oracle, n_mics):
    """X.rule_stream in one chunk, cut so that the n_mics-th estimation frame opens the second chunk (n_mics - 1 carried
    in the count: 7 at 8 microphones, one short of where the word saturates, and 8, 9, 10 behind it), and one block per
    call: the rule, the bars from the n_mics-th frame on, and the same bytes and state from all three.  At 8 microphones
    also beside a second stream three blocks behind, so that the two counts differ in every call."""
    x = X.rule_stream(n_mics)
    n = n_mics + 9
    m = eng.mvdr_multi(n_mics, K.delays_of(n_mics), 0.0)
    m.open_streams(2, 2 * n)
    res, states = {}, {}
    for kind, sizes in X.rule_plans(n_mics).items():
        m.reset_streams()
        res[kind] = S.deliver(m, [x], S.plan_of(sizes))[0]
        states[kind] = state(m, [0])
        share = check_rule(oracle, x, res[kind], n_mics)
        print("rule stream, %d microphones, %-5s: finite samples per emitted block %s, %.3f of the bar" % (
            n_mics, kind, np.isfinite(res[kind][1][B:]).reshape(-1, B).sum(axis=1).tolist(), share))
    if n_mics == 8:
        y = X.rule_stream(n_mics, 191)
        m.reset_streams()
        got = S.deliver(m, [x, y], X.rule_pair_plan(n))
        res["beside a later stream"], states["beside a later stream"] = got[0], state(m, [0])
        check_rule(oracle, y, got[1], n_mics)
        later = state(m, [1])
        m.reset_streams()
        assert S.same_bytes(S.deliver(m, {1: y}, S.plan_of([n], 1))[1], got[1]) and state(m, [1]) == later
    assert all(S.same_bytes(r, res["whole"]) for r in res.values()), n_mics
    assert all(st == states["whole"] and st[0] == [n] for st in states.values()), n_mics
    m.close()
