"""GPU tests of the live n-microphone MVDR streams (jdsp_mvdrn_streams_reserve / _streams_dev / _streams /
_streams_reset_dev / _streams_state, MvdrMulti.open_streams / process_streams): a stream delivered in ragged chunks over
many calls comes out as the oracle's stream of all its blocks, and -- what the header promises bit for bit -- as the
same bytes however it is cut, wherever it stands and whoever stands beside it.  The scenes, cuts and comparisons are
tests/mvdrn_streams_cases.py's; tests/test_mvdrn_streams_cpu.py shows that they are not vacuous."""
import ctypes as C

import numpy as np
import pytest

import mvdrn_batch_cases as K
import mvdrn_streams_cases as S
from mvdrn_batch_cases import B

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def lib():
    from jeicyboodsp_amd.engine import L
    return L


def last_error(eng):
    return lib().jdsp_last_error(eng._h).decode()


def vp(t):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr()) if hasattr(t, "data_ptr") else t.ctypes.data_as(C.c_void_p)


def handle(eng, n_mics=3, n_streams=6, cap=128, loading=K.LOADING):
    m = eng.mvdr_multi(n_mics, K.delays_of(n_mics), loading)
    m.open_streams(n_streams, cap)
    return m


def state(m, ids):
    seen, cov = m.streams_state(ids, want_cov=True)
    return seen.tolist(), cov.tobytes()


# ---- 1. the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["dev", "host"])
@pytest.mark.parametrize("n_mics", S.ORACLE_MICS)
def test_every_stream_matches_the_oracle_on_all_its_blocks(eng, oracle, n_mics, entry):
    streams = S.oracle_streams(n_mics)
    plan = S.random_plan(11 + n_mics, S.ORACLE_TOTALS, 7)
    m = handle(eng, n_mics, n_streams=5, cap=64)
    got = S.deliver(m, streams, plan, entry, gaps=True)
    worst = max(S.check_oracle(oracle, x, got[s]) for s, x in enumerate(streams))
    assert m.streams_state(range(5)).tolist() == S.ORACLE_TOTALS
    print("n_mics %d, %s entry: worst precast error %.3f of the 1e-5 bar" % (n_mics, entry, worst))
    m.close()


def test_only_the_spans_are_written_and_never_a_lifes_first_block(eng):
    import torch
    from jeicyboodsp_amd.sharding import mvdrn_stream_written
    streams = [S.scene(700 + s, 3, n) for s, n in enumerate([4, 1, 6, 2])]
    m = handle(eng, 3, n_streams=4, cap=16)
    L, seen = lib(), [0] * 4
    for call in ([(2, 3), (0, 0), (1, 1)], [(1, 0), (3, 2), (2, 3), (0, 4)]):
        chunks = [streams[s][:, seen[s] * B:(seen[s] + n) * B] for s, n in call]
        pcm, counts, first = K.pack(chunks, gaps=[6, 2, 2, 10][:len(call)], pad=16)
        n, total = pcm.shape[1], int(counts.sum())
        arrays = [torch.from_numpy(np.ascontiguousarray(a, np.int64)).cuda()
                  for a in ([s for s, _ in call], first, np.concatenate([[0], np.cumsum(counts)]))]
        d_pcm = torch.from_numpy(pcm).cuda()
        out = torch.full((n,), 0x5A5A, dtype=torch.int16, device="cuda")
        pre = torch.full((n,), -12345.5, dtype=torch.float32, device="cuda")
        eng._use_torch_stream()
        assert L.jdsp_mvdrn_streams_dev(m._h, vp(d_pcm), n, vp(arrays[0]), vp(arrays[1]), vp(arrays[2]), len(call), total,
                                        vp(out), vp(pre), None) == 0
        torch.cuda.synchronize()
        keep = np.ones(n, bool)
        skip = mvdrn_stream_written([seen[s] for s, _ in call], counts)
        for (s, nb), a, k in zip(call, first, skip):
            keep[int(a) + int(k) * B:int(a) + nb * B] = False
            seen[s] += nb
        out, pre = out.cpu().numpy(), pre.cpu().numpy()
        assert np.all(out[keep] == 0x5A5A) and np.all(pre[keep] == np.float32(-12345.5))
        assert not np.any(pre[~keep] == np.float32(-12345.5))  # and every other sample of the spans is written
        assert np.count_nonzero(~keep) == (total - int(skip.sum())) * B
    m.close()


# ---- 2. cuts, as bytes ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cut_base(eng, oracle):
    """the 40-block stream in one chunk: what every other delivery of it is compared with, itself held to the oracle"""
    x = S.cut_stream()
    m = handle(eng)
    res = S.deliver(m, [x], S.plan_of([40]))[0]
    S.check_oracle(oracle, x, res)
    st = state(m, [0])
    m.close()
    return x, res, st


@pytest.mark.parametrize("entry", ["dev", "host"])
@pytest.mark.parametrize("cuts", ["each", "random", "between"])
def test_bits_do_not_depend_on_the_cuts(eng, cut_base, cuts, entry):
    x, want, want_state = cut_base
    sizes = {"each": S.cuts_each(40), "random": S.cuts_random(5, 40), "between": [S.CUT_AT, 40 - S.CUT_AT]}[cuts]
    m = handle(eng)
    if cuts == "each":                                         # a first call of exactly one block emits nothing
        first = S.deliver(m, [x], S.plan_of([1]), entry)[0]
        assert not first[0].any() and not first[1].any() and m.streams_state([0]).tolist() == [1]
        m.reset_streams([0])
    got = S.deliver(m, [x], S.plan_of(sizes), entry)[0]
    assert S.same_bytes(got, want), (cuts, entry)
    assert state(m, [0]) == want_state
    m.close()


# ---- 3. independence ----------------------------------------------------------------------------------------------------
OTHERS = [20, 9, 0, 33]                                       # the four streams beside the one that is compared


def test_bits_do_not_depend_on_the_company_the_order_the_id_or_the_layout(eng, cut_base):
    x, want, want_state = cut_base
    streams = {0: x}
    streams.update({s + 1: S.scene(500 + s, 3, n) for s, n in enumerate(OTHERS)})
    plan = S.random_plan(3, [40] + OTHERS, 6)
    alone = [[c for c in call if c[0] == 0] for call in plan]
    m = handle(eng)
    assert S.same_bytes(S.deliver(m, streams, alone)[0], want), "alone, in the plan's cuts"
    before = state(m, [1, 2, 3, 4, 5])
    assert before[0] == [0] * 5 and not any(before[1])         # the absent streams: untouched and fresh
    m.reset_streams()
    among = S.deliver(m, streams, plan)
    assert S.same_bytes(among[0], want), "among four others"
    assert state(m, [0]) == want_state
    others_state = state(m, [1, 2, 3, 4])
    m.reset_streams()
    got = S.deliver(m, streams, [call[::-1] for call in plan])
    assert all(S.same_bytes(got[s], among[s]) for s in streams), "chunk order reversed"
    assert state(m, [1, 2, 3, 4]) == others_state
    m.reset_streams()
    ids = {0: 4, 1: 0, 2: 5, 3: 2, 4: 1}
    got = S.deliver(m, streams, plan, ids=ids)
    assert all(S.same_bytes(got[s], among[s]) for s in streams), "under other ids"
    assert state(m, [4]) == want_state and state(m, [3]) == ([0], bytes(513 * 64 * 16))
    m.close()
    m = handle(eng, n_streams=11)
    got = S.deliver(m, streams, plan, ids={s: 2 * s + 1 for s in streams}, gaps=True, stride_pad=64)
    assert all(S.same_bytes(got[s], among[s]) for s in streams), "another n_streams, gaps, another chan_stride"
    assert state(m, [1]) == want_state
    # a stream without a chunk in a call stays as it is: deliver to stream 3 only, the rest keep their state
    rest = state(m, [1, 5, 7, 9])
    S.deliver(m, {1: S.scene(9, 3, 5)}, [[(1, 5)]], ids={1: 3})
    assert state(m, [1, 5, 7, 9]) == rest
    m.close()


# ---- 4. against the batch -----------------------------------------------------------------------------------------------
def batch_of(eng, x):
    import torch
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    res = m.process_batch(torch.from_numpy(x).cuda(), [x.shape[1] // B], want_precast=True, want_flags=True)
    torch.cuda.synchronize()
    m.close()
    return tuple(r.cpu().numpy() for r in res)


@pytest.mark.parametrize("n_events", S.BATCH_EQUAL)
def test_bits_equal_the_batch_up_to_128_estimation_frames(eng, n_events):
    x = K.events_run(300 + n_events, n_events)
    n = x.shape[1] // B
    m = handle(eng, cap=8)
    got = S.deliver(m, [x], S.plan_of(S.cuts_of(n, 5)))[0]
    assert S.same_bytes(got, batch_of(eng, x)), n_events
    m.close()


def test_beyond_128_estimation_frames_the_walk_goes_on_one_by_one(eng, oracle):
    for n_events, how in sorted(S.BATCH_BARS.items()):
        x = K.events_run(300 + n_events, n_events)
        n = x.shape[1] // B
        cuts = [50, 1, n - 51] if n_events == 130 else S.cuts_of(n, 64)
        m = handle(eng, cap=max(cuts))
        got = S.deliver(m, [x], S.plan_of(cuts))[0]
        worst = S.check_oracle(oracle, x, got)
        print("%d events, %s: worst %.3f of the bar; bits equal to the batch's: %s" % (
            n_events, how, worst, S.same_bytes(got, batch_of(eng, x))))
        if n_events == 130:                                     # the unbounded serial walk against one block per call
            st = state(m, [0])
            m.reset_streams()
            assert S.same_bytes(S.deliver(m, [x], S.plan_of(S.cuts_each(n)))[0], got)
            assert state(m, [0]) == st
        m.close()


# ---- 5. loading 0 -------------------------------------------------------------------------------------------------------
def test_loading_0_is_non_finite_until_the_third_estimation_frame_across_a_cut(eng, oracle):
    """On 3 microphones without loading the output is non-finite until 3 estimation frames have been seen, and the
    finite masks equal the oracle's, in one chunk and across a cut behind the second estimation frame: the third is then
    added to a carried rank-2 matrix, and the count of estimation frames is carried with it.  From the third on the
    samples meet the bars, and the cut gives the bytes of the one chunk, carried covariance included.

    The live kernels spell the rule out (mvdrn_live_kernels.hip: fewer than n_mics estimation frames at loading 0 means
    NaN weights).  Left to the elimination's rounding, as _process and the batch leave it, the block of the second
    estimation frame came out finite on an MI355X (512 of 512 samples, |x| up to 148) where the oracle's is NaN."""
    x = S.loading0_stream()
    held = np.repeat(np.arange(1, 12) >= 3, B)                 # emitted blocks from the third estimation frame (block 3) on
    _, o_pre = K.oracle_utt(oracle, x, 0.0)
    m = handle(eng, loading=0.0)
    res, states = [], []
    for cuts in ([12], [S.LOADING0_CUT, 12 - S.LOADING0_CUT], S.cuts_each(12)):
        m.reset_streams()
        res.append(S.deliver(m, [x], S.plan_of(cuts))[0])
        states.append(state(m, [0]))
        out, pre, flags = res[-1]
        print("cuts %s: finite samples per emitted block, stream %s, oracle %s" % (
            cuts, np.isfinite(pre[B:]).reshape(-1, B).sum(axis=1).tolist(), np.isfinite(o_pre).reshape(-1, B).sum(axis=1).tolist()))
        assert not np.isfinite(pre[B:3 * B]).any() and np.isfinite(pre[3 * B:]).all() and not out[:3 * B].any(), cuts
        assert np.array_equal(np.isfinite(pre[B:]), np.isfinite(o_pre)), cuts
        S.check_oracle(oracle, x, res[-1], 0.0, held)
    assert all(S.same_bytes(r, res[0]) for r in res) and all(st == states[0] for st in states)
    m.close()


# ---- 6. reset -----------------------------------------------------------------------------------------------------------
def test_reset_makes_the_listed_streams_fresh_and_leaves_the_others(eng, cut_base):
    x, want, want_state = cut_base
    y = S.scene(61, 3, 20)
    m = handle(eng)
    S.deliver(m, [x, y], [[(0, 13), (1, 7)]])
    m.reset_streams([1])
    assert state(m, [1]) == ([0], bytes(513 * 64 * 16))
    got = S.deliver(m, {0: x[:, 13 * B:], 1: y}, [[(1, 20), (0, 27)]])
    m2 = handle(eng)
    fresh = S.deliver(m2, [y], S.plan_of([20]))[0]
    m2.close()
    assert S.same_bytes(got[1], fresh)                          # the reset one starts again from its block 0 ...
    assert tuple(a[13 * B:].tobytes() for a in want[:2]) == tuple(a.tobytes() for a in got[0][:2])   # ... the other goes on
    assert state(m, [0]) == want_state
    m.reset_streams()                                           # NULL: all
    assert state(m, range(6)) == ([0] * 6, bytes(6 * 513 * 64 * 16))
    assert S.same_bytes(S.deliver(m, [x], S.plan_of([40]))[0], want)
    m.close()


# ---- 7. the handle's other entries ----------------------------------------------------------------------------------------
def test_process_and_a_batch_between_two_deliveries(eng, oracle, cut_base):
    x, want, want_state = cut_base
    a = K.array_scene(9, 3, 30, quiet=((2, 5), (14, 6)))[0]
    o_out, o_pre = oracle.mvdrn_stream(a, K.delays_of(3), K.LOADING)
    other = [K.utterance(900 + u, 3, n) for u, n in enumerate([6, 11])]
    pcm, counts, first = K.pack(other)
    m = handle(eng)
    batch_alone = m.process_batch(pcm, counts, first, want_precast=True, want_flags=True)
    o1, p1 = m.process(a[:, :12 * B], want_precast=True)
    part1 = S.deliver(m, [x], S.plan_of([17]))[0]
    batch_between = m.process_batch(pcm, counts, first, want_precast=True, want_flags=True)
    o2, p2 = m.process(a[:, 12 * B:], want_precast=True)
    part2 = S.deliver(m, [x[:, 17 * B:]], S.plan_of([23]))[0]
    assert S.same_bytes(tuple(np.concatenate(p) for p in zip(part1, part2)), want)
    assert state(m, [0]) == want_state
    assert S.same_bytes(batch_between, batch_alone)
    K.check(np.concatenate([o1, o2]), np.concatenate([p1, p2]), o_out, o_pre)
    m.close()
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)            # ... and the bits of the same two calls without the others
    q = [m.process(part, want_precast=True) for part in (a[:, :12 * B], a[:, 12 * B:])]
    assert [o1.tobytes(), o2.tobytes()] == [r[0].tobytes() for r in q]
    assert S.same_bytes((o1, p1, o1[:0]), q[0] + (o1[:0],)) and S.same_bytes((o2, p2, o2[:0]), q[1] + (o2[:0],))
    m.close()


# ---- 8. all outputs NULL --------------------------------------------------------------------------------------------------
def test_a_delivery_without_outputs_advances_the_state_all_the_same(eng, cut_base):
    x, want, want_state = cut_base
    m = handle(eng)
    S.deliver(m, [x], S.plan_of([9, 8]), outputs=False)
    assert m.streams_state([0]).tolist() == [17]
    got = S.deliver(m, [x[:, 17 * B:]], S.plan_of([23]))[0]
    assert tuple(a[17 * B:].tobytes() for a in want[:2]) == tuple(a.tobytes() for a in got[:2])
    assert got[2].tobytes() == want[2][17:].tobytes() and state(m, [0]) == want_state
    m.close()


# ---- 9. errors ------------------------------------------------------------------------------------------------------------
def test_512_point_handles_are_refused_by_every_entry(eng):
    L = lib()
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING, n_fft=512)
    for rc in (L.jdsp_mvdrn_streams_reserve(m._h, 4, 8), L.jdsp_mvdrn_streams_reset_dev(m._h, None, 0),
               L.jdsp_mvdrn_streams_dev(m._h, None, 0, None, None, None, 1, 2, None, None, None),
               L.jdsp_mvdrn_streams(m._h, None, 0, 0, None, None, None, 1, None, None, None),
               L.jdsp_mvdrn_streams_state(m._h, None, 0, None, None)):
        assert rc == EINVAL and "1024-point handles only" in last_error(eng)
    m.close()


def test_errors_leave_every_stream_as_it_was(eng):
    import torch
    L = lib()
    x = S.scene(950, 3, 10)
    chunks = [x[:, :4 * B], x[:, 4 * B:10 * B]]
    pcm, counts, first = K.pack(chunks, gaps=[2, 2])
    n = pcm.shape[1]
    block_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ids = np.array([1, 2], np.int64)
    d_pcm = torch.from_numpy(pcm).cuda()
    d_ids, d_s, d_b = (torch.from_numpy(a).cuda() for a in (ids, first, block_first))
    out = torch.zeros(n, dtype=torch.int16, device="cuda")
    h_out = np.zeros(n, np.int16)
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    eng._use_torch_stream()

    def dev(n_chunks=2, n_blocks=10, p=None):
        return L.jdsp_mvdrn_streams_dev(m._h, p or vp(d_pcm), n, vp(d_ids), vp(d_s), vp(d_b), n_chunks, n_blocks, vp(out),
                                        None, None)

    def host(i=ids, s=first, b=block_first, n_chunks=2, n_samples=n):
        i, s, b = (np.ascontiguousarray(a, np.int64) for a in (i, s, b))
        return L.jdsp_mvdrn_streams(m._h, vp(pcm), n, n_samples, vp(i), vp(s), vp(b), n_chunks, vp(h_out), None, None)
    for rc in (dev(), host(), L.jdsp_mvdrn_streams_reset_dev(m._h, None, 0),
               L.jdsp_mvdrn_streams_state(m._h, vp(ids), 2, None, None)):
        assert rc == EINVAL and "jdsp_mvdrn_streams_reserve" in last_error(eng)            # before any reserve
    m.open_streams(3, 10)
    S.deliver(m, {1: S.scene(951, 3, 6)}, [[(1, 6)]])
    before = state(m, [0, 1, 2])
    assert before[0] == [0, 6, 0]
    assert dev(n_chunks=4) == EINVAL and "more chunks than live streams" in last_error(eng)
    assert dev(n_blocks=11) == EINVAL and "jdsp_mvdrn_streams_reserve" in last_error(eng)
    assert dev(p=C.c_void_p(d_pcm.data_ptr() + 2)) == EINVAL and "aligned" in last_error(eng)
    assert dev(n_chunks=-1) == EINVAL
    assert host(i=[1, 1]) == EINVAL and "twice" in last_error(eng)
    assert host(i=[1, 3]) == EINVAL and "outside" in last_error(eng)
    assert host(s=first[::-1]) == EINVAL
    assert host(s=first + [1, 0]) == EINVAL and "even" in last_error(eng)
    assert host(s=[first[0], first[0] + 2 * B]) == EINVAL and "overlap" in last_error(eng)
    assert host(n_samples=int(first[1]) + 6 * B - 2) == EINVAL
    assert host(b=block_first + 1) == EINVAL and "block_first[0]" in last_error(eng)
    assert host(b=np.array([0, 4, 11]), n_samples=n) == EINVAL
    torch.cuda.synchronize()
    assert state(m, [0, 1, 2]) == before
    assert host() == 0 and dev(n_chunks=0, n_blocks=0) == 0 and dev(n_chunks=2, n_blocks=0) == 0
    assert state(m, [0, 1, 2])[0] == [0, 10, 6]
    m.close()
