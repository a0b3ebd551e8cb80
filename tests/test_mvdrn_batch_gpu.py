"""GPU tests of the batched n-microphone MVDR (jdsp_mvdrn_batch_reserve / _batch_dev / _batch, MvdrMulti.process_batch):
every utterance of a ragged batch comes out as a fresh handle's process of it alone.  Each utterance is checked against
oracle.mvdrn_stream on it alone at the bars of tests/test_mvdr_multi_gpu.py (mvdrn_batch_cases.check); what the header
promises bit for bit -- independence of place, neighbours, gaps, chan_stride and the split into calls -- is checked
with byte equality."""
import ctypes as C

import numpy as np
import pytest

import mvdrn_batch_cases as K
from mvdrn_batch_cases import B, P

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


def run(m, pcm, counts, sample_first, entry="dev"):
    """(out, precast, flags) as numpy, through the device entry (torch) or the host entry (numpy)"""
    if entry == "host":
        return m.process_batch(pcm, counts, sample_first, want_precast=True, want_flags=True)
    import torch
    res = m.process_batch(torch.from_numpy(pcm).cuda(), counts, sample_first, want_precast=True, want_flags=True)
    torch.cuda.synchronize()
    return tuple(r.cpu().numpy() for r in res)


def per_utt(res, counts, sample_first):
    """the bytes of every utterance's own results: (out, precast, flags) of its emitted blocks"""
    out, pre, flags = res
    first = np.concatenate([[0], np.cumsum(counts)])
    return [(K.span_of(out, int(s), int(n)).tobytes(), K.span_of(pre, int(s), int(n)).tobytes(),
             flags[first[u]:first[u + 1]].tobytes()) for u, (n, s) in enumerate(zip(counts, sample_first))]


# ---- the oracle, utterance by utterance --------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["dev", "host"])
@pytest.mark.parametrize("n_mics", K.N_MICS)
def test_every_utterance_matches_its_own_oracle(eng, oracle, n_mics, entry):
    utts = K.oracle_batch_utts(n_mics)
    pcm, counts, first = K.pack(utts)
    assert counts.tolist() == K.COUNTS
    m = eng.mvdr_multi(n_mics, K.delays_of(n_mics), K.LOADING)
    out, pre, flags = run(m, pcm, counts, first, entry)
    assert out.shape == (pcm.shape[1],) and pre.shape == out.shape and flags.shape == (sum(K.COUNTS),)
    worst = K.check_batch(oracle, utts, first, out, pre, flags)
    print("n_mics %d, %s entry: worst precast error %.3f of the 1e-5 bar" % (n_mics, entry, worst))
    m.close()


def test_the_boundary_takes_nothing_across(eng, oracle):
    """A ends in two quiet blocks, B starts with two: as one stream B's first block would be an estimation frame and
    its first frame would read A's last block (tests/test_mvdrn_batch_cpu.py: 6.6 % of the peak apart)."""
    a, b = K.boundary_pair()
    pcm, counts, first = K.pack([a, b])
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    for entry in ("dev", "host"):
        out, pre, flags = run(m, pcm, counts, first, entry)
        K.check_batch(oracle, [a, b], first, out, pre, flags)
        assert flags.tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1]
        # B's block 0 emits nothing and, with no estimate of its own yet, neither does A's covariance speak for it: B's
        # block 1 is B's first estimation frame, so every emitted sample of B is finite and equals B alone
        alone = run(m, b, counts[1:], first[:1], entry)
        assert per_utt((out, pre, flags), counts, first)[1] == per_utt(alone, counts[1:], first[:1])[0]
    m.close()


# ---- independence, bit for bit -----------------------------------------------------------------------------------------
IND_COUNTS = [5, 12, 0, 9, 20, 1, 2]


def ind_utts(n_mics=3):
    utts = [K.utterance(500 + u, n_mics, n) for u, n in enumerate(IND_COUNTS)]
    utts[3] = K.utterance(503, n_mics, 9, quiet=())            # a loud neighbour: no estimation frame at all
    return utts


@pytest.fixture(scope="module")
def ind_base(eng, oracle):
    """the batch every independence case is compared with, itself checked against the oracle"""
    utts = ind_utts()
    pcm, counts, first = K.pack(utts)
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    res = run(m, pcm, counts, first)
    K.check_batch(oracle, utts, first, *res)
    m.close()
    return utts, per_utt(res, counts, first)


@pytest.mark.parametrize("entry", ["dev", "host"])
def test_bits_do_not_depend_on_the_order_or_the_gaps(eng, ind_base, entry):
    utts, want = ind_base
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    order = [4, 2, 0, 6, 3, 5, 1]
    pcm, counts, first = K.pack([utts[i] for i in order])
    got = per_utt(run(m, pcm, counts, first, entry), counts, first)
    assert [got[order.index(u)] for u in range(len(utts))] == want
    gaps = [2, 6, 10, 2, 14, 6, 1026]
    assert all(g % 4 == 2 for g in gaps)                       # odd multiples of 2 samples: spans 4-byte aligned and no more
    pcm, counts, first = K.pack(utts, gaps=gaps)
    assert per_utt(run(m, pcm, counts, first, entry), counts, first) == want
    m.close()


@pytest.mark.parametrize("cuts", [(3,), (2, 5)], ids=["two-calls", "three-calls"])
def test_bits_do_not_depend_on_the_split_into_calls(eng, ind_base, cuts):
    utts, want = ind_base
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    got, lo = [], 0
    for hi in list(cuts) + [len(utts)]:
        pcm, counts, first = K.pack(utts[lo:hi])
        got += per_utt(run(m, pcm, counts, first), counts, first)
        lo = hi
    assert got == want
    m.close()


def test_bits_do_not_depend_on_chan_stride(eng, ind_base):
    import torch
    utts, want = ind_base
    pcm, counts, first = K.pack(utts)
    n = pcm.shape[1]
    wide = torch.full((3, n + 24), 7777, dtype=torch.int16, device="cuda")
    wide[:, :n] = torch.from_numpy(pcm).cuda()
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    view = wide[:, :n]
    assert view.stride(0) == n + 24 and not view.is_contiguous()
    res = m.process_batch(view, counts, first, want_precast=True, want_flags=True)
    torch.cuda.synchronize()
    assert per_utt(tuple(r.cpu().numpy() for r in res), counts, first) == want
    m.close()


def test_bits_do_not_depend_on_a_neighbour(eng, ind_base):
    utts, want = ind_base
    silent = list(utts)
    silent[3] = np.zeros_like(utts[3])                         # the loud neighbour replaced by silence
    pcm, counts, first = K.pack(silent)
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    got = per_utt(run(m, pcm, counts, first), counts, first)
    assert [g for u, g in enumerate(got) if u != 3] == [w for u, w in enumerate(want) if u != 3]
    assert got[3] != want[3]
    m.close()


def test_a_singular_utterance_without_loading_leaves_its_neighbours_alone(eng, oracle):
    """loading = 0 and 4 microphones: an utterance with 2 estimation frames has a rank-deficient matrix in every bin, so
    its weights are non-finite or meaningless on both sides.  Pinned: nothing crashes, sizes are right, and the
    neighbours have the bits of the batch without it."""
    utts = [K.utterance(600, 4, 12), K.utterance(601, 4, 24, quiet=((0, 3),)), K.utterance(602, 4, 10)]
    assert K.events_of(K.oracle_flags(oracle, utts[1])) == 2
    m = eng.mvdr_multi(4, K.delays_of(4), 0.0)
    for entry in ("dev", "host"):
        pcm, counts, first = K.pack(utts)
        res = run(m, pcm, counts, first, entry)
        assert res[0].shape == (pcm.shape[1],) and res[1].shape == (pcm.shape[1],) and res[2].shape == (46,)
        with_it = per_utt(res, counts, first)
        pcm, counts, first = K.pack([utts[0], utts[2]])
        without = per_utt(run(m, pcm, counts, first, entry), counts, first)
        assert [with_it[0], with_it[2]] == without
        for u in (0, 1):                       # the neighbours themselves are sound from their block 5 on: 5 events >= 4 microphones
            _, o_pre = K.oracle_utt(oracle, utts[2 * u], 0.0)
            got_pre = np.frombuffer(without[u][1], np.float32)
            assert np.isfinite(o_pre[4 * B:]).all() and np.isfinite(got_pre[4 * B:]).all()
    m.close()


# ---- nothing else is written -------------------------------------------------------------------------------------------
def test_only_the_emitted_blocks_are_written(eng):
    import torch
    utts = [K.utterance(700 + u, 3, n) for u, n in enumerate([4, 0, 1, 6, 2])]
    pcm, counts, first = K.pack(utts, gaps=[6, 2, 2, 10, 2], pad=16)
    n, total = pcm.shape[1], int(counts.sum())
    block_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    d_pcm, d_s, d_b = torch.from_numpy(pcm).cuda(), torch.from_numpy(first).cuda(), torch.from_numpy(block_first).cuda()
    out = torch.full((n,), 0x5A5A, dtype=torch.int16, device="cuda")
    pre = torch.full((n,), -12345.5, dtype=torch.float32, device="cuda")
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    m.reserve_batch(total, len(utts))
    eng._use_torch_stream()
    assert lib().jdsp_mvdrn_batch_dev(m._h, vp(d_pcm), n, vp(d_s), vp(d_b), len(utts), total, vp(out), vp(pre), None) == 0
    torch.cuda.synchronize()
    keep = np.ones(n, bool)
    for s, nb in zip(first, counts):
        keep[int(s) + B:int(s) + int(nb) * B] = False
    out, pre = out.cpu().numpy(), pre.cpu().numpy()
    assert np.all(out[keep] == 0x5A5A) and np.all(pre[keep] == np.float32(-12345.5))
    assert not np.any(pre[~keep] == np.float32(-12345.5))     # and every emitted sample is
    assert np.count_nonzero(~keep) == (3 + 5 + 1) * B
    m.close()


# ---- chunk geometry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_events", [P - 1, P, P + 1, 2 * P, 2 * P + 1])
def test_event_counts_around_the_chunk_length(eng, oracle, n_events):
    """P = kMvnBatchEvents (csrc/jdsp_internal.h) estimation frames make a chunk of the covariance update: one chunk up to
    P, two from P + 1 (the chunk sums and their prefix in play), three from 2 P + 1; the utterance stands between two
    ordinary ones, whose chunk slots and weight rows lie around its own."""
    utts = [K.utterance(800, 3, 7), K.events_run(300 + n_events, n_events), K.utterance(801, 3, 9)]
    assert K.events_of(K.oracle_flags(oracle, utts[1])) == n_events
    pcm, counts, first = K.pack(utts)
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    out, pre, flags = run(m, pcm, counts, first)
    worst = K.check_batch(oracle, utts, first, out, pre, flags)
    # measured, not promised (include/jdsp.h): the bits against process() of a fresh handle on the utterance alone
    o1, p1 = m.process(utts[1], want_precast=True)
    same = K.span_of(pre, int(first[1]), int(counts[1])).tobytes() == p1.tobytes()
    print("%d events: worst %.3f of the bar; precast bits equal to process(): %s" % (n_events, worst, same))
    m.close()


def test_more_blocks_than_one_tile_of_the_prefix_sum(eng, oracle):
    """The event prefix sum runs in tiles of 2,048 blocks (kMvnbTile, csrc/mvdrn_batch_kernels.hip) with the tiles'
    offsets scanned between two passes: three tiles here, an utterance of 150 estimation frames (two chunks) across the
    first tile boundary, an ordinary one across the second, empty utterances in between."""
    tile = 2048
    utts, total = [], 0
    while total < tile - 60:
        utts.append(K.utterance(1000 + len(utts), 2, 37 + 7 * len(utts) % 30, quiet=((0, 6), (15, 5))))
        total += utts[-1].shape[1] // B
    long_one = len(utts)
    utts.append(K.events_run(1999, 150, n_mics=2))
    utts.append(K.utterance(1998, 2, 0))
    total += 155
    while total < 2 * tile + 100:
        utts.append(K.utterance(1000 + len(utts), 2, 41 + 11 * len(utts) % 37, quiet=((0, 6), (15, 5))))
        total += utts[-1].shape[1] // B
    pcm, counts, first = K.pack(utts)
    block_first = np.concatenate([[0], np.cumsum(counts)])
    assert block_first[long_one] < tile - 2 and block_first[long_one + 1] > tile + 2 and block_first[-1] > 2 * tile
    assert not np.any(block_first == 2 * tile)                 # an utterance lies across the second boundary too
    m = eng.mvdr_multi(2, K.delays_of(2), K.LOADING)
    out, pre, flags = run(m, pcm, counts, first)
    K.check_batch(oracle, utts, first, out, pre, flags)
    m.close()


def test_bits_against_process_are_within_the_bars(eng, oracle):
    """Against process() of a fresh handle on the utterance alone the agreement is to the oracle's bars.  Whether the
    bits are equal as well is printed per utterance: measured, not promised."""
    n_mics = 8
    utts = K.oracle_batch_utts(n_mics)
    pcm, counts, first = K.pack(utts)
    m = eng.mvdr_multi(n_mics, K.delays_of(n_mics), K.LOADING)
    out, pre, _ = run(m, pcm, counts, first)
    equal = []
    for u, s in zip(utts, first):
        nb = u.shape[1] // B
        if nb == 0:
            continue
        m.reset()
        o1, p1 = m.process(u, want_precast=True)
        got_o, got_p = K.span_of(out, int(s), nb), K.span_of(pre, int(s), nb)
        fin = np.isfinite(p1)
        assert np.array_equal(np.isfinite(got_p), fin)
        if fin.any():                                          # each side within one bar of the oracle: two bars apart at most
            assert np.abs(got_p[fin] - p1[fin]).max() < 2 * K.TOL * max(np.abs(p1[fin]).max(), 1.0)
        assert got_o.size == 0 or np.abs(got_o.astype(np.int32) - o1.astype(np.int32)).max() <= 2
        equal.append(got_p.tobytes() == p1.tobytes() and got_o.tobytes() == o1.tobytes())
    print("bits equal to process() in %d of %d utterances (8 microphones, <= 128 events each)" % (sum(equal), len(equal)))
    m.close()


# ---- the handle's own stream -------------------------------------------------------------------------------------------
def test_a_batch_between_two_process_calls_leaves_the_stream_alone(eng, oracle):
    a = K.array_scene(9, 3, 30, quiet=((2, 5), (14, 6)))[0]
    o_out, o_pre = oracle.mvdrn_stream(a, K.delays_of(3), K.LOADING)
    other = [K.utterance(900 + u, 3, n) for u, n in enumerate([6, 11])]
    pcm, counts, first = K.pack(other)
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    o1, p1 = m.process(a[:, :12 * B], want_precast=True)
    res = run(m, pcm, counts, first)
    K.check_batch(oracle, other, first, *res)
    o2, p2 = m.process(a[:, 12 * B:], want_precast=True)
    K.check(np.concatenate([o1, o2]), np.concatenate([p1, p2]), o_out, o_pre)
    m.close()


# ---- errors and empties ------------------------------------------------------------------------------------------------
def test_512_point_handles_are_refused_by_all_three_entries(eng):
    L = lib()
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING, n_fft=512)
    for rc in (L.jdsp_mvdrn_batch_reserve(m._h, 8, 2),
               L.jdsp_mvdrn_batch_dev(m._h, None, 0, None, None, 1, 2, None, None, None),
               L.jdsp_mvdrn_batch(m._h, None, 0, 0, None, None, 1, None, None, None)):
        assert rc == EINVAL and "1024-point handles only" in last_error(eng)
    m.close()


def test_device_entry_needs_a_reservation_that_covers_the_batch(eng, oracle):
    import torch
    L = lib()
    utts = [K.utterance(950 + u, 3, n) for u, n in enumerate([4, 6])]
    pcm, counts, first = K.pack(utts)
    n = pcm.shape[1]
    block_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    d_pcm, d_s, d_b = torch.from_numpy(pcm).cuda(), torch.from_numpy(first).cuda(), torch.from_numpy(block_first).cuda()
    out = torch.zeros(n, dtype=torch.int16, device="cuda")
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    eng._use_torch_stream()

    def call(n_utts, n_blocks, p=d_pcm):
        return L.jdsp_mvdrn_batch_dev(m._h, vp(p), n, vp(d_s), vp(d_b), n_utts, n_blocks, vp(out), None, None)
    assert call(2, 10) == EINVAL and "jdsp_mvdrn_batch_reserve" in last_error(eng)        # before any reserve
    m.reserve_batch(9, 1)
    assert call(2, 10) == EINVAL and "jdsp_mvdrn_batch_reserve" in last_error(eng)        # more blocks than reserved
    m.reserve_batch(10, 1)
    assert call(2, 10) == EINVAL                                                          # more utterances than reserved
    assert call(-1, 10) == EINVAL
    assert L.jdsp_mvdrn_batch_dev(m._h, C.c_void_p(d_pcm.data_ptr() + 2), n, vp(d_s), vp(d_b), 2, 10, vp(out), None,
                                  None) == EINVAL and "aligned" in last_error(eng)
    m.reserve_batch(10, 2)
    assert call(2, 10) == 0
    torch.cuda.synchronize()
    res = m.process_batch(d_pcm, counts, first, want_precast=True, want_flags=True)
    torch.cuda.synchronize()
    assert np.array_equal(res[0].cpu().numpy(), out.cpu().numpy())
    K.check_batch(oracle, utts, first, *[r.cpu().numpy() for r in res])
    m.close()


def test_host_entry_checks_the_offsets_and_goes_on_working(eng, oracle):
    L = lib()
    utts = [K.utterance(960 + u, 3, n) for u, n in enumerate([4, 6])]
    pcm, counts, first = K.pack(utts, gaps=[2, 2])
    n = pcm.shape[1]
    block_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = np.zeros(n, np.int16)
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)

    def call(s, b, n_utts=2):
        s, b = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(b, np.int64)
        return L.jdsp_mvdrn_batch(m._h, vp(pcm), n, n, vp(s), vp(b), n_utts, vp(out), None, None)
    assert call(first + [1, 0], block_first) == EINVAL and "even" in last_error(eng)
    assert call([first[0], first[0] + 2 * B], block_first) == EINVAL and "overlap" in last_error(eng)
    assert call(first, block_first + 1) == EINVAL and "block_first[0]" in last_error(eng)
    assert call(first, block_first, -1) == EINVAL
    assert call(first, block_first) == 0
    res = run(m, pcm, counts, first, "host")
    assert np.array_equal(res[0], out)
    K.check_batch(oracle, utts, first, *res)
    m.close()


def test_empty_batches_and_no_outputs_succeed(eng):
    import torch
    L = lib()
    m = eng.mvdr_multi(3, K.delays_of(3), K.LOADING)
    pcm = K.utterance(970, 3, 4)
    n = pcm.shape[1]
    zeros3 = np.zeros(3, np.int64)
    zeros4 = np.zeros(4, np.int64)
    d_pcm, d_s, d_b = torch.from_numpy(pcm).cuda(), torch.from_numpy(zeros3).cuda(), torch.from_numpy(zeros4).cuda()
    eng._use_torch_stream()
    # no reservation was made: none of these launches anything
    assert L.jdsp_mvdrn_batch_dev(m._h, vp(d_pcm), n, None, None, 0, 0, None, None, None) == 0
    assert L.jdsp_mvdrn_batch_dev(m._h, vp(d_pcm), n, vp(d_s), vp(d_b), 3, 0, None, None, None) == 0
    assert L.jdsp_mvdrn_batch_dev(m._h, vp(d_pcm), n, vp(d_s), vp(d_b), 1, 4, None, None, None) == 0
    out = np.full(n, 77, np.int16)
    assert L.jdsp_mvdrn_batch(m._h, vp(pcm), n, n, None, None, 0, vp(out), None, None) == 0 and not out.any()
    assert L.jdsp_mvdrn_batch(m._h, vp(pcm), n, n, vp(zeros3), vp(zeros4), 3, vp(out), None, None) == 0
    assert L.jdsp_mvdrn_batch(m._h, vp(pcm), n, n, vp(zeros3[:1]), vp(np.array([0, 4], np.int64)), 1, None, None, None) == 0
    # through the Python layer: no utterance, and utterances without a block
    for counts in ([], [0, 0, 0]):
        o = m.process_batch(pcm, counts)
        assert o.shape == (n,) and not o.any()
        o, f = m.process_batch(torch.from_numpy(pcm).cuda(), counts, want_flags=True)
        torch.cuda.synchronize()
        assert o.shape == (n,) and not o.cpu().numpy().any() and f.numel() == 0
    m.close()
