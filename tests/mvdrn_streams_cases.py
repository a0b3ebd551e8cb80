"""The cases the live n-microphone MVDR stream tests share (jdsp_mvdrn_streams*, include/jdsp.h): the streams, the cuts
of a stream into chunks and calls, the delivery of a plan through MvdrMulti.process_streams and the comparisons.  The
scenes, the packing, the oracle and the bars are tests/mvdrn_batch_cases.py's.  No GPU import at module level:
tests/test_mvdrn_streams_cpu.py uses the same scenes and plans to show that the GPU comparisons are not vacuous.

A PLAN is a list of calls, a call a list of chunks (stream, blocks) in the order they stand in the call; a stream's
chunks continue where its last one ended."""
import numpy as np

import mvdrn_batch_cases as K
from mvdrn_batch_cases import B

ORACLE_TOTALS = [1, 2, 12, 40, 0]                         # blocks of the five streams of the oracle case
ORACLE_MICS = [2, 3, 8]
CUT_AT = 8                                                # cut_stream(): blocks 7 and 8 are quiet, A | B of boundary_pair()
BATCH_EQUAL = [127, 128]                                  # events_run sizes whose bits equal the batch's
BATCH_BARS = {130: "50 / 1 / rest", 257: "chunks of 64"}  # ... and those held to the bars only


def scene(seed, n_mics, n_blocks):
    """quiet stretches at blocks 0..5, 15..19 and 28..33 where they fit: estimation frames early, in the middle and late"""
    return K.utterance(seed, n_mics, n_blocks, quiet=((0, 6), (15, 5), (28, 6)))


def oracle_streams(n_mics):
    return [scene(40 * n_mics + s, n_mics, n) for s, n in enumerate(ORACLE_TOTALS)]


def cut_stream():
    """40 blocks on 3 microphones: boundary_pair() joined into one stream (its blocks 6 .. 9 are quiet, so 7, 8 and 9
    are estimation frames and a cut at CUT_AT puts one at a chunk's block 0, where it reads the carried PCM), then 24
    blocks of scene()"""
    a, b = K.boundary_pair()
    return np.concatenate([a, b, scene(77, 3, 24)], axis=1)


def loading0_stream():
    """3 microphones for loading 0: blocks 0 .. 4 quiet, so the estimation frames are blocks 1, 2, 3, 4 and the third
    is block 3; 12 blocks"""
    return K.utterance(91, 3, 12, quiet=((0, 5),))


LOADING0_CUT = 3                                          # behind the second estimation frame (block 2)


def event_blocks(flags):
    """the blocks of a stream that are estimation frames, given the VAD decisions of all its blocks"""
    quiet = np.asarray(flags) == 0
    return (np.nonzero(quiet[1:] & quiet[:-1])[0] + 1).tolist()


# ---- cuts: a stream's blocks as the sizes of its chunks, one chunk per call -------------------------------------------
def cuts_each(n):
    return [1] * n


def cuts_of(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


def cuts_random(seed, n, most=9):
    """random sizes 0 .. most that add up to n, a chunk of 0 blocks among them"""
    rng = np.random.default_rng(seed)
    cuts = []
    while sum(cuts) < n:
        cuts.append(int(min(rng.integers(0, most + 1), n - sum(cuts))))
    if 0 not in cuts:
        cuts.insert(len(cuts) // 2, 0)
    return cuts


def plan_of(cuts, stream=0):
    return [[(stream, n)] for n in cuts]


def random_plan(seed, totals, n_calls):
    """every stream's blocks dealt over n_calls calls: in each call a random subset of the streams in random order, each
    with 0 .. 9 blocks; the last call takes the rest of every stream"""
    rng = np.random.default_rng(seed)
    left, plan = list(totals), []
    for k in range(n_calls):
        call = []
        for s in rng.permutation(len(totals)).tolist():
            if k + 1 == n_calls:
                call.append((s, left[s]))
            elif rng.random() < 0.7:
                call.append((s, int(rng.integers(0, min(left[s], 9) + 1))))
            else:
                continue
            left[s] -= call[-1][1]
        plan.append(call)
    assert not any(left)
    return plan


def calls_with_events(plan, stream, events):
    """the calls of the plan in which the stream has an estimation frame, and whether one of them is a chunk's block 0"""
    at, calls, at_zero = 0, set(), False
    for k, call in enumerate(plan):
        for s, n in call:
            if s == stream:
                mine = [e for e in events if at <= e < at + n]
                if mine:
                    calls.add(k)
                at_zero |= at in mine
                at += n
    return sorted(calls), at_zero


# ---- delivery -----------------------------------------------------------------------------------------------------------
def deliver(m, streams, plan, entry="dev", ids=None, gaps=False, stride_pad=0, outputs=True):
    """Runs the plan on the handle's live streams (open_streams first).  streams: {stream: int16 [n_mics, 512 n]} or a
    list; ids: the live stream each of them is delivered as (default: its own key).  gaps: even gaps in front of the
    chunks and a pad behind; stride_pad: the planes of the device buffer lie that many samples further apart.
    outputs False: every call with all three outputs NULL (nothing comes back).  Returns {stream: (out int16, precast
    float32, flags uint8)} with the spans of all its chunks concatenated: 512 samples per delivered block, block 0 of the
    stream's life included (it is never written)."""
    if not isinstance(streams, dict):
        streams = dict(enumerate(streams))
    at = {s: 0 for s in streams}
    got = {s: ([], [], []) for s in streams}
    for k, call in enumerate(plan):
        if not call:
            continue
        chunks = [streams[s][:, at[s] * B:(at[s] + n) * B] for s, n in call]
        pcm, counts, first = K.pack(chunks, gaps=[2 * ((k + i) % 4) for i in range(len(call))] if gaps else None,
                                    pad=8 if gaps else 0)
        live = [s if ids is None else ids[s] for s, _ in call]
        if not outputs:
            _no_outputs(m, pcm, live, counts, first)
            res = None
        elif entry == "host":
            res = m.process_streams(pcm, live, counts, first, want_precast=True, want_flags=True)
        else:
            import torch
            wide = torch.zeros((pcm.shape[0], pcm.shape[1] + stride_pad), dtype=torch.int16, device="cuda")
            wide[:, :pcm.shape[1]] = torch.from_numpy(pcm).cuda()
            res = m.process_streams(wide[:, :pcm.shape[1]], live, counts, first, want_precast=True, want_flags=True)
            torch.cuda.synchronize()
            res = tuple(r.cpu().numpy() for r in res)
        b = 0
        for (s, n), a in zip(call, first):
            if res is not None:
                got[s][0].append(res[0][int(a):int(a) + n * B])
                got[s][1].append(res[1][int(a):int(a) + n * B])
                got[s][2].append(res[2][b:b + n])
            at[s] += n
            b += n
    if not outputs:
        return None
    return {s: (np.concatenate(g[0] + [np.zeros(0, np.int16)]), np.concatenate(g[1] + [np.zeros(0, np.float32)]),
                np.concatenate(g[2] + [np.zeros(0, np.uint8)])) for s, g in got.items()}


def _no_outputs(m, pcm, live, counts, first):
    import torch
    from jeicyboodsp_amd.engine import L, _vp
    t = torch.from_numpy(pcm).cuda()
    arrays = [torch.from_numpy(np.ascontiguousarray(a, np.int64)).cuda()
              for a in (live, first, np.concatenate([[0], np.cumsum(counts)]))]
    m.eng._use_torch_stream()
    rc = L.jdsp_mvdrn_streams_dev(m._h, _vp(t), t.shape[1], _vp(arrays[0]), _vp(arrays[1]), _vp(arrays[2]), len(live),
                                  int(np.sum(counts)), None, None, None)
    torch.cuda.synchronize()
    assert rc == 0, rc


# ---- comparisons --------------------------------------------------------------------------------------------------------
def same_bytes(a, b):
    """two results of one stream (out, precast, flags): out and flags equal as bytes, the same samples finite, and the
    finite precast samples equal as bytes (sign and payload of a NaN are no part of any comparison)"""
    fa, fb = np.isfinite(a[1]), np.isfinite(b[1])
    return (a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes() and np.array_equal(fa, fb) and
            a[1][fa].tobytes() == b[1][fb].tobytes())


def check_oracle(orc, pcm, res, loading=K.LOADING, held=None):
    """a stream's concatenated spans against the oracle's stream of all its blocks; returns the share of the bar"""
    out, pre, flags = res
    n = pcm.shape[1] // B
    assert out.size == n * B and pre.size == n * B and flags.size == n
    if n == 0:
        return 0.0
    assert not out[:B].any() and not pre[:B].any()             # block 0 of the stream's life: never written
    assert np.array_equal(flags, K.oracle_flags(orc, pcm))
    o_out, o_pre = K.oracle_utt(orc, pcm, loading)
    return K.check(out[B:], pre[B:].astype(np.float64), o_out, o_pre, held)
