"""Live reverberation streams (jdsp_reverb_streams*): the streams, the cut patterns, the deliveries and the per-chunk
oracle that test_reverb_streams_cpu.py (CPU) and test_reverb_streams_gpu.py (device) share (not a test module).  Built
on reverb_cases.py (banks, families, bars, restate32, int16 rules) and reverb_ref.py (the FP64 direct convolution).

  BANKS                     the eight banks of reverb_cases.banks(): tap1 (P = 1, no history at all), taps512 (P = 1, only
                            the carried previous block matters), taps513 (P = 2, a ring of one row), taps1025, wrap1025
                            (P = 3), dense7680 and rir7169 (P = 15), highpass (256 taps)
  streams(name)             the bank's streams, computed once, read-only.  Constant ones (one (ir, gain) throughout):
                            one of L = 3 (P - 1) + 5 blocks per input family of reverb_cases.FAMILIES, so the ring wraps
                            more than twice (loud_then_quiet: max(L, 9) blocks -- from 9 blocks on the family's loud sixth
                            stands a quarter into the stream and quiet blocks follow it, so the ring carries loud rows
                            into quiet chunks), gains 1, 0.25, -3 and 0 dealt over them; one SHORT stream of max(P - 1,
                            1) blocks -- fewer than P wherever P > 1 -- whose walk ends at the stream's first row in
                            every chunk.  Switched ones: two per bank whose (ir, gain) changes at every chunk boundary,
                            fixed cuts: response 0 -> 1 at gains 1 -> 0.25 (the banks' rows are about equally loud, so a
                            quiet response is a row at a quarter of the gain; in the highpass bank row 1 IS -0.5 row
                            0), then gain -3 -> 0 -> 1.
  patterns(n, P)            name -> the calls of one stream of n blocks: a list with one entry per call, a block count
                            (0: a chunk of no blocks) or None (the stream sits the call out)
  deliveries(...)           the calls of several streams run side by side, each under its own pattern
  chunk_oracle(...)         per chunk: reverb_ref.reverb(all blocks so far, taps[ir_c], gain_c) and reverb_cases.bars_of of
                            the same arguments, both sliced to the chunk

The issue's pattern [1, P - 2, P - 1, P, P + 1, rest] adds up to 4 P - 1 blocks before its rest, 59 at P = 15, and
L is 47 there: cut to the stream it never reaches P + 1.  It is kept as "around_p", and "around_p_desc" delivers the
same sizes from the largest down, so every size occurs in every bank."""
import collections
import functools

import numpy as np

import reverb_cases as K
import reverb_ref

B = K.B
BANKS = ("tap1", "taps512", "taps513", "taps1025", "dense7680", "rir7169", "wrap1025", "highpass")
# family -> gain of its constant stream: every gain on a family that shows it
FAMILY_GAIN = (("white", 1.0), ("full_square", 0.25), ("constant", -3.0), ("sine_fs_off", 0.0), ("impulse", 1.0),
               ("silence", 0.25), ("loud_then_quiet", 1.0), ("silence_then_white", -3.0))
assert tuple(f for f, _ in FAMILY_GAIN) == K.FAMILIES and {g for _, g in FAMILY_GAIN} == set(K.GAINS)

Stream = collections.namedtuple("Stream", "x family cuts ir gain")
# x: int16 [512 n]; cuts: None (constant: delivered under every pattern) or the fixed chunk sizes of a switched stream;
# ir, gain: one value per chunk for a switched stream, scalars for a constant one


def long_len(P):
    return 3 * (P - 1) + 5


def switched_cuts(n, P):
    """chunk sizes of a switched stream of n blocks: short, longer than the ring, single, ... then the rest"""
    out, left = [], n
    for c in (2, P + 1, 1, 3, P - 1, 2, P):
        c = min(c, left)
        if c > 0:
            out.append(c)
            left -= c
    if left:
        out.append(left)
    return out


SWITCH_A = ((0, 1.0), (1, 0.25), (2, -3.0), (0, 0.0), (1, 1.0), (2, 1.0), (0, 0.25), (1, -3.0))
SWITCH_B = ((2, -3.0), (0, 0.0), (1, 1.0), (0, 1.0), (1, 0.25), (2, 0.0), (0, 1.0), (2, 0.25))


@functools.lru_cache(maxsize=None)
def streams(name):
    taps = K.banks()[name]
    n_irs, P = taps.shape[0], K.n_part(taps.shape[1])
    assert n_irs == 3
    L = long_len(P)
    out = []
    for k, (fam, gain) in enumerate(FAMILY_GAIN):
        n = max(L, 9) if fam == "loud_then_quiet" else L
        out.append(Stream(K.utterance(fam, n, 300 + k), fam, None, k % n_irs, gain))
    out.append(Stream(K.utterance("white", max(P - 1, 1), 320), "white", None, n_irs - 1, 1.0))       # the short one
    for j, (fam, cycle) in enumerate((("white", SWITCH_A), ("loud_then_quiet", SWITCH_B))):
        n = max(L, 9) if fam == "loud_then_quiet" else L
        cuts = switched_cuts(n, P)
        assert len(cuts) <= len(cycle) and sum(cuts) == n
        out.append(Stream(K.utterance(fam, n, 330 + j), fam, tuple(cuts), tuple(c[0] for c in cycle[:len(cuts)]),
                          tuple(c[1] for c in cycle[:len(cuts)])))
    return tuple(out)


def loud_blocks(x):
    """the blocks of a loud_then_quiet stream that hold loud samples"""
    return np.flatnonzero(np.abs(x.astype(np.int32)).reshape(-1, B).max(axis=1) > 1000)


# ---- cut patterns ------------------------------------------------------------------------------------------------------
def _cut(sizes, n, cycle=False):
    out, left, i = [], n, 0
    while left > 0 and (cycle or i < len(sizes)):
        c = min(sizes[i % len(sizes)], left)
        if c > 0:
            out.append(c)
            left -= c
        i += 1
    if left:
        out.append(left)
    return out


def patterns(n, P):
    """name -> calls of a stream of n blocks (see the module's text)"""
    pairs = []
    for i, c in enumerate(_cut([2], n, cycle=True)):
        pairs.append(c)
        pairs.append(None if i % 2 == 0 else 0)               # sits a call out / a chunk of no blocks, in turn
    p = collections.OrderedDict()
    p["one"] = [n]
    p["single"] = [1] * n
    p["around_p"] = _cut([1, P - 2, P - 1, P, P + 1], n)
    p["around_p_desc"] = _cut([P + 1, P, P - 1, P - 2, 1], n)
    p["odd"] = _cut([3, 5, 7], n, cycle=True)
    p["pairs_absent"] = pairs
    for calls in p.values():
        assert sum(c for c in calls if c) == n
    return p


PATTERNS = tuple(patterns(5, 1))


def calls_of(s, P, pattern):
    """the calls of stream s: a switched stream has its own cuts, with a call sat out and an empty chunk among them"""
    if s.cuts is None:
        return patterns(s.x.size // B, P)[pattern]
    out = []
    for i, c in enumerate(s.cuts):
        out.append(c)
        if i % 3 == 0:
            out.append(None if i % 2 == 0 else 0)
    return out


def chunks_of(calls):
    """[(first block, blocks)] of the chunks that hold blocks, in order"""
    out, at = [], 0
    for c in calls:
        if c:
            out.append((at, c))
            at += c
    return out


def params_of(s):
    """[(ir, gain)] per chunk that holds blocks; for a constant stream the one pair, whatever the pattern"""
    return None if s.cuts is None else list(zip(s.ir, s.gain))


Chunk = collections.namedtuple("Chunk", "stream first blocks ir gain")


def deliveries(strs, P, pattern_of, order_seed=0):
    """[[Chunk]]: call t holds the t-th call of every stream that has one and does not sit it out, in an order shuffled
    per call.  strs: the streams; pattern_of[k]: the pattern of stream k."""
    plans = [calls_of(s, P, pattern_of[k]) for k, s in enumerate(strs)]
    rng = np.random.default_rng(order_seed)
    calls = []
    at = [0] * len(strs)
    n_chunk = [0] * len(strs)
    for t in range(max(len(p) for p in plans)):
        row = []
        for k, (s, plan) in enumerate(zip(strs, plans)):
            if t >= len(plan) or plan[t] is None:
                continue
            c = plan[t]
            if s.cuts is None:
                ir, gain = s.ir, s.gain
            else:
                j = min(n_chunk[k], len(s.ir) - 1)             # an empty chunk names the pair of the chunk that follows
                ir, gain = s.ir[j], s.gain[j]
            row.append(Chunk(k, at[k], c, ir, gain))
            at[k] += c
            n_chunk[k] += 1 if c else 0
        calls.append([row[i] for i in rng.permutation(len(row))])
    assert at == [s.x.size // B for s in strs]
    return calls


def pack_call(strs, chunks, gaps=None, fill=32767, tail=0):
    """(pcm, sample_first, counts) of one call: the chunks' new blocks in list order, `gaps` samples (even) in front of
    each span, the gaps and the tail full-scale"""
    xs = [strs[c.stream].x[c.first * B:(c.first + c.blocks) * B] for c in chunks]
    pcm, first, _ = K.pack(xs, gaps, fill=fill, tail=tail)
    return pcm, first, np.array([c.blocks for c in chunks], np.int64)


# ---- the oracle ----------------------------------------------------------------------------------------------------------
Want = collections.namedtuple("Want", "w global_bar local_bar zero")


@functools.lru_cache(maxsize=None)
def _oracle(name, k, end_blocks, ir, gain):
    s = streams(name)[k]
    taps = K.banks()[name]
    x = s.x[:end_blocks * B]
    w = reverb_ref.reverb(x, taps[ir], gain)
    g, loc = K.bars_of(x, taps[ir], gain, w)
    for a in (w, loc):
        a.setflags(write=False)
    return w, g, loc


def chunk_oracle(name, k, first, blocks, ir, gain):
    """Want of the chunk [first, first + blocks) of stream k delivered with (ir, gain): the FP64 value of all blocks so
    far with that pair and its bars, sliced to the chunk; zero: the output must be exact zeros (a zero bar)"""
    w, g, loc = _oracle(name, k, first + blocks, int(ir), float(gain))
    sl = slice(first * B, (first + blocks) * B)
    return Want(w[sl], g, loc[sl], g == 0.0)


def whole_oracle(name, k):
    """a constant stream as the batch's utterance of all its blocks: a reverb_cases.Utt"""
    s = streams(name)[k]
    assert s.cuts is None
    w, g, loc = _oracle(name, k, s.x.size // B, s.ir, s.gain)
    return K.Utt(s.x, s.ir, s.gain, s.family, w, g, loc)


def ratios(got, want):
    """worst |got - w| over (the global bar, the local bar); an error under a zero bar is inf"""
    u = K.Utt(None, 0, 0.0, "", want.w, want.global_bar, want.local_bar)
    return K.ratios_of(got, u)


def history_matters(name, k, first, blocks, ir, gain):
    """(the history is not silent, it matters).  Not silent: a sample within the response's reach in front of the chunk
    is not zero, and the gain is not 0.  It matters: in FP64, what the blocks delivered before the chunk add to it is,
    at some sample, more than TWICE the smaller of the two bars there.  A computation that forgets the history and is
    itself within a bar of the chunk-alone value then stands more than a bar from the true one.  (A history can be
    audible and still not matter: the measured response of rir7169 starts with silent taps and has faint late ones.)"""
    taps = K.banks()[name]
    x = streams(name)[k].x
    audible = bool(gain != 0.0 and first > 0 and x[max(0, first * B - (taps.shape[1] - 1)):first * B].any())
    if not audible:
        return False, False
    want = chunk_oracle(name, k, first, blocks, ir, gain)
    alone = reverb_ref.reverb(x[first * B:(first + blocks) * B], taps[ir], gain)
    return True, bool(np.any(np.abs(want.w - alone) > 2.0 * np.minimum(want.local_bar, want.global_bar)))
