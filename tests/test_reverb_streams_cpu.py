"""CPU tests of the live reverberation streams' boundary and of their test cases: libjdsp.so exports the five
jdsp_reverb_streams* entries and the Python binding knows them, the header states the contract, the "Graph capture"
conventions name the device entries in class D and the reserve call among the allocating ones, the ABI version stays
2; the cases of reverb_streams_cases.py are not vacuous (plain FP32 that carries its history meets both bars on every
chunk, plain FP32 that forgets it misses them wherever the history matters) and the cut patterns hold what they claim."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reverb_cases as K
import reverb_streams_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jdsp.h")
LIB = os.path.join(ROOT, "jeicyboodsp_amd", "libjdsp.so")
ENTRIES = {"jdsp_reverb_streams_reserve": 3, "jdsp_reverb_streams_reset_dev": 3, "jdsp_reverb_streams_dev": 11,
           "jdsp_reverb_streams": 11, "jdsp_reverb_streams_state": 5}
B = K.B


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build_hip()
    return C.CDLL(LIB)


def test_the_library_exports_the_five_entries_and_the_binding_knows_them(lib):
    missing = [n for n in ENTRIES if not hasattr(lib, n)]
    assert not missing, missing
    import jeicyboodsp_amd
    from jeicyboodsp_amd.engine import L, Reverb
    EINVAL = jeicyboodsp_amd._lib.EINVAL
    for n, argc in ENTRIES.items():
        assert len(getattr(L, n).argtypes) == argc, n
    for m in ("open_streams", "process_streams", "reset_streams", "streams_state"):
        assert callable(getattr(Reverb, m)), m
    # handles of nothing are refused
    assert L.jdsp_reverb_streams_reserve(None, 1, 1) == EINVAL
    assert L.jdsp_reverb_streams_reset_dev(None, None, 0) == EINVAL
    assert L.jdsp_reverb_streams_dev(None, None, None, None, None, None, None, 0, 0, None, None) == EINVAL
    assert L.jdsp_reverb_streams(None, None, 0, None, None, None, None, None, 0, None, None) == EINVAL
    assert L.jdsp_reverb_streams_state(None, None, 0, None, None) == EINVAL


def test_the_header_states_the_contract(lib):
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, code), n
    # behind the batch entries, whose section keeps its place
    assert code.index("jdsp_reverb_batch(") < code.index("jdsp_reverb_streams_reserve(")
    assert re.search(r"#define\s+JDSP_ABI_VERSION\s+2\b", txt)
    lib.jdsp_abi_version.restype = C.c_int
    assert lib.jdsp_abi_version() == 2
    flat = re.sub(r"[\s*]+", " ", txt)
    sec = flat[flat.index("live reverberation streams: carried spectra"):flat.index("int jdsp_reverb_streams_reserve(")]
    for phrase in ("never presents a block twice", "all blocks so far", "HARD SWITCH", "whole carried history",
                   "Cross-fading is not built", "the walk ends at the stream's block 0", "p ascending",
                   "gain[c] 2^-10", "one block per call included", "EQUAL THE BYTES jdsp_reverb_batch writes",
                   "is not touched", "STATE ADVANCES", "launches nothing", "i mod (P - 1)", "59,272 bytes per stream",
                   "4,160 (P - 1) bytes", "one row (4,160 bytes) per block", "is the only call that allocates",
                   "calling it again discards them", "kept apart", "no host read of any array",
                   "every grid comes from the scalars alone", "no parallel branches", "The commit is a launch of its own",
                   "class D", "every replay advances the named streams", "distinct within a call",
                   "clamped into [0, n_irs)", "no speed is promised", "LEAVES EVERY STREAM AS IT WAS",
                   "ZERO outside the spans", "zeros for a fresh stream", "must not overlap pcm"):
        assert phrase in sec, phrase
    # the conventions: the device entries carry their state on the device, and the workspace has a reserve call
    conv = flat[flat.index("Class D, state on the device only"):flat.index("Class H, state the host carries")]
    for n in ("jdsp_reverb_streams_dev", "jdsp_reverb_streams_reset_dev"):
        assert n in conv, n
    assert "jdsp_reverb_streams_reserve" in flat[:flat.index("GRAPH CAPTURE.")]


# ---- the cases are not vacuous ---------------------------------------------------------------------------------------------
def _met(got, want):
    """both bars met; a cell that must be exact zeros counts as met when the restatement gives zeros"""
    if want.zero:
        return (0.0, 0.0) if not np.asarray(got).any() else (np.inf, np.inf)
    return S.ratios(got, want)


@pytest.mark.parametrize("name", S.BANKS)
def test_plain_fp32_meets_the_bars_with_its_history_and_misses_them_without(name):
    taps = K.banks()[name]
    P = K.n_part(taps.shape[1])
    strs = S.streams(name)
    worst, n_chunks, n_audible, n_matter = [0.0, 0.0], 0, 0, 0
    for k, s in enumerate(strs):
        for pattern in (S.PATTERNS if s.cuts is None else ("own",)):
            calls = S.chunks_of(S.calls_of(s, P, pattern))
            pairs = S.params_of(s) or [(s.ir, s.gain)] * len(calls)
            assert len(pairs) == len(calls)
            for (first, blocks), (ir, gain) in zip(calls, pairs):
                want = S.chunk_oracle(name, k, first, blocks, ir, gain)
                sl = slice(first * B, (first + blocks) * B)
                # plain FP32 on all blocks so far, with the chunk's response and gain
                carried = K.restate32(s.x[:sl.stop], taps[ir], gain)[sl]
                g, loc = _met(carried, want)
                what = (name, k, s.family, pattern, first, blocks, ir, gain)
                assert g <= 1.0 and loc <= 1.0, (what, g, loc)
                worst = [max(worst[0], g), max(worst[1], loc)]
                n_chunks += 1
                # the same with the history forgotten: the chunk as a fresh utterance
                audible, matters = S.history_matters(name, k, first, blocks, ir, gain)
                n_audible += audible
                if matters:
                    fresh = K.restate32(s.x[sl], taps[ir], gain)
                    n_matter += 1
                    assert max(_met(fresh, want)) > 1.0, ("a fresh utterance passes", what)
    print("\n  %-10s P = %2d, %2d streams, %4d chunks: plain FP32 at worst %.4f of the global bar, %.4f of the local "
          "bar; the history is not silent in front of %d chunks and adds more than two bars to %d of them: each of "
          "those misses a bar when it is forgotten" % (name, P, len(strs), n_chunks, worst[0], worst[1], n_audible, n_matter))
    if taps.shape[1] == 1:
        assert n_audible == 0                                  # tap1: one tap reaches no history at all
    else:
        # silent families, gain 0, first chunks and the chunks in front of an impulse have no audible history: the
        # rest is more than a third of all chunks, and only a measured response's faint late taps fail to matter
        assert n_audible > n_chunks // 3 and n_matter > 0.9 * n_audible


# ---- the cut patterns hold what they claim -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in S.BANKS if K.n_part(K.banks()[n].shape[1]) == 15])
def test_the_cut_patterns_hold_what_they_claim(name):
    P, strs = 15, S.streams(name)
    L = S.long_len(P)
    assert L == 47 and L > 3 * (P - 1)                         # the ring wraps more than twice
    pats = S.patterns(L, P)
    sizes = {c for calls in pats.values() for c in calls if c}
    assert {1, P - 2, P - 1, P, P + 1} <= sizes and pats["one"] == [L] and pats["single"] == [1] * L
    assert max(sizes) > P - 1                                  # a chunk longer than the ring
    assert all(c % 2 == 1 for c in pats["odd"][:-1]) and {3, 5, 7} <= set(pats["odd"])
    assert None in pats["pairs_absent"] and 0 in pats["pairs_absent"] and 2 in pats["pairs_absent"]
    wraps = [(first, n) for calls in pats.values() for first, n in S.chunks_of(calls)
             if first > 0 and 1 < n <= P - 1 and first % (P - 1) + n > P - 1]
    assert wraps, "no chunk shorter than the ring wraps it"
    # the streams: one per family, the short one, two switched ones; the loud blocks stand in front of quiet ones
    assert [s.family for s in strs[:len(K.FAMILIES)]] == list(K.FAMILIES)
    short = [s for s in strs if s.cuts is None and s.x.size // B < P]
    assert len(short) == 1
    for s in strs:
        if s.family == "loud_then_quiet":
            loud = S.loud_blocks(s.x)
            assert loud.size and 0 < loud.min() and loud.max() + P < s.x.size // B
    sw = [s for s in strs if s.cuts is not None]
    assert len(sw) == 2
    for s in sw:
        pairs = S.params_of(s)
        assert all(a != b for a, b in zip(pairs, pairs[1:]))   # every boundary switches
        assert any(g0 == -3.0 and g1 == 0.0 for (_, g0), (_, g1) in zip(pairs, pairs[1:]))
        assert max(s.cuts) > P - 1 and None in S.calls_of(s, P, None) and 0 in S.calls_of(s, P, None)
    # side by side: every stream under its own pattern, all blocks delivered (deliveries() asserts it)
    for r in range(len(S.PATTERNS)):
        calls = S.deliveries(strs, P, [S.PATTERNS[(k + r) % len(S.PATTERNS)] for k in range(len(strs))], r)
        assert any(len(c) > 1 for c in calls) and any(ch.blocks == 0 for c in calls for ch in c)
