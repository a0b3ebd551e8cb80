"""The host side of the live n-microphone MVDR streams (jdsp_mvdrn_streams*, MvdrMulti.process_streams): the entries are
declared, exported and bound, sharding.mvdrn_stream_written is the rule "only block 0 of a stream's life is never
written", and the cases of tests/test_mvdrn_streams_gpu.py are not vacuous -- checked with the oracle on the CPU.  No GPU
needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mvdrn_batch_cases as K  # noqa: E402
import mvdrn_streams_cases as S  # noqa: E402
from mvdrn_batch_cases import B  # noqa: E402

ENTRIES = (("jdsp_mvdrn_streams_reserve", 3), ("jdsp_mvdrn_streams_reset_dev", 3), ("jdsp_mvdrn_streams_dev", 11),
           ("jdsp_mvdrn_streams", 11), ("jdsp_mvdrn_streams_state", 5))


def test_entries_are_declared_exported_and_bound():
    import ctypes as C
    from jeicyboodsp_amd import _lib
    assert _lib.lib.jdsp_abi_version() == 2
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    assert "#define JDSP_ABI_VERSION 2" in txt
    raw = C.CDLL(_lib.LIB_PATH)                                  # the library's own symbol table, not the binding's
    for name, n_args in ENTRIES:
        assert "int %s(" % name in txt, name
        decl = txt[txt.index("int %s(" % name):]
        assert decl[:decl.index(";")].count(",") + 1 == n_args, name
        assert getattr(raw, name) is not None, name
        assert len(getattr(_lib.lib, name).argtypes) == n_args, name
    conventions = txt[:txt.index("#ifndef JDSP_H")]
    for name in ("jdsp_mvdrn_streams_dev", "jdsp_mvdrn_streams_reset_dev"):
        assert name in conventions[conventions.index("Class D"):conventions.index("Class H")], name
    assert "jdsp_mvdrn_streams*" in txt[txt.index("#ifdef __cplusplus"):txt.index("#define JDSP_ABI_VERSION")]


def test_the_wrapper_has_the_methods():
    from jeicyboodsp_amd.engine import MvdrMulti
    for m in ("open_streams", "process_streams", "reset_streams", "streams_state"):
        assert callable(getattr(MvdrMulti, m)), m


# ---- sharding.mvdrn_stream_written ---------------------------------------------------------------------------------------
def first_written_block(seen, blocks):
    """a stream's block i is written iff i >= 1: walking the chunk, the index behind its last block that is not (the
    chunk's written blocks are [that, blocks): none when the chunk is block 0 alone)"""
    first = 0
    for b in range(blocks):
        if seen + b < 1:
            first = b + 1
    return first


def test_written_is_every_block_but_the_first_of_a_life():
    from jeicyboodsp_amd import sharding
    for n in range(4):
        for b in range(6):
            assert sharding.mvdrn_stream_written([n], [b]).tolist() == [first_written_block(n, b)], (n, b)
    seen = [n for n in range(4) for _ in range(6)]
    counts = [b for _ in range(4) for b in range(6)]
    w = sharding.mvdrn_stream_written(seen, counts)
    assert w.dtype == np.int64 and w.tolist() == [first_written_block(n, b) for n, b in zip(seen, counts)]
    assert sharding.mvdrn_stream_written(0, [0, 1, 2, 5]).tolist() == [0, 1, 1, 1]       # a scalar stands for all chunks
    assert sharding.mvdrn_stream_written(3, [0, 1, 2, 5]).tolist() == [0, 0, 0, 0]
    assert sharding.mvdrn_stream_written([], []).size == 0
    for seen, counts in (([0, 1], [3]), ([-1], [3]), ([0], [-2]), ([0, 0, 0], [1, 2])):
        with pytest.raises(ValueError):
            sharding.mvdrn_stream_written(seen, counts)


def test_stream_ids_split_over_ranks_with_stream_shard():
    from jeicyboodsp_amd import sharding
    owned = []
    for rank in range(3):
        first, count = sharding.stream_shard(1000, rank, 3)
        owned.extend(range(first, first + count))
    assert owned == list(range(1000))


# ---- the GPU cases are not vacuous ---------------------------------------------------------------------------------------
def events(oracle, pcm):
    return S.event_blocks(K.oracle_flags(oracle, pcm))


def test_the_cut_stream_has_an_estimation_frame_at_a_chunks_first_block(oracle):
    x = S.cut_stream()
    ev = events(oracle, x)
    assert x.shape == (3, 40 * B)
    assert [e for e in ev if e < 16] == [S.CUT_AT - 1, S.CUT_AT, S.CUT_AT + 1]
    assert len(ev) >= 12 and max(ev) > 30
    for cuts in ([40], S.cuts_each(40), S.cuts_random(5, 40), [S.CUT_AT, 40 - S.CUT_AT]):
        assert sum(cuts) == 40
    assert 0 in S.cuts_random(5, 40) and len(S.cuts_random(5, 40)) > 4
    calls, at_zero = S.calls_with_events(S.plan_of([S.CUT_AT, 40 - S.CUT_AT]), 0, ev)
    assert calls == [0, 1] and at_zero                         # block CUT_AT opens the second chunk and is one
    calls, at_zero = S.calls_with_events(S.plan_of(S.cuts_random(5, 40)), 0, ev)
    assert len(calls) >= 2
    calls, at_zero = S.calls_with_events(S.plan_of(S.cuts_each(40)), 0, ev)
    assert len(calls) == len(ev) and at_zero


def test_boundary_pair_as_one_stream_and_alone(oracle):
    a, b = K.boundary_pair()
    joined = events(oracle, np.concatenate([a, b], axis=1))
    assert 8 in joined and 7 in joined                          # B's first block is an estimation frame behind A ...
    assert events(oracle, b) == [1]                             # ... and alone it is not
    # and it matters: B's emitted block 1 differs between the two by far more than the bar
    _, together = K.oracle_utt(oracle, np.concatenate([a, b], axis=1))
    _, alone = K.oracle_utt(oracle, b)
    d = np.abs(together[8 * B:9 * B] - alone[:B]).max() / np.abs(alone[:B]).max()
    assert d > 100 * K.TOL, d


@pytest.mark.parametrize("n_mics", S.ORACLE_MICS)
def test_the_oracle_plan_has_estimation_frames_in_several_calls(oracle, n_mics):
    streams = S.oracle_streams(n_mics)
    assert [x.shape[1] // B for x in streams] == S.ORACLE_TOTALS
    plan = S.random_plan(11 + n_mics, S.ORACLE_TOTALS, 7)
    calls, _ = S.calls_with_events(plan, 3, events(oracle, streams[3]))
    assert len(calls) >= 2, calls                              # the 40-block stream's, at the least
    sizes = [n for call in plan for _, n in call]
    assert 0 in sizes and max(sizes) > 1 and any(len(call) < 5 for call in plan)
    assert any(S.calls_with_events(plan, s, events(oracle, streams[s]))[1] for s in (2, 3))


@pytest.mark.parametrize("n_events", S.BATCH_EQUAL + sorted(S.BATCH_BARS))
def test_the_event_runs_have_exactly_their_events(oracle, n_events):
    x = K.events_run(300 + n_events, n_events)
    assert K.events_of(K.oracle_flags(oracle, x)) == n_events
    assert (n_events <= K.P) == (n_events in S.BATCH_EQUAL)


def test_loading_0_is_finite_only_after_the_third_estimation_frame(oracle):
    x = S.loading0_stream()
    ev = events(oracle, x)
    assert ev == [1, 2, 3, 4] and ev[1] < S.LOADING0_CUT <= ev[2]
    _, pre = K.oracle_utt(oracle, x, 0.0)
    fin = np.isfinite(pre).reshape(-1, B)                       # emitted block i - 1 belongs to input block i
    assert not fin[:ev[2] - 1].any() and fin[ev[2] - 1:].all()
