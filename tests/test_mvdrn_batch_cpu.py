"""CPU side of the batched n-microphone MVDR (jdsp_mvdrn_batch*): the declaration and ctypes binding of the three
entries, and two conditions on the scenes of tests/test_mvdrn_batch_gpu.py that the oracle alone can show -- that the
comparison there is not a comparison of NaN with NaN, and that the utterance boundary is visible at the bars."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mvdrn_batch_cases as K  # noqa: E402


def test_batch_entries_are_declared_and_bound():
    from jeicyboodsp_amd._lib import lib
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    for name, n_args in (("jdsp_mvdrn_batch_reserve", 3), ("jdsp_mvdrn_batch_dev", 10), ("jdsp_mvdrn_batch", 10)):
        m = re.search(r"\bint\s+%s\(([^)]*)\)" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name     # the header's own argument count
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert "#define JDSP_ABI_VERSION 2" in txt
    from jeicyboodsp_amd.engine import MvdrMulti
    assert callable(MvdrMulti.reserve_batch) and callable(MvdrMulti.process_batch)
    # the chunk length the tests walk around is the kernels'
    internal = open(os.path.join(ROOT, "jeicyboodsp_amd", "csrc", "jdsp_internal.h")).read()
    assert re.search(r"constexpr int kMvnBatchEvents = %d;" % K.P, internal)


@pytest.mark.parametrize("n_mics", K.N_MICS)
def test_most_emitted_samples_of_the_oracle_case_are_finite(oracle, n_mics):
    """A condition on the scenes, not a measurement: at least 80 % of all emitted samples of the oracle-per-utterance
    batch are finite in the oracle.  (Seeds 100 n_mics + u give 0.992 for 2, 3, 5 and 8 microphones: 125 of the 126
    emitted blocks; only the 2-block utterance, which has no quiet lead, is all non-finite, and the 1-block ones emit
    nothing.)"""
    finite = total = 0
    for utt in K.oracle_batch_utts(n_mics):
        _, pre = K.oracle_utt(oracle, utt)
        finite += int(np.isfinite(pre).sum())
        total += pre.size
    assert total == 126 * K.B
    assert finite >= 0.8 * total, finite / total


def test_the_boundary_pair_differs_from_one_stream_by_more_than_100_bars(oracle):
    """The oracle over A|B as ONE stream against B alone, in B's blocks: a kernel that lets an estimation frame or a
    previous block cross the utterance boundary computes the former and cannot pass for the latter.  (Seeds 1 and 2:
    6.6 % of B's peak, 3,563 of 3,584 int16 samples different.)"""
    a, b = K.boundary_pair()
    assert K.oracle_flags(oracle, a)[-2:].tolist() == [0, 0] and K.oracle_flags(oracle, b)[:3].tolist() == [0, 0, 1]
    o_ab, p_ab = K.oracle_utt(oracle, np.concatenate([a, b], axis=1))
    o_b, p_b = K.oracle_utt(oracle, b)
    o_ab, p_ab = o_ab[8 * K.B:], p_ab[8 * K.B:]               # the emissions for B's blocks 1 .. 7
    assert p_ab.shape == p_b.shape and np.isfinite(p_b).all() and np.isfinite(p_ab).all()
    peak = np.abs(p_b).max()
    assert np.abs(p_ab - p_b).max() > 100 * K.TOL * peak
    assert np.count_nonzero(o_ab != o_b) > 100


@pytest.mark.parametrize("n_events", [K.P - 1, K.P, K.P + 1, 2 * K.P, 2 * K.P + 1])
def test_chunk_scenes_have_the_event_counts_they_are_named_for(oracle, n_events):
    utt = K.events_run(300 + n_events, n_events)
    assert K.events_of(K.oracle_flags(oracle, utt)) == n_events
