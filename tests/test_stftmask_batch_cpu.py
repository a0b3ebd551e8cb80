"""CPU tests of the batched fused STFT masking's host side: the frame layout of a packed batch
(sharding.stftmask_batch_layout), the utterance split over ranks (sharding.stftmask_batch_shard) and the ctypes
binding of the two new entries."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jeicyboodsp_amd import sharding  # noqa: E402

N = 1024


@pytest.mark.parametrize("hop", [1024, 512, 256])
def test_layout_on_ragged_offsets(hop):
    # shorter than n (none, also empty), exactly n, exact multiples of the hop past n, remainders below a hop
    lens = [0, 2, N - 2, N, N + hop - 2, N + hop, N + hop + 2, N + 7 * hop, N + 8 * hop - 2, 10, N + 36 * hop + 6]
    want = [0, 0, 0, 1, 1, 2, 2, 8, 8, 0, 37]
    offs = np.concatenate([[0], np.cumsum(lens)])
    counts, first = sharding.stftmask_batch_layout(offs, N, hop)
    assert counts.dtype == np.int64 and first.dtype == np.int64
    assert counts.tolist() == want
    assert first.tolist() == [0] + np.cumsum(want).tolist()
    # every span fits its utterance, and one more frame would not
    for L, f in zip(lens, counts):
        assert (hop * (f - 1) + N <= L) if f else L < N
        assert hop * f + N > L
    # a list and a shifted (even) origin give the same counts
    c2, f2 = sharding.stftmask_batch_layout([int(o) + 64 for o in offs], N, hop)
    assert c2.tolist() == want and f2.tolist() == first.tolist()
    # no utterance at all
    c0, f0 = sharding.stftmask_batch_layout([0], N, hop)
    assert c0.size == 0 and f0.tolist() == [0]


def test_layout_rejects_odd_and_decreasing_offsets():
    with pytest.raises(ValueError):
        sharding.stftmask_batch_layout([0, 2049, 4096], N, 512)
    with pytest.raises(ValueError):
        sharding.stftmask_batch_layout([1, 2048], N, 512)
    with pytest.raises(ValueError):
        sharding.stftmask_batch_layout([0, 4096, 2048], N, 512)
    with pytest.raises(ValueError):
        sharding.stftmask_batch_layout([], N, 512)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("counts", [[1, 0, 3, 4, 2, 0, 0, 9, 1, 1, 37], [5], [0, 0, 0], [7, 7, 7, 7, 7, 7, 7, 7, 7], []],
                         ids=["ragged", "one", "empty-utts", "even", "none"])
def test_batch_shard_covers_every_utterance_once(world, counts):
    seen, frames = [], []
    for rank in range(world):
        first, n = sharding.stftmask_batch_shard(np.asarray(counts, np.int64), rank, world)
        assert n >= 0 and first == len(seen)                   # contiguous, in rank order
        seen.extend(range(first, first + n))
        frames.append(sum(counts[first:first + n]))
    assert seen == list(range(len(counts)))                    # each once, worlds above the utterance count included
    assert sum(frames) == sum(counts)
    if counts == [7] * 9 and world == 3:
        assert frames == [21, 21, 21]                          # balanced by frame count


def test_batch_entries_are_bound_and_declared():
    from jeicyboodsp_amd._lib import lib
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    for name, n_args in (("jdsp_stftmask_batch_dev", 10), ("jdsp_stftmask_batch", 10)):
        assert name + "(" in txt
        assert len(getattr(lib, name).argtypes) == n_args
