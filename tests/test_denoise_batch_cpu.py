"""CPU tests of the batched denoiser's host side: the packing of a batch (sharding.denoise_batch_layout), the utterance
split over ranks (sharding.stftmask_batch_shard on the block counts) and the declaration and ctypes binding of the
three new entries."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jeicyboodsp_amd import sharding  # noqa: E402


@pytest.mark.parametrize("hop", [512, 256])
def test_layout_on_ragged_counts(hop):
    counts = [0, 1, 2, 3, 0, 5, 12, 40, 333, 1, 70, 0]
    sample_first, block_first, n_samples = sharding.denoise_batch_layout(counts, hop)
    assert sample_first.dtype == np.int64 and block_first.dtype == np.int64
    assert block_first.tolist() == [0] + np.cumsum(counts).tolist()
    assert sample_first.tolist() == (np.asarray(block_first[:-1]) * hop).tolist()
    assert n_samples == hop * sum(counts)
    assert not np.any(sample_first & 1)
    # packed: every span ends where the next begins, empty utterances take nothing
    ends = sample_first + hop * np.asarray(counts)
    assert ends[:-1].tolist() == sample_first[1:].tolist() and ends[-1] == n_samples
    # an array gives what a list gives
    s2, b2, n2 = sharding.denoise_batch_layout(np.asarray(counts, np.int32), hop)
    assert s2.tolist() == sample_first.tolist() and b2.tolist() == block_first.tolist() and n2 == n_samples


def test_layout_of_no_utterance():
    sample_first, block_first, n_samples = sharding.denoise_batch_layout([], 512)
    assert sample_first.size == 0 and block_first.tolist() == [0] and n_samples == 0


def test_layout_rejects_negative_counts_and_odd_hops():
    with pytest.raises(ValueError):
        sharding.denoise_batch_layout([3, -1, 4], 512)
    with pytest.raises(ValueError):
        sharding.denoise_batch_layout([3, 4], 511)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("counts", [[0, 1, 2, 3, 0, 5, 12, 40, 333, 1, 70], [5], [0, 0, 0], [7] * 9, []],
                         ids=["ragged", "one", "empty-utts", "even", "none"])
def test_shard_split_covers_every_utterance_once(world, counts):
    seen, blocks = [], []
    for rank in range(world):
        first, n = sharding.stftmask_batch_shard(np.asarray(counts, np.int64), rank, world)
        assert n >= 0 and first == len(seen)                   # contiguous, in rank order
        seen.extend(range(first, first + n))
        blocks.append(sum(counts[first:first + n]))
        # the rank's own layout: its utterances' spans rebased to its first sample
        s_all, b_all, _ = sharding.denoise_batch_layout(counts, 512)
        s_own, b_own, n_own = sharding.denoise_batch_layout(counts[first:first + n], 512)
        if n:
            assert (s_all[first:first + n] - s_all[first]).tolist() == s_own.tolist()
        assert n_own == 512 * blocks[-1]
    assert seen == list(range(len(counts)))
    assert sum(blocks) == sum(counts)
    if counts == [7] * 9 and world == 3:
        assert blocks == [21, 21, 21]                          # balanced by block count
    assert "Denoiser.process_batch" in sharding.stftmask_batch_shard.__doc__


def test_batch_entries_are_declared_and_bound():
    from jeicyboodsp_amd._lib import lib
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    for name, n_args in (("jdsp_denoise_batch_reserve", 3), ("jdsp_denoise_batch_dev", 10), ("jdsp_denoise_batch", 10)):
        m = re.search(r"\bint\s+%s\(([^)]*)\)" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name     # the header's own argument count
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert "#define JDSP_ABI_VERSION 2" in txt
