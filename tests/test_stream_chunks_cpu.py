"""CPU tests of the live streams' host side: the back-to-back packing of a call's chunks
(sharding.stream_chunks_layout) against hand-written offsets, its errors, and the binding and declaration of the twelve
jdsp_{stftmask,istft}_streams* entries at an unchanged ABI version."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jeicyboodsp_amd import sharding  # noqa: E402

N = 1024
COUNTS = [3, 0, 1, 0, 0, 5, 1]

# hand-written: chunk c of F > 0 frames takes hop (F - 1) + N samples with its PCM, hop F without
WITH_PCM = {1024: [0, 3072, 3072, 4096, 4096, 4096, 9216, 10240],
            512: [0, 2048, 2048, 3072, 3072, 3072, 6144, 7168],
            256: [0, 1536, 1536, 2560, 2560, 2560, 4608, 5632]}
OUTPUT_ONLY = {1024: [0, 3072, 3072, 4096, 4096, 4096, 9216, 10240],
               512: [0, 1536, 1536, 2048, 2048, 2048, 4608, 5120],
               256: [0, 768, 768, 1024, 1024, 1024, 2304, 2560]}


@pytest.mark.parametrize("with_pcm", [True, False])
@pytest.mark.parametrize("hop", [1024, 512, 256])
def test_layout_against_hand_written_offsets(hop, with_pcm):
    want = (WITH_PCM if with_pcm else OUTPUT_ONLY)[hop]
    sample_first, frame_first, n_samples = sharding.stream_chunks_layout(COUNTS, N, hop, with_pcm)
    assert sample_first.dtype == np.int64 and frame_first.dtype == np.int64 and isinstance(n_samples, int)
    assert sample_first.tolist() == want[:-1] and n_samples == want[-1]
    assert frame_first.tolist() == [0, 3, 3, 4, 4, 4, 9, 10]
    assert not np.any(sample_first & 1)                            # even offsets
    # disjoint spans of the stated lengths, back to back: a chunk of no frames takes nothing
    spans = [(hop * (f - 1) + N if with_pcm else hop * f) if f else 0 for f in COUNTS]
    ends = sample_first + np.asarray(spans)
    assert np.all(ends[:-1] == sample_first[1:]) and ends[-1] == n_samples
    # a numpy array gives the same; no chunk at all gives nothing
    s2, f2, n2 = sharding.stream_chunks_layout(np.asarray(COUNTS, np.int32), N, hop, with_pcm)
    assert s2.tolist() == sample_first.tolist() and f2.tolist() == frame_first.tolist() and n2 == n_samples
    s0, f0, n0 = sharding.stream_chunks_layout([], N, hop, with_pcm)
    assert s0.size == 0 and f0.tolist() == [0] and n0 == 0
    # only empty chunks
    s1, f1, n1 = sharding.stream_chunks_layout([0, 0], N, hop, with_pcm)
    assert s1.tolist() == [0, 0] and f1.tolist() == [0, 0, 0] and n1 == 0


def test_layout_of_a_512_point_synthesis():
    sample_first, frame_first, n_samples = sharding.stream_chunks_layout([2, 0, 4], 512, 128, False)
    assert sample_first.tolist() == [0, 256, 256] and frame_first.tolist() == [0, 2, 2, 6] and n_samples == 768


def test_layout_errors():
    for bad in ([1, -1], [-3]):
        with pytest.raises(ValueError):
            sharding.stream_chunks_layout(bad, N, 256, True)
    for n, hop in ((N, 0), (N, -256), (N, 255), (1023, 256), (256, 512)):
        with pytest.raises(ValueError):
            sharding.stream_chunks_layout([1, 2], n, hop, False)


def test_stream_ids_split_over_ranks_with_stream_shard():
    # a live stream lives on one device: ranks own whole streams
    seen = []
    for rank in range(3):
        first, count = sharding.stream_shard(10, rank, 3)
        seen.extend(range(first, first + count))
    assert seen == list(range(10))


def test_streams_entries_are_bound_and_declared():
    from jeicyboodsp_amd._lib import lib
    assert lib.jdsp_abi_version() == 2
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    for name, n_args in (("jdsp_stftmask_streams_reserve", 2), ("jdsp_stftmask_streams_reset_dev", 3),
                         ("jdsp_stftmask_streams_dev", 11), ("jdsp_stftmask_streams_flush_dev", 6),
                         ("jdsp_stftmask_streams", 11), ("jdsp_stftmask_streams_flush", 7),
                         ("jdsp_istft_streams_reserve", 2), ("jdsp_istft_streams_reset_dev", 3),
                         ("jdsp_istft_streams_dev", 10), ("jdsp_istft_streams_flush_dev", 6),
                         ("jdsp_istft_streams", 10), ("jdsp_istft_streams_flush", 7)):
        assert name + "(" in txt, name
        assert len(getattr(lib, name).argtypes) == n_args, name
