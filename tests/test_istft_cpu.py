"""CPU tests of the STFT synthesis' host side: the frame sharding of sharding.istft_frame_shard, and the ctypes
binding of every jdsp_istft_* entry the header declares."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jeicyboodsp_amd import sharding  # noqa: E402


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("n_frames", [0, 1, 5, 97, 65536])
def test_istft_frame_shard_covers_every_frame_once(world, R, n_frames):
    seen = []
    prev_end = 0
    for rank in range(world):
        halo, first, end = sharding.istft_frame_shard(n_frames, world, rank, R)
        assert first == prev_end and first <= end
        assert halo == max(first - (R - 1), 0)
        seen.extend(range(first, end))
        prev_end = end
    assert seen == list(range(n_frames))


def test_header_istft_entries_are_bound():
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(jdsp_istft_[a-z0-9_]+)\s*\(", txt)))
    assert len(names) >= 8
    src = open(os.path.join(ROOT, "jeicyboodsp_amd", "_lib.py")).read()
    missing = [n for n in names if '"%s"' % n not in src]
    assert not missing, missing
