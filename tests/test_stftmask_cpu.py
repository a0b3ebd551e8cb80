"""CPU tests of the fused STFT masking's host side: the ctypes binding of every jdsp_stftmask_* entry the header
declares, the unchanged ABI version, and the frame split sharding.stftmask_sharded walks."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jeicyboodsp_amd import sharding  # noqa: E402


def test_header_stftmask_entries_are_bound():
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(jdsp_stftmask_[a-z0-9_]+)\s*\(", txt)))
    assert len(names) >= 9, names
    src = open(os.path.join(ROOT, "jeicyboodsp_amd", "_lib.py")).read()
    missing = [n for n in names if '"%s"' % n not in src]
    assert not missing, missing
    from jeicyboodsp_amd._lib import lib
    for n in names:
        assert getattr(lib, n).argtypes is not None, n


def test_abi_version_is_still_2():
    from jeicyboodsp_amd._lib import lib
    assert lib.jdsp_abi_version() == 2
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    assert re.search(r"#define\s+JDSP_ABI_VERSION\s+2\b", txt)


class FakeStream:
    """Records what stftmask_sharded asks of a StftMask: (first sample, samples, mask rows, n_frames, write)."""

    def __init__(self, hop):
        self.n_fft, self.hop, self.calls, self.resets = 1024, hop, [], 0

    def reset(self):
        self.resets += 1

    def process(self, pcm, mask, n_frames, want_f32=False, write=True):
        self.calls.append((pcm.start, len(pcm), len(mask), n_frames, write))
        return n_frames


class Rows:
    ndim = 2

    def __init__(self, n):
        self.n = n

    def __getitem__(self, s):
        return range(self.n)[s]


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("hop", [1024, 512, 256])
@pytest.mark.parametrize("n_frames", [1, 5, 97])
def test_stftmask_sharded_covers_every_frame_once(world, hop, n_frames):
    R = 1024 // hop
    pcm = range(hop * (n_frames - 1) + 1024)
    seen = []
    for rank in range(world):
        s = FakeStream(hop)
        got = sharding.stftmask_sharded(s, pcm, Rows(n_frames), n_frames, world, rank)
        halo, first, end = sharding.istft_frame_shard(n_frames, world, rank, R)
        assert s.resets == 1
        if end == first:
            assert got is None and not s.calls
            continue
        want = []
        if first > halo:
            want.append((hop * halo, hop * (first - halo - 1) + 1024, first - halo, first - halo, False))
        want.append((hop * first, hop * (end - first - 1) + 1024, end - first, end - first, True))
        assert s.calls == want
        seen.extend(range(first, end))
    assert seen == list(range(n_frames))
