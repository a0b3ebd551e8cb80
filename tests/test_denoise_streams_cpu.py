"""The host side of the live denoise streams (jdsp_denoise_streams*, Denoiser.process_streams): the entries are
declared, exported and bound, and sharding.denoise_stream_emitted is the reference's call counter.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jeicyboodsp_amd import sharding  # noqa: E402

ENTRIES = (("jdsp_denoise_streams_reserve", 3), ("jdsp_denoise_streams_reset_dev", 3), ("jdsp_denoise_streams_dev", 11),
           ("jdsp_denoise_streams", 11), ("jdsp_denoise_streams_state", 5))


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
    for name in ("jdsp_denoise_streams_dev", "jdsp_denoise_streams_reset_dev"):
        conventions = txt[:txt.index("#ifndef JDSP_H")]
        assert name in conventions[conventions.index("Class D"):conventions.index("Class H")], name


def test_the_wrapper_has_the_methods():
    from jeicyboodsp_amd.engine import Denoiser
    for m in ("open_streams", "process_streams", "reset_streams", "streams_state"):
        assert callable(getattr(Denoiser, m)), m


def reference_call_counter(seen, blocks):
    """SS:260-263 as main() runs it: the counter goes up with every block, and a block is written out only once it has
    passed 2"""
    calls, emitted = seen, 0
    for _ in range(blocks):
        calls += 1
        if calls > 2:
            emitted += 1
    return emitted


def test_emitted_is_the_references_call_counter():
    for n in range(4):
        for b in range(6):
            assert sharding.denoise_stream_emitted([n], [b]).tolist() == [reference_call_counter(n, b)], (n, b)
    seen = [n for n in range(4) for _ in range(6)]
    counts = [b for _ in range(4) for b in range(6)]
    e = sharding.denoise_stream_emitted(seen, counts)
    assert e.dtype == np.int64
    assert e.tolist() == [reference_call_counter(n, b) for n, b in zip(seen, counts)]
    assert sharding.denoise_stream_emitted(1, [0, 1, 2, 5]).tolist() == [0, 0, 1, 4]      # a scalar stands for all chunks
    assert sharding.denoise_stream_emitted([], []).size == 0


def test_emitted_errors():
    for seen, counts in (([0, 1], [3]), ([-1], [3]), ([0], [-2]), ([0, 0, 0], [1, 2])):
        with pytest.raises(ValueError):
            sharding.denoise_stream_emitted(seen, counts)


def test_stream_ids_split_over_ranks_with_stream_shard():
    owned = []
    for rank in range(4):
        first, count = sharding.stream_shard(10, rank, 4)
        owned.extend(range(first, first + count))
    assert owned == list(range(10))
