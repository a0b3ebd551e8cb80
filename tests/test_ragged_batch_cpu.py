"""CPU tests of the host side of the ragged-batch analysis and synthesis (jdsp_stft_half_batch*, jdsp_istft_batch*):
the back-to-back packing of a batch of synthesis outputs (sharding.istft_batch_layout), the header declarations and
ctypes bindings of the four entries, the ABI version, the NULL context / handle answers, which need no device, and
the two helpers every batch method of engine.py allocates through (the device-offset cache, the output buffers)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jeicyboodsp_amd import sharding  # noqa: E402

ENTRIES = (("jdsp_stft_half_batch_dev", 9), ("jdsp_stft_half_batch", 9), ("jdsp_istft_batch_dev", 9),
           ("jdsp_istft_batch", 9))


@pytest.mark.parametrize("n,hop", [(1024, 1024), (1024, 512), (1024, 256), (512, 512), (512, 256), (512, 128)])
def test_layout_spans_evenness_and_empty_utterances(n, hop):
    counts = [1, 0, n // hop, 2, 0, 0, 9, 1, 1, 37, 0]
    offs, first = sharding.istft_batch_layout(counts, n, hop)
    assert offs.dtype == np.int64 and first.dtype == np.int64
    assert offs.size == len(counts) + 1 and first.size == len(counts) + 1
    assert offs[0] == 0 and first.tolist() == [0] + np.cumsum(counts).tolist()
    assert not np.any(offs & 1)                                    # even by construction
    for u, f in enumerate(counts):
        span = int(offs[u + 1] - offs[u])
        assert span == (hop * (f - 1) + n if f else 0), u          # back to back: no gap, an empty one takes nothing
    # the inverse of stftmask_batch_layout on its own output
    c2, f2 = sharding.stftmask_batch_layout(offs, n, hop)
    assert c2.tolist() == counts and f2.tolist() == first.tolist()
    # a numpy array gives the same; no utterance at all
    o3, f3 = sharding.istft_batch_layout(np.asarray(counts, np.int32), n, hop)
    assert o3.tolist() == offs.tolist() and f3.tolist() == first.tolist()
    o0, f0 = sharding.istft_batch_layout([], n, hop)
    assert o0.tolist() == [0] and f0.tolist() == [0]
    oe, fe = sharding.istft_batch_layout([0, 0, 0], n, hop)
    assert oe.tolist() == [0, 0, 0, 0] and fe.tolist() == [0, 0, 0, 0]


def test_layout_rejects_negative_counts():
    with pytest.raises(ValueError):
        sharding.istft_batch_layout([3, -1, 2], 1024, 512)
    with pytest.raises(ValueError):
        sharding.istft_batch_layout([-5], 512, 128)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_whole_utterance_split_reuses_the_masking_shard(world):
    counts = [1, 0, 3, 4, 2, 0, 0, 9, 1, 1, 37]
    offs, first = sharding.istft_batch_layout(counts, 1024, 256)
    seen = []
    for rank in range(world):
        u0, nu = sharding.stftmask_batch_shard(counts, rank, world)
        assert u0 == len(seen)
        seen.extend(range(u0, u0 + nu))
        # a rank's rebased offsets are the layout of its own counts
        o, f = sharding.istft_batch_layout(counts[u0:u0 + nu], 1024, 256)
        assert o.tolist() == (offs[u0:u0 + nu + 1] - offs[u0]).tolist()
        assert f.tolist() == (first[u0:u0 + nu + 1] - first[u0]).tolist()
    assert seen == list(range(len(counts)))
    assert "stft_half_batch" in sharding.stftmask_batch_shard.__doc__ and "process_batch" in sharding.stftmask_batch_shard.__doc__


def test_entries_are_declared_and_bound():
    from jeicyboodsp_amd._lib import lib
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n_args in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name          # the header's own argument count
        assert len(getattr(lib, name).argtypes) == n_args, name
    # the pitch rule of the batched analysis is stated in the header
    block = txt[txt.index("Half spectra of a batch"):txt.index("int jdsp_stft_half_batch_dev")]
    assert "EVEN" in block and "514" in block


def test_abi_version_is_still_2():
    from jeicyboodsp_amd._lib import lib
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    assert re.search(r"#define\s+JDSP_ABI_VERSION\s+2\b", txt)
    assert lib.jdsp_abi_version() == 2


def test_null_context_and_handle_are_einval_without_a_device():
    from jeicyboodsp_amd._lib import lib
    a = np.zeros(8, np.int64)
    p = a.ctypes.data
    assert lib.jdsp_stft_half_batch_dev(None, p, p, p, 1, 1, 512, p, 520) == -1
    assert lib.jdsp_stft_half_batch(None, p, 0, p, p, 0, 512, p, 520) == -1
    assert lib.jdsp_istft_batch_dev(None, p, 513, p, p, 1, 1, p, None) == -1
    assert lib.jdsp_istft_batch(None, p, 513, p, p, 0, 0, p, None) == -1
    # ... and with nothing to do as well
    assert lib.jdsp_stft_half_batch_dev(None, None, None, None, 0, 0, 512, None, 520) == -1
    assert lib.jdsp_istft_batch_dev(None, None, 513, None, None, 0, 0, None, None) == -1


class _Holder:
    pass


def test_offset_cache_keeps_the_last_batch_and_renews_on_any_change_of_key():
    import torch
    from jeicyboodsp_amd import engine
    cpu = torch.device("cpu")
    offs, counts = np.array([0, 1536, 1538, 4100], np.int64), np.array([2, 0, 4], np.int64)
    sample_first, first = np.ascontiguousarray(offs[:-1]), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    h = _Holder()
    key = (offs.tobytes(), counts.tobytes())
    a = engine._batch_offsets(h, key, sample_first, first, cpu)
    assert a[2] is True and a[0].tolist() == sample_first.tolist() and a[1].tolist() == first.tolist()
    assert a[0].dtype == torch.int64 and a[1].dtype == torch.int64 and a[0].device == cpu
    # an equal key (not the same object): the same two tensors, not fresh
    b = engine._batch_offsets(h, (offs.copy().tobytes(), counts.copy().tobytes()), sample_first, first, cpu)
    assert b[2] is False and b[0] is a[0] and b[1] is a[1]
    # the key covers the offsets, the counts and the device
    offs2, counts2 = offs + np.array([0, 0, 2, 2]), counts + np.array([0, 1, -1])
    for k, dev in (((offs2.tobytes(), counts.tobytes()), cpu), ((offs.tobytes(), counts2.tobytes()), cpu),
                   (key, torch.device("meta"))):
        h2 = _Holder()
        first_call = engine._batch_offsets(h2, key, sample_first, first, cpu)
        c = engine._batch_offsets(h2, k, sample_first, first, dev)
        assert c[2] is True and c[0] is not first_call[0] and c[1] is not first_call[1]
        assert c[0].device == dev and c[1].device == dev
        d = engine._batch_offsets(h2, k, sample_first, first, dev)      # ... and the new one is the one kept
        assert d[2] is False and d[0] is c[0] and d[1] is c[1]
    # two holders never share: an Engine's cache cannot meet a stream object's
    other = engine._batch_offsets(_Holder(), key, sample_first, first, cpu)
    assert other[2] is True and other[0] is not a[0]


def test_output_helper_zero_fills_at_least_one_element_and_keeps_a_given_buffer():
    import torch
    from jeicyboodsp_amd import engine
    cpu = torch.device("cpu")
    for n in (0, 1, 7):
        for dtype in (np.int16, np.float32, np.uint8):
            a = engine._batch_out(n, dtype, None)
            assert isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == (max(n, 1),) and not a.any()
            t = engine._batch_out(n, dtype, cpu)
            assert t.dtype == getattr(torch, np.dtype(dtype).name) and tuple(t.shape) == (max(n, 1),)
            assert t.device == cpu and not t.any()
        a = engine._batch_out(n, np.float32, None, tail=(1024,))
        t = engine._batch_out(n, np.float32, cpu, tail=(1024,))
        assert a.shape == (max(n, 1), 1024) and tuple(t.shape) == (max(n, 1), 1024) and not a.any() and not t.any()
    # a given buffer comes back as it is: the same object, not resized, not cleared
    given_np, given_t = np.full(3, 5, np.int16), torch.full((3,), 5, dtype=torch.int16)
    assert engine._batch_out(9, np.int16, None, given_np) is given_np and given_np.tolist() == [5, 5, 5]
    assert engine._batch_out(9, np.int16, cpu, given_t) is given_t and given_t.tolist() == [5, 5, 5]
