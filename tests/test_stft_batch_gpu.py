"""Ragged-batch STFT analysis (jdsp_stft_half_batch*, Engine.stft_half_batch): the half spectra of a batch of ragged
utterances in one launch against the single-stream entry run on every utterance alone --
Engine.stft(pcm_u, F_u, 1024, hop)[:, :513], which tests/test_stft_gpu.py pins to the oracle -- BIT FOR BIT, over hops,
windows, launch geometries, boundary geometries and pitches; against numpy.fft; the host entry; the error paths;
simulated ranks; one random batch.

Where a bit differs the assertion names the single-stream kernel the utterance was compared with
(stft1024_hop512_kernel for hop 512, stft1024_anyhop_kernel otherwise) and the worst |difference| / row peak."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_istft_gpu import pcm_of  # noqa: E402
from test_stft_gpu import _check  # noqa: E402

pytestmark = pytest.mark.gpu

N, BINS = 1024, 513
HOPS = [1024, 512, 256]
SENT = np.complex64(-7777.5 + 1234.25j)
GAPS = [0, 2, 6]                 # samples between one span's end and the next utterance's start
EMPTY = 10                       # samples of an utterance too short for a frame
SPARE = 2                        # rows behind the batch's last: they must keep the sentinel


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def untouched(a):
    """every element still holds the sentinel, bit for bit"""
    return bool(np.all(bits(a).reshape(-1, 2) == bits(np.array([SENT]))))


class Batch:
    """Utterances of the frame counts `frames` packed with the gaps GAPS (in turn) behind their spans; the gap and
    the too-short utterances' samples are full scale, so reading one would show."""

    def __init__(self, rng, hop, frames):
        self.hop, self.frames = hop, list(frames)
        self.spans = [hop * (f - 1) + N if f else 0 for f in self.frames]
        lens = [(s if f else EMPTY) + GAPS[u % 3] for u, (f, s) in enumerate(zip(self.frames, self.spans))]
        self.offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.frames)]).astype(np.int64)
        self.total = int(self.first[-1])
        self.pcm = np.full(int(self.offs[-1]), 32767, np.int16)
        for u, f in enumerate(self.frames):
            if f:
                self.pcm[self.offs[u]:self.offs[u] + self.spans[u]] = pcm_of(rng, self.spans[u])

    def utt(self, u):
        a = int(self.offs[u])
        return self.pcm[a:a + self.spans[u]]

    def reference(self, eng):
        """[total, 513] complex64: every utterance through the single-stream entry on its own (one buffer each)"""
        import torch
        parts = [eng.stft(torch.from_numpy(self.utt(u)).cuda(), f, N, self.hop)[:, :BINS] for u, f in enumerate(self.frames) if f]
        torch.cuda.synchronize()
        if not parts:
            return np.zeros((0, BINS), np.complex64)
        return torch.cat(parts).cpu().numpy()


def run_batch(eng, b, fpw=0, pitch=520, d_pcm=None):
    """the device entry into a sentinel-filled [total + SPARE, pitch] tensor -> numpy"""
    import torch
    d_pcm = torch.from_numpy(b.pcm).cuda() if d_pcm is None else d_pcm
    out = torch.full((b.total + SPARE, pitch), complex(SENT), dtype=torch.complex64, device="cuda")
    eng.set_option("stft.frames_per_wave", fpw)
    try:
        got = eng.stft_half_batch(d_pcm, b.offs, hop=b.hop, pitch=pitch, out=out)
    finally:
        eng.set_option("stft.frames_per_wave", 0)
    torch.cuda.synchronize()
    assert got.shape == (b.total, pitch)
    return out.cpu().numpy()


def check(b, full, want, what):
    """rows 0..total-1, bins 0..512 equal `want` bit for bit; every other element holds the sentinel"""
    got = full[:b.total, :BINS]
    if not np.array_equal(bits(got), bits(want)):
        pair = "stft_half_batch_kernel against " + ("stft1024_hop512_kernel" if b.hop == 512 else "stft1024_anyhop_kernel")
        peak = np.abs(want).max(axis=1)
        rel = np.abs(got.astype(np.complex128) - want).max(axis=1) / np.where(peak > 0, peak, 1)
        bad = np.flatnonzero((bits(got) != bits(want)).reshape(b.total, -1).any(axis=1))
        raise AssertionError("%s: %s differ in %d of %d rows (first %s), worst |d| / row peak %.3g"
                             % (what, pair, bad.size, b.total, bad[:8].tolist(), rel.max()))
    assert untouched(full[:b.total, BINS:]), (what, "columns past 512 written")
    assert untouched(full[b.total:]), (what, "rows past the batch written")


def equal_on_device(eng, b, fpws, what, pitch=520):
    want = b.reference(eng)
    for fpw in fpws:
        check(b, run_batch(eng, b, fpw, pitch), want, (what, "frames_per_wave", fpw))
    return want


# ---- 1. bit identity over hops, windows and launch geometries -------------------------------------------------------
@pytest.mark.parametrize("window", [0, 1], ids=["hamming", "hann"])
@pytest.mark.parametrize("hop", HOPS)
def test_bit_identical_to_single_streams(eng, hop, window):
    R = N // hop
    frames = [1, 0] + ([R - 1] if R > 1 else []) + [R, 2, 0, 0, 9, 1, 1, 37]
    b = Batch(np.random.default_rng(8000 + hop + window), hop, frames)
    eng.set_option("stft.window", window)
    try:
        # 64: one wave walks every utterance; the small values start and end runs inside utterances
        equal_on_device(eng, b, [0, 1, 2, 3, 5, 64], (hop, window))
    finally:
        eng.set_option("stft.window", 0)


# ---- 2. boundary geometry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,fpw", [
    ([4, 4, 4], 4),              # a run starts on an utterance's first frame
    ([5, 5], 3),                 # a run starts one frame into utterance 1
    ([3, 6, 0, 0, 0], 4),        # the last utterances are empty
    ([0, 0, 5, 4], 3),           # the first are empty
    ([0, 7, 0], 0),
], ids=["run-at-first-frame", "one-frame-in", "empty-last", "empty-first", "empty-around"])
def test_boundary_geometry(eng, frames, fpw):
    b = Batch(np.random.default_rng(8100 + len(frames) + fpw), 256, frames)
    equal_on_device(eng, b, [fpw], frames)


# ---- 3. pitch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", HOPS)
def test_pitch(eng, hop):
    b = Batch(np.random.default_rng(8200 + hop), hop, [3, 0, 1, 6])
    want = b.reference(eng)
    for pitch in (514, 520, 1024):
        for fpw in (0, 3):
            check(b, run_batch(eng, b, fpw, pitch), want, ("pitch", pitch, fpw))


# ---- 4. numpy.fft --------------------------------------------------------------------------------------------------
def test_against_numpy_fft(eng):
    hop = 256
    b = Batch(np.random.default_rng(8300), hop, [5, 0, 1, 12])
    got = run_batch(eng, b)[:b.total, :BINS].astype(np.complex128)
    w = 0.54 - 0.46 * np.cos(2 * 3.141592 * np.arange(N) / (N - 1))
    want = []
    for u, f in enumerate(b.frames):
        x = b.utt(u).astype(np.float64)
        want += [np.fft.fft(x[hop * k: hop * k + N] * w)[:BINS] for k in range(f)]
    _check(got, np.array(want))


# ---- 5. the host entry ---------------------------------------------------------------------------------------------
def vp(a, off=0):
    if a is None:
        return None
    return C.c_void_p((a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) + off)


@pytest.mark.parametrize("hop", HOPS)
def test_host_entry_and_empty_batches(eng, hop):
    import torch
    from jeicyboodsp_amd._lib import lib as L
    b = Batch(np.random.default_rng(8400 + hop), hop, [2, 0, 7, 1])
    dev = run_batch(eng, b)
    out = np.full((b.total + SPARE, 520), SENT)
    got = eng.stft_half_batch(b.pcm, b.offs, hop=hop, pitch=520, out=out)
    assert got.shape == (b.total, 520)
    check(b, out, dev[:b.total, :BINS], "host against device")            # and the host's padding is left alone
    fresh = eng.stft_half_batch(b.pcm, b.offs, hop=hop)
    assert np.array_equal(bits(fresh[:, :BINS]), bits(dev[:b.total, :BINS]))
    # nothing to do: no utterances, no frames, only empty utterances
    assert L.jdsp_stft_half_batch(eng._h, None, 0, None, None, 0, hop, None, 520) == 0
    assert L.jdsp_stft_half_batch_dev(eng._h, None, None, None, 0, 0, hop, None, 520) == 0
    e = Batch(np.random.default_rng(1), hop, [0, 0, 0])
    assert eng.stft_half_batch(e.pcm, e.offs, hop=hop).shape == (0, 520)
    full = run_batch(eng, e)
    check(e, full, np.zeros((0, BINS), np.complex64), "only empty utterances")
    d_s, d_f = torch.from_numpy(np.ascontiguousarray(e.offs[:-1])).cuda(), torch.from_numpy(e.first).cuda()
    d_pcm = torch.from_numpy(e.pcm).cuda()
    spec = torch.full((SPARE, 520), complex(SENT), dtype=torch.complex64, device="cuda")
    eng._use_torch_stream()
    assert L.jdsp_stft_half_batch_dev(eng._h, vp(d_pcm), vp(d_s), vp(d_f), 3, 0, hop, vp(spec), 520) == 0
    torch.cuda.synchronize()
    assert untouched(spec.cpu().numpy())


# ---- 6. errors -----------------------------------------------------------------------------------------------------
def test_errors(eng):
    import torch
    from jeicyboodsp_amd._lib import lib as L
    hop = 512
    b = Batch(np.random.default_rng(8500), hop, [2, 3, 1])
    want = b.reference(eng)
    good_s, good_f, n = np.ascontiguousarray(b.offs[:-1]), b.first, len(b.frames)
    out = np.full((b.total, 520), SENT)

    def host(s=good_s, f=good_f, n_utts=n, n_samples=b.pcm.size, hop=hop, pitch=520):
        s, f = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(f, np.int64)
        return L.jdsp_stft_half_batch(eng._h, vp(b.pcm), n_samples, vp(s), vp(f), n_utts, hop, vp(out), pitch)

    def poke(a, i, d):
        a = a.copy()
        a[i] += d
        return a

    bad = {
        "decreasing frame_first": dict(f=[0, 5, 2, 6]),
        "frame_first[0] != 0": dict(f=good_f + 1),
        "an odd sample_first": dict(s=poke(good_s, 1, 1)),
        "overlapping spans": dict(s=poke(good_s, 1, -2)),
        "a span past n_samples": dict(n_samples=int(b.offs[2]) + b.spans[2] - 2),
        "odd pitch": dict(pitch=521), "pitch 513": dict(pitch=513), "pitch 512": dict(pitch=512),
        "hop 128": dict(hop=128), "hop 300": dict(hop=300),
        "negative n_utts": dict(n_utts=-1),
    }
    assert host() == 0
    assert np.array_equal(bits(out[:, :BINS]), bits(want))
    out[:] = SENT
    for what, kw in bad.items():
        assert host(**kw) == -1, what
        assert b"jdsp_stft_half_batch" in L.jdsp_last_error(eng._h), what
    assert untouched(out)                      # nothing was written
    # the device entry: base pointers, counts, hop and pitch -- offsets on the device are the caller's contract
    d_pcm = torch.from_numpy(b.pcm).cuda()
    d_s, d_f = torch.from_numpy(good_s).cuda(), torch.from_numpy(good_f).cuda()
    spec = torch.full((b.total + SPARE, 1024), complex(SENT), dtype=torch.complex64, device="cuda")
    eng._use_torch_stream()

    def dev(pcm=vp(d_pcm), s=vp(d_s), f=vp(d_f), n_utts=n, n_total=b.total, hop=hop, o=vp(spec), pitch=1024):
        return L.jdsp_stft_half_batch_dev(eng._h, pcm, s, f, n_utts, n_total, hop, o, pitch)

    for what, kw in {
        "odd pitch": dict(pitch=521), "pitch 513": dict(pitch=513), "pitch 512": dict(pitch=512),
        "hop 128": dict(hop=128), "hop 300": dict(hop=300),
        "spec not 16-aligned": dict(o=vp(spec, 8)), "pcm not 4-aligned": dict(pcm=vp(d_pcm, 2)),
        "sample_first not 8-aligned": dict(s=vp(d_s, 4)), "frame_first not 8-aligned": dict(f=vp(d_f, 4)),
        "negative n_utts": dict(n_utts=-1), "negative n_frames_total": dict(n_total=-1),
    }.items():
        assert dev(**kw) == -1, what
        assert len(L.jdsp_last_error(eng._h)) > 0 and b"jdsp_stft_half_batch" in L.jdsp_last_error(eng._h), what
    torch.cuda.synchronize()
    assert untouched(spec.cpu().numpy())       # nothing was launched
    # the context is still usable
    assert dev() == 0
    torch.cuda.synchronize()
    check(b, spec.cpu().numpy(), want, "after the errors")


# ---- 7. simulated ranks --------------------------------------------------------------------------------------------
def test_simulated_ranks(eng):
    import torch
    from jeicyboodsp_amd import sharding
    hop = 256
    b = Batch(np.random.default_rng(8600), hop, [1, 0, 3, 4, 2, 0, 0, 9, 1, 1, 37])
    counts, first = sharding.stftmask_batch_layout(b.offs, N, hop)
    assert counts.tolist() == b.frames and first.tolist() == b.first.tolist()
    d_pcm = torch.from_numpy(b.pcm).cuda()
    whole = eng.stft_half_batch(d_pcm, b.offs, hop=hop)[:, :BINS].clone()
    for world in (1, 2, 3, 8):
        parts = []
        for rank in range(world):
            u0, nu = sharding.stftmask_batch_shard(counts, rank, world)
            lo, hi = int(b.offs[u0]), int(b.offs[u0 + nu])
            got = eng.stft_half_batch(d_pcm[lo:hi], b.offs[u0:u0 + nu + 1] - lo, hop=hop)
            assert got.shape[0] == int(first[u0 + nu] - first[u0])
            parts.append(got[:, :BINS].clone())
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(torch.cat(parts)).view(torch.int32),
                           torch.view_as_real(whole).view(torch.int32)), world


# ---- 8. a random batch ---------------------------------------------------------------------------------------------
def test_random_batch_of_300_utterances(eng):
    rng = np.random.default_rng(8700)
    b = Batch(rng, 512, rng.integers(0, 41, 300).tolist())
    equal_on_device(eng, b, [0], "300 utterances")
