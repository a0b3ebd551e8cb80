"""Batched fused STFT masking (jdsp_stftmask_batch*, StftMask.process_batch): a batch of ragged utterances in one
launch against the single-stream path -- a fresh handle's process + flush per utterance, which tests/test_stftmask_gpu.py
pins to the FP64 restatement -- bit for bit, over hops, mask kinds, launch geometries, boundary geometries, mask
pitches, the host entry, simulated ranks; the handle's own stream untouched; the error paths.

test_against_restatement prints |float32 - restatement| / (1e-5 P g) per utterance (run with -s)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_stftmask_gpu import (BINS, HOPS, KINDS, N, bits, cast_i16, cfg_of, mask_of, pcm_of, restate, run,  # noqa: E402
                               stream_combo)

pytestmark = pytest.mark.gpu

SENT_I = np.int16(-12345)
SENT_F = np.float32(-7777.5)
GAPS = [0, 2, 6]                 # samples between one span's end and the next utterance's start
EMPTY = 10                       # samples of an utterance too short for a frame


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


class Batch:
    """Utterances of the frame counts `frames` packed with the gaps GAPS (in turn) behind their spans; the gap and
    the too-short utterances' samples are full scale, so reading one would show."""

    def __init__(self, rng, kind, hop, frames, pitch=BINS, one_row=False):
        self.hop, self.frames = hop, list(frames)
        self.spans = [hop * (f - 1) + N if f else 0 for f in self.frames]
        lens = [(s if f else EMPTY) + GAPS[u % 3] for u, (f, s) in enumerate(zip(self.frames, self.spans))]
        self.offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.frames)]).astype(np.int64)
        self.pcm = np.full(int(self.offs[-1]), 32767, np.int16)
        for u, f in enumerate(self.frames):
            if f:
                self.pcm[self.offs[u]:self.offs[u] + self.spans[u]] = pcm_of(rng, f, hop)
        self.mask = mask_of(rng, kind, None if one_row else max(int(self.first[-1]), 1), pitch)

    def utt(self, u):
        """(pcm, mask rows, F) of utterance u as the single-stream path takes them"""
        a, f = int(self.offs[u]), self.frames[u]
        rows = self.mask if self.mask.ndim == 1 else self.mask[self.first[u]:self.first[u] + f]
        return self.pcm[a:a + self.spans[u]], rows, f

    def reference(self, eng, cfg):
        """per utterance (int16, float32) of a fresh handle's process + flush, None for an empty one"""
        ref = []
        for u, f in enumerate(self.frames):
            if not f:
                ref.append(None)
                continue
            o, fl, to, tf = run(eng, *self.utt(u), **cfg)
            ref.append((np.concatenate([o, to]), np.concatenate([fl, tf])))
        return ref

    def check(self, got_i, got_f, ref, outside_i, outside_f, what):
        """every utterance's span equals its reference, bit for bit; every other sample holds `outside`"""
        covered = np.zeros(self.pcm.size, bool)
        for u, f in enumerate(self.frames):
            if not f:
                continue
            a, b = int(self.offs[u]), int(self.offs[u]) + self.spans[u]
            covered[a:b] = True
            if got_i is not None:
                assert np.array_equal(got_i[a:b], ref[u][0]), (what, u, "int16")
            if got_f is not None:
                assert np.array_equal(got_f[a:b].view(np.int32), ref[u][1].view(np.int32)), (what, u, "float32")
        if got_i is not None:
            assert got_i.size == self.pcm.size and np.all(got_i[~covered] == outside_i), (what, "int16 outside the spans")
        if got_f is not None:
            assert got_f.size == self.pcm.size
            assert np.all(got_f[~covered].view(np.int32) == np.float32(outside_f).view(np.int32)), (what, "float32 outside")


def run_batch(sm, b, fpw=0, d_pcm=None, d_mask=None):
    """the device path into sentinel-filled outputs -> (int16, float32) as numpy"""
    import torch
    sm.set_option("frames_per_wave", fpw)
    d_pcm = torch.from_numpy(b.pcm).cuda() if d_pcm is None else d_pcm
    d_mask = torch.from_numpy(b.mask).cuda() if d_mask is None else d_mask
    out = torch.full((max(b.pcm.size, 1),), int(SENT_I), dtype=torch.int16, device="cuda")
    f32 = torch.full((max(b.pcm.size, 1),), float(SENT_F), dtype=torch.float32, device="cuda")
    o, f = sm.process_batch(d_pcm, d_mask, b.offs, want_f32=True, out=out, out_f32=f32)
    torch.cuda.synchronize()
    return o.cpu().numpy(), f.cpu().numpy()


def equal_on_device(eng, b, cfg, fpws, what):
    ref = b.reference(eng, cfg)
    sm = eng.stft_mask(**cfg)
    for fpw in fpws:
        o, f = run_batch(sm, b, fpw)
        b.check(o, f, ref, SENT_I, SENT_F, (what, "frames_per_wave", fpw))
    sm.close()
    return ref


# ---- 1. bit identity over the grid ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", HOPS)
def test_bit_identical_to_single_streams(eng, hop, kind):
    R = N // hop
    frames = [1, 0] + ([R - 1] if R > 1 else []) + [R, 2, 0, 0, 9, 1, 1, 37]
    b = Batch(np.random.default_rng(7000 + hop + len(kind)), kind, hop, frames)
    # 64: one wave walks every utterance; the small values start and end runs inside utterances
    equal_on_device(eng, b, cfg_of(hop, kind, stream_combo(hop)), sorted({0, max(R - 1, 1), 3, 5, 64}), (hop, kind))


# ---- 2. boundary geometry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("frames,fpw", [
    ([4, 4, 4], 4),              # a run starts on an utterance's first frame: no halo, nothing of the one before
    ([5, 5], 3),                 # a run starts one frame into utterance 1: a halo of 1 < R - 1
    ([3, 6, 0, 0, 0], 4),        # the last utterances are empty
    ([0, 0, 5, 4], 3),           # the first are empty
    ([0, 7, 0], 0),
], ids=["run-at-first-frame", "short-halo", "empty-last", "empty-first", "empty-around"])
def test_boundary_geometry(eng, frames, fpw, kind):
    hop = 256                                                      # R = 4
    b = Batch(np.random.default_rng(7100 + len(frames) + fpw), kind, hop, frames)
    equal_on_device(eng, b, cfg_of(hop, kind, stream_combo(hop)), [fpw], frames)


# ---- 3. mask pitch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", HOPS)
def test_mask_pitch(eng, hop, kind):
    frames = [3, 0, 1, 6]
    cfg = cfg_of(hop, kind, stream_combo(hop))
    padded = Batch(np.random.default_rng(7200 + hop), kind, hop, frames, pitch=520)
    equal_on_device(eng, padded, cfg, [0, 3], "pitch 520")
    one = Batch(np.random.default_rng(7300 + hop), kind, hop, frames, one_row=True)
    assert one.mask.ndim == 1
    equal_on_device(eng, one, cfg, [0, 3], "pitch 0")


# ---- 4. the FP64 restatement ---------------------------------------------------------------------------------------
def test_against_restatement(eng):
    hop, kind, combo = 512, "real", stream_combo(512)
    b = Batch(np.random.default_rng(7400), kind, hop, [5, 1, 12])
    sm = eng.stft_mask(**cfg_of(hop, kind, combo))
    got_i, got_f = run_batch(sm, b)
    sm.close()
    worst = 0.0
    for u, F in enumerate(b.frames):
        pcm, rows, _ = b.utt(u)
        em, tail, P, g = restate(pcm, rows, F, hop, *combo)
        want = np.concatenate([em, tail])
        tol = 1e-5 * P * np.resize(g, want.size)
        a = int(b.offs[u])
        gf, gi = got_f[a:a + want.size].astype(np.float64), got_i[a:a + want.size]
        ratio = float(np.max(np.abs(gf - want) / tol))
        worst = max(worst, ratio)
        print("stftmask batch utterance %d (F %d): max |err| / (1e-5 P g) = %.4f" % (u, F, ratio))
        assert np.all(np.abs(gf - want) <= tol), (u, ratio)
        assert np.array_equal(gi, cast_i16(gf.astype(np.float32))), u
        d = gi.astype(np.int64) - cast_i16(want).astype(np.int64)
        assert np.all(np.abs(d) <= 1), (u, np.abs(d).max())
    print("stftmask batch: worst ratio %.4f" % worst)


# ---- 5. the handle's own stream ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_handle_stream_is_independent(eng, kind):
    import torch
    hop, F, k = 512, 10, 4
    rng = np.random.default_rng(7500 + len(kind))
    cfg = cfg_of(hop, kind, stream_combo(hop))
    pcm = torch.from_numpy(pcm_of(rng, F, hop)).cuda()
    mask = torch.from_numpy(mask_of(rng, kind, F)).cuda()
    b = Batch(rng, kind, hop, [2, 0, 5])
    ref = b.reference(eng, cfg)
    sm = eng.stft_mask(**cfg)

    def stream(with_batch):
        oa, fa = sm.process(pcm, mask[:k], k, want_f32=True)
        oa, fa = oa.clone(), fa.clone()
        if with_batch:
            o, f = run_batch(sm, b)
            b.check(o, f, ref, SENT_I, SENT_F, "between two calls of the handle's stream")
        ob, fb = sm.process(pcm[hop * k:], mask[k:], F - k, want_f32=True)
        t, tf = sm.flush(want_f32=True)
        torch.cuda.synchronize()
        return torch.cat([oa, ob, t]), bits(torch.cat([fa, fb, tf]))

    plain, mixed = stream(False), stream(True)
    assert torch.equal(plain[0], mixed[0]) and torch.equal(plain[1], mixed[1])
    sm.close()


# ---- 6. the host entry, NULL outputs, empty batches ----------------------------------------------------------------
def vp(a, off=0):
    if a is None:
        return None
    return C.c_void_p((a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) + off)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", HOPS)
def test_host_entry_and_null_outputs(eng, hop, kind):
    import torch
    from jeicyboodsp_amd._lib import lib as L
    cfg = cfg_of(hop, kind, stream_combo(hop))
    b = Batch(np.random.default_rng(7600 + hop + len(kind)), kind, hop, [2, 0, 7, 1], pitch=520)
    ref = equal_on_device(eng, b, cfg, [0], "device")
    sm = eng.stft_mask(**cfg)
    # numpy in and out: the same values, zeros outside the spans (the outputs given are overwritten everywhere)
    o, f = sm.process_batch(b.pcm, b.mask, b.offs, want_f32=True, out=np.full(b.pcm.size, SENT_I),
                            out_f32=np.full(b.pcm.size, SENT_F))
    b.check(o, f, ref, 0, 0.0, "host")
    b.check(sm.process_batch(b.pcm, b.mask, b.offs), None, ref, 0, 0.0, "host, float32 NULL")
    sample_first, n_utts, n_total = np.ascontiguousarray(b.offs[:-1]), len(b.frames), int(b.first[-1])
    f = np.full(b.pcm.size, SENT_F)
    assert L.jdsp_stftmask_batch(sm._h, vp(b.pcm), b.pcm.size, vp(b.mask), 520, vp(sample_first), vp(b.first), n_utts,
                                 None, vp(f)) == 0
    b.check(None, f, ref, 0, 0.0, "host, int16 NULL")
    # the device entry with either output NULL
    d_pcm, d_mask = torch.from_numpy(b.pcm).cuda(), torch.from_numpy(b.mask).cuda()
    d_sample, d_first = torch.from_numpy(sample_first).cuda(), torch.from_numpy(b.first).cuda()
    d_o = torch.full((b.pcm.size,), int(SENT_I), dtype=torch.int16, device="cuda")
    d_f = torch.full((b.pcm.size,), float(SENT_F), dtype=torch.float32, device="cuda")
    eng._use_torch_stream()
    call = lambda *a: L.jdsp_stftmask_batch_dev(sm._h, vp(d_pcm), vp(d_mask), 520, vp(d_sample), vp(d_first), *a)  # noqa: E731
    assert call(n_utts, n_total, vp(d_o), None) == 0
    assert call(n_utts, n_total, None, vp(d_f)) == 0
    assert call(n_utts, n_total, None, None) == 0
    torch.cuda.synchronize()
    b.check(d_o.cpu().numpy(), d_f.cpu().numpy(), ref, SENT_I, SENT_F, "device, one output at a time")
    # nothing to do: no utterances, no frames, only empty utterances
    assert L.jdsp_stftmask_batch(sm._h, None, 0, None, 0, None, None, 0, None, None) == 0
    assert call(0, 0, vp(d_o), vp(d_f)) == 0
    assert L.jdsp_stftmask_batch_dev(sm._h, None, None, 0, None, None, 0, 0, None, None) == 0
    e = Batch(np.random.default_rng(1), kind, hop, [0, 0, 0])
    o, f = sm.process_batch(e.pcm, e.mask, e.offs, want_f32=True, out=np.full(e.pcm.size, SENT_I),
                            out_f32=np.full(e.pcm.size, SENT_F))
    assert o.size == e.pcm.size and not o.any() and not f.any()
    o, f = run_batch(sm, e)
    e.check(o, f, [None] * 3, SENT_I, SENT_F, "only empty utterances")
    sm.close()


# ---- 7. errors -----------------------------------------------------------------------------------------------------
def test_errors(eng):
    import torch
    from jeicyboodsp_amd._lib import lib as L
    hop, kind = 512, "real"
    cfg = cfg_of(hop, kind, stream_combo(hop))
    b = Batch(np.random.default_rng(7700), kind, hop, [2, 3, 1])
    ref = b.reference(eng, cfg)
    sm = eng.stft_mask(**cfg)
    out = np.zeros(b.pcm.size, np.int16)
    good_s, good_f, n = np.ascontiguousarray(b.offs[:-1]), b.first, len(b.frames)

    def host(s=good_s, f=good_f, n_utts=n, n_samples=b.pcm.size, pitch=BINS):
        s, f = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(f, np.int64)
        return L.jdsp_stftmask_batch(sm._h, vp(b.pcm), n_samples, vp(b.mask), pitch, vp(s), vp(f), n_utts, vp(out), None)

    def poke(a, i, d):
        a = a.copy()
        a[i] += d
        return a

    bad = {
        "decreasing frame_first": dict(f=[0, 5, 2, 6]),
        "frame_first[0] != 0": dict(f=good_f + 1),
        "an odd sample_first": dict(s=poke(good_s, 1, 1)),
        "overlapping spans": dict(s=poke(good_s, 1, -2)),
        "sample_first descending": dict(s=good_s[::-1]),
        "a negative sample_first": dict(s=poke(good_s, 0, -2)),
        "a span past n_samples": dict(n_samples=int(b.offs[2]) + b.spans[2] - 2),
        "one frame too many in the last utterance": dict(f=poke(good_f, 3, 1)),
        "mask_pitch 256": dict(pitch=256),
        "negative n_utts": dict(n_utts=-1),
    }
    assert host() == 0
    for what, kw in bad.items():
        assert host(**kw) == -1, what
        assert b"jdsp_stftmask_batch" in L.jdsp_last_error(eng._h), what
    # the device entry: base pointers and counts only -- offsets on the device are the caller's contract
    d_pcm, d_mask = torch.from_numpy(b.pcm).cuda(), torch.from_numpy(b.mask).cuda()
    d_s, d_f = torch.from_numpy(good_s).cuda(), torch.from_numpy(good_f).cuda()
    d_o = torch.zeros(b.pcm.size + 8, dtype=torch.int16, device="cuda")
    d_f32 = torch.zeros(b.pcm.size + 8, dtype=torch.float32, device="cuda")
    total = int(good_f[-1])

    def dev(pcm=vp(d_pcm), mask=vp(d_mask), pitch=BINS, s=vp(d_s), f=vp(d_f), n_utts=n, n_total=total, o=vp(d_o), f32=None):
        return L.jdsp_stftmask_batch_dev(sm._h, pcm, mask, pitch, s, f, n_utts, n_total, o, f32)

    for what, kw in {
        "pcm not 4-aligned": dict(pcm=vp(d_pcm, 2)), "mask not element-aligned": dict(mask=vp(d_mask, 2)),
        "int16 out not 4-aligned": dict(o=vp(d_o, 2)), "float out not 8-aligned": dict(o=None, f32=vp(d_f32, 4)),
        "sample_first not 8-aligned": dict(s=vp(d_s, 4)), "frame_first not 8-aligned": dict(f=vp(d_f, 4)),
        "negative n_utts": dict(n_utts=-1), "negative n_frames_total": dict(n_total=-1), "mask_pitch 512": dict(pitch=512),
    }.items():
        assert dev(**kw) == -1, what
        assert b"jdsp_stftmask_batch" in L.jdsp_last_error(eng._h), what
    # the handle is still usable, for the batch and for its own stream
    o, f = run_batch(sm, b)
    b.check(o, f, ref, SENT_I, SENT_F, "after the errors")
    pcm, rows, F = b.utt(1)
    o = sm.process(torch.from_numpy(pcm).cuda(), torch.from_numpy(rows).cuda(), F)
    t = sm.flush()
    torch.cuda.synchronize()
    assert np.array_equal(np.concatenate([o.cpu().numpy(), t.cpu().numpy()]), ref[1][0])
    sm.close()


# ---- 8. simulated ranks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_simulated_ranks(eng, kind):
    import torch
    from jeicyboodsp_amd import sharding
    hop = 256
    b = Batch(np.random.default_rng(7800 + len(kind)), kind, hop, [1, 0, 3, 4, 2, 0, 0, 9, 1, 1, 37])
    sm = eng.stft_mask(**cfg_of(hop, kind, stream_combo(hop)))
    counts, first = sharding.stftmask_batch_layout(b.offs, N, hop)
    assert counts.tolist() == b.frames and first.tolist() == b.first.tolist()
    d_pcm, d_mask = torch.from_numpy(b.pcm).cuda(), torch.from_numpy(b.mask).cuda()
    whole = sm.process_batch(d_pcm, d_mask, b.offs, want_f32=True)
    whole = [t.clone() for t in whole]
    for world in (1, 2, 3):
        parts, fparts = [], []
        for rank in range(world):
            u0, nu = sharding.stftmask_batch_shard(counts, rank, world)
            lo, hi = int(b.offs[u0]), int(b.offs[u0 + nu])
            o, f = sm.process_batch(d_pcm[lo:hi], d_mask[int(first[u0]):max(int(first[u0 + nu]), int(first[u0]) + 1)],
                                    b.offs[u0:u0 + nu + 1] - lo, want_f32=True)
            parts.append(o[:hi - lo].clone())
            fparts.append(f[:hi - lo].clone())
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts), whole[0]), world
        assert torch.equal(bits(torch.cat(fparts)), bits(whole[1])), world
    sm.close()
