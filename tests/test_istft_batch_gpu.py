"""Ragged-batch STFT synthesis (jdsp_istft_batch*, Istft.process_batch): a batch of ragged utterances in one launch
against the single-stream path -- a fresh handle's process + flush per utterance, which tests/test_istft_gpu.py pins to
the FP64 restatement -- bit for bit, over all twelve (n, hop, layout) configurations, launch geometries, boundary
geometries, row pitches, the host entry, simulated ranks; the handle's own stream untouched; the error paths; and the
round trip through the batched analysis (Engine.stft_half_batch) back to the PCM."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_istft_gpu import CONFIGS, check_against_restatement, rows, run  # noqa: E402
from test_stft_batch_gpu import Batch as PcmBatch  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_I = np.int16(-12345)
SENT_F = np.float32(-7777.5)
GAPS = [0, 2, 6]                 # samples between one span's end and the next utterance's start
EMPTY = 10                       # samples left for an utterance without a frame


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def fbits(t):
    import torch
    return t.view(torch.int32)


def cfg_of(n, hop, layout, syn="hann", ana="hann"):
    # Hann / Hann has a WOLA inverse for every R > 1; at R = 1 the analysis window would vanish at the frame's ends
    if n == hop:
        syn, ana = "hamming", "none"
    return dict(n_fft=n, hop=hop, layout=layout, synthesis_window=syn, analysis_window=ana)


class Batch:
    """Spectrum rows of utterances with the frame counts `frames`, and output spans packed with the gaps GAPS (in
    turn) behind them; an utterance without a frame still owns EMPTY samples, which nothing may write."""

    def __init__(self, rng, n, hop, layout, frames, pitch=None):
        self.n, self.hop, self.layout, self.frames = n, hop, layout, list(frames)
        self.bins = n // 2 + 1 if layout == "half" else n
        self.pitch = pitch or self.bins
        self.spans = [hop * (f - 1) + n if f else 0 for f in self.frames]
        lens = [(s if f else EMPTY) + GAPS[u % 3] for u, (f, s) in enumerate(zip(self.frames, self.spans))]
        self.offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.frames)]).astype(np.int64)
        self.total, self.size = int(self.first[-1]), int(self.offs[-1])
        self.spec = rows(rng, max(self.total, 1), n, self.pitch)

    def utt(self, u):
        return self.spec[self.first[u]:self.first[u] + self.frames[u]]

    def reference(self, eng, cfg):
        """per utterance (int16, float32) of a fresh handle's process + flush, None for an empty one"""
        ref = []
        for u, f in enumerate(self.frames):
            if not f:
                ref.append(None)
                continue
            o, fl, to, tf = run(eng, np.ascontiguousarray(self.utt(u)), **cfg)
            ref.append((np.concatenate([o, to]), np.concatenate([fl, tf])))
        return ref

    def check(self, got_i, got_f, ref, outside_i, outside_f, what):
        """every utterance's span equals its reference, bit for bit; every other sample holds `outside`"""
        covered = np.zeros(self.size, bool)
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
            assert got_i.size == self.size and np.all(got_i[~covered] == outside_i), (what, "int16 outside the spans")
        if got_f is not None:
            assert got_f.size == self.size
            assert np.all(got_f[~covered].view(np.int32) == np.float32(outside_f).view(np.int32)), (what, "float32 outside")


def run_batch(ist, b, fpw=0, d_spec=None):
    """the device path into sentinel-filled outputs -> (int16, float32) as numpy"""
    import torch
    ist.set_option("frames_per_wave", fpw)
    d_spec = torch.from_numpy(b.spec).cuda() if d_spec is None else d_spec
    out = torch.full((max(b.size, 1),), int(SENT_I), dtype=torch.int16, device="cuda")
    f32 = torch.full((max(b.size, 1),), float(SENT_F), dtype=torch.float32, device="cuda")
    o, f = ist.process_batch(d_spec, b.frames, b.offs, want_f32=True, out=out, out_f32=f32)
    torch.cuda.synchronize()
    return o.cpu().numpy(), f.cpu().numpy()


def equal_on_device(eng, b, cfg, fpws, what):
    ref = b.reference(eng, cfg)
    ist = eng.istft(**cfg)
    for fpw in fpws:
        o, f = run_batch(ist, b, fpw)
        b.check(o, f, ref, SENT_I, SENT_F, (what, "frames_per_wave", fpw))
    ist.close()
    return ref


# ---- 1. bit identity over the twelve instantiations ----------------------------------------------------------------
@pytest.mark.parametrize("layout", ["full", "half"])
@pytest.mark.parametrize("n,hop", CONFIGS)
def test_bit_identical_to_single_streams(eng, n, hop, layout):
    R = n // hop
    frames = [1, 0] + ([R - 1] if R > 1 else []) + [R, 2, 0, 0, 9, 1, 1, 37]
    b = Batch(np.random.default_rng(9000 + n + hop + len(layout)), n, hop, layout, frames)
    # 64: one wave walks every utterance; the small values start and end runs inside utterances
    equal_on_device(eng, b, cfg_of(n, hop, layout), sorted({0, max(R - 1, 1), 3, 5, 64}), (n, hop, layout))


# ---- 2. boundary geometry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop", [(1024, 256), (512, 128)])
@pytest.mark.parametrize("frames,fpw", [
    ([4, 4, 4], 4),              # a run starts on an utterance's first frame: no halo, nothing of the one before
    ([5, 5], 3),                 # a run starts one frame into utterance 1: a halo of 1 < R - 1
    ([3, 6, 0, 0, 0], 4),        # the last utterances are empty
    ([0, 0, 5, 4], 3),           # the first are empty
    ([0, 7, 0], 0),
], ids=["run-at-first-frame", "short-halo", "empty-last", "empty-first", "empty-around"])
def test_boundary_geometry(eng, frames, fpw, n, hop):
    for layout in ("full", "half"):
        b = Batch(np.random.default_rng(9100 + len(frames) + fpw + n), n, hop, layout, frames)
        equal_on_device(eng, b, cfg_of(n, hop, layout), [fpw], (frames, layout))


# ---- 3. row pitch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop", [(1024, 512), (512, 128)])
def test_row_pitch(eng, n, hop):
    frames = [3, 0, 1, 6]
    half = Batch(np.random.default_rng(9200 + n), n, hop, "half", frames, pitch=n // 2 + 1 + 3)
    equal_on_device(eng, half, cfg_of(n, hop, "half"), [0, 3], "half, pitch bins + 3")
    full = Batch(np.random.default_rng(9300 + n), n, hop, "full", frames, pitch=n + 8)
    equal_on_device(eng, full, cfg_of(n, hop, "full"), [0, 3], "full, pitch n + 8")


# ---- 4. the FP64 restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop,layout", [(1024, 512, "half"), (512, 128, "full")])
def test_against_restatement(eng, n, hop, layout):
    b = Batch(np.random.default_rng(9400 + n), n, hop, layout, [5, 1, 0, 12])
    ist = eng.istft(**cfg_of(n, hop, layout, "hann", "hann"))
    got_i, got_f = run_batch(ist, b)
    ist.close()
    for u, F in enumerate(b.frames):
        if not F:
            continue
        a, e = int(b.offs[u]), F * hop
        o, f = got_i[a:a + b.spans[u]], got_f[a:a + b.spans[u]]
        check_against_restatement(o[:e], f[:e], o[e:], f[e:], b.utt(u), n, hop, layout, "hann", "hann")


# ---- 5. the handle's own stream ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop,layout", [(1024, 512, "half"), (512, 128, "full")])
def test_handle_stream_is_independent(eng, n, hop, layout):
    import torch
    F, k = 10, 4
    rng = np.random.default_rng(9500 + n)
    cfg = cfg_of(n, hop, layout)
    spec = torch.from_numpy(rows(rng, F, n, n if layout == "full" else n // 2 + 1)).cuda()
    b = Batch(rng, n, hop, layout, [2, 0, 5])
    ref = b.reference(eng, cfg)
    ist = eng.istft(**cfg)

    def stream(with_batch):
        oa, fa = ist.process(spec[:k], want_f32=True)
        oa, fa = oa.clone(), fa.clone()
        if with_batch:
            o, f = run_batch(ist, b)
            b.check(o, f, ref, SENT_I, SENT_F, "between two calls of the handle's stream")
        ob, fb = ist.process(spec[k:], want_f32=True)
        t, tf = ist.flush(want_f32=True)
        torch.cuda.synchronize()
        return torch.cat([oa, ob, t]), fbits(torch.cat([fa, fb, tf]))

    plain, mixed = stream(False), stream(True)
    assert torch.equal(plain[0], mixed[0]) and torch.equal(plain[1], mixed[1])
    ist.close()


# ---- 6. the host entry, NULL outputs, empty batches ----------------------------------------------------------------
def vp(a, off=0):
    if a is None:
        return None
    return C.c_void_p((a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) + off)


@pytest.mark.parametrize("n,hop,layout", [(1024, 256, "half"), (1024, 1024, "full"), (512, 256, "full"), (512, 128, "half")])
def test_host_entry_and_null_outputs(eng, n, hop, layout):
    import torch
    from jeicyboodsp_amd._lib import lib as L
    cfg = cfg_of(n, hop, layout)
    b = Batch(np.random.default_rng(9600 + n + hop), n, hop, layout, [2, 0, 7, 1], pitch=n + 8)
    ref = equal_on_device(eng, b, cfg, [0], "device")
    ist = eng.istft(**cfg)
    # numpy in and out: the same values, zeros outside the spans (the outputs given are overwritten everywhere)
    o, f = ist.process_batch(b.spec, b.frames, b.offs, want_f32=True, out=np.full(b.size, SENT_I),
                             out_f32=np.full(b.size, SENT_F))
    b.check(o, f, ref, 0, 0.0, "host")
    b.check(ist.process_batch(b.spec, b.frames, b.offs), None, ref, 0, 0.0, "host, float32 NULL")
    sample_first, n_utts = np.ascontiguousarray(b.offs[:-1]), len(b.frames)
    f = np.full(b.size, SENT_F)
    assert L.jdsp_istft_batch(ist._h, vp(b.spec), b.pitch, vp(sample_first), vp(b.first), n_utts, b.size, None, vp(f)) == 0
    b.check(None, f, ref, 0, 0.0, "host, int16 NULL")
    assert L.jdsp_istft_batch(ist._h, vp(b.spec), b.pitch, vp(sample_first), vp(b.first), n_utts, b.size, None, None) == 0
    # the device entry with either output NULL
    d_spec = torch.from_numpy(b.spec).cuda()
    d_sample, d_first = torch.from_numpy(sample_first).cuda(), torch.from_numpy(b.first).cuda()
    d_o = torch.full((b.size,), int(SENT_I), dtype=torch.int16, device="cuda")
    d_f = torch.full((b.size,), float(SENT_F), dtype=torch.float32, device="cuda")
    eng._use_torch_stream()
    call = lambda *a: L.jdsp_istft_batch_dev(ist._h, vp(d_spec), b.pitch, vp(d_sample), vp(d_first), *a)  # noqa: E731
    assert call(n_utts, b.total, None, None) == 0
    torch.cuda.synchronize()
    assert torch.all(d_o == int(SENT_I)) and torch.all(d_f == float(SENT_F))       # both NULL: nothing is touched
    assert call(n_utts, b.total, vp(d_o), None) == 0
    assert call(n_utts, b.total, None, vp(d_f)) == 0
    torch.cuda.synchronize()
    b.check(d_o.cpu().numpy(), d_f.cpu().numpy(), ref, SENT_I, SENT_F, "device, one output at a time")
    # nothing to do: no utterances, no frames, only empty utterances
    assert L.jdsp_istft_batch(ist._h, None, b.pitch, None, None, 0, 0, None, None) == 0
    assert call(0, 0, vp(d_o), vp(d_f)) == 0
    assert L.jdsp_istft_batch_dev(ist._h, None, b.pitch, None, None, 0, 0, None, None) == 0
    e = Batch(np.random.default_rng(1), n, hop, layout, [0, 0, 0])
    o, f = ist.process_batch(e.spec, e.frames, e.offs, want_f32=True, out=np.full(e.size, SENT_I),
                             out_f32=np.full(e.size, SENT_F))
    assert o.size == e.size and not o.any() and not f.any()
    o, f = run_batch(ist, e)
    e.check(o, f, [None] * 3, SENT_I, SENT_F, "only empty utterances")
    ist.close()


# ---- 7. errors -----------------------------------------------------------------------------------------------------
def test_errors(eng):
    import torch
    from jeicyboodsp_amd._lib import lib as L
    n, hop, layout = 1024, 512, "half"
    cfg = cfg_of(n, hop, layout)
    b = Batch(np.random.default_rng(9700), n, hop, layout, [2, 3, 1])
    ref = b.reference(eng, cfg)
    ist = eng.istft(**cfg)
    out = np.zeros(b.size, np.int16)
    good_s, good_f, nu = np.ascontiguousarray(b.offs[:-1]), b.first, len(b.frames)

    def host(s=good_s, f=good_f, n_utts=nu, n_samples=b.size, pitch=b.pitch):
        s, f = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(f, np.int64)
        return L.jdsp_istft_batch(ist._h, vp(b.spec), pitch, vp(s), vp(f), n_utts, n_samples, vp(out), None)

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
        "row_pitch below the bins": dict(pitch=512),
        "negative n_utts": dict(n_utts=-1),
        "negative n_samples": dict(n_samples=-1),
    }
    assert host() == 0
    for what, kw in bad.items():
        assert host(**kw) == -1, what
        assert b"jdsp_istft_batch" in L.jdsp_last_error(eng._h), what
    # the device entry: base pointers, counts and pitch -- offsets on the device are the caller's contract
    d_spec = torch.from_numpy(b.spec).cuda()
    d_s, d_f = torch.from_numpy(good_s).cuda(), torch.from_numpy(good_f).cuda()
    d_o = torch.full((b.size + 8,), int(SENT_I), dtype=torch.int16, device="cuda")
    d_f32 = torch.full((b.size + 8,), float(SENT_F), dtype=torch.float32, device="cuda")
    eng._use_torch_stream()

    def dev(spec=vp(d_spec), pitch=b.pitch, s=vp(d_s), f=vp(d_f), n_utts=nu, n_total=b.total, o=vp(d_o), f32=None):
        return L.jdsp_istft_batch_dev(ist._h, spec, pitch, s, f, n_utts, n_total, o, f32)

    for what, kw in {
        "spec not 8-aligned": dict(spec=vp(d_spec, 4)), "row_pitch below the bins": dict(pitch=512),
        "int16 out not 4-aligned": dict(o=vp(d_o, 2)), "float out not 8-aligned": dict(o=None, f32=vp(d_f32, 4)),
        "sample_first not 8-aligned": dict(s=vp(d_s, 4)), "frame_first not 8-aligned": dict(f=vp(d_f, 4)),
        "negative n_utts": dict(n_utts=-1), "negative n_frames_total": dict(n_total=-1),
    }.items():
        assert dev(**kw) == -1, what
        assert b"jdsp_istft_batch" in L.jdsp_last_error(eng._h), what
    torch.cuda.synchronize()
    assert torch.all(d_o == int(SENT_I)) and torch.all(d_f32 == float(SENT_F))      # nothing was launched
    # the handle is still usable, for the batch and for its own stream
    o, f = run_batch(ist, b)
    b.check(o, f, ref, SENT_I, SENT_F, "after the errors")
    o = ist.process(torch.from_numpy(np.ascontiguousarray(b.utt(1))).cuda())
    t = ist.flush()
    torch.cuda.synchronize()
    assert np.array_equal(np.concatenate([o.cpu().numpy(), t.cpu().numpy()]), ref[1][0])
    ist.close()


# ---- 8. simulated ranks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop,layout", [(1024, 256, "half"), (512, 128, "full")])
def test_simulated_ranks(eng, n, hop, layout):
    import torch
    from jeicyboodsp_amd import sharding
    frames = [1, 0, 3, 4, 2, 0, 0, 9, 1, 1, 37]
    b = Batch(np.random.default_rng(9800 + n), n, hop, layout, frames)
    ist = eng.istft(**cfg_of(n, hop, layout))
    d_spec = torch.from_numpy(b.spec).cuda()
    whole = [t.clone() for t in ist.process_batch(d_spec, frames, b.offs, want_f32=True)]
    for world in (1, 2, 3, 8):
        parts, fparts = [], []
        for rank in range(world):
            u0, nu = sharding.stftmask_batch_shard(frames, rank, world)
            lo, hi = int(b.offs[u0]), int(b.offs[u0 + nu])
            r0, r1 = int(b.first[u0]), int(b.first[u0 + nu])
            o, f = ist.process_batch(d_spec[r0:max(r1, r0 + 1)], frames[u0:u0 + nu], b.offs[u0:u0 + nu + 1] - lo,
                                     want_f32=True)
            parts.append(o[:hi - lo].clone())
            fparts.append(f[:hi - lo].clone())
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts), whole[0]), world
        assert torch.equal(fbits(torch.cat(fparts)), fbits(whole[1])), world
    ist.close()


# ---- 9. the round trip through both batched entries ----------------------------------------------------------------
@pytest.mark.parametrize("syn", ["none", "same"])
@pytest.mark.parametrize("hop", [512, 256])
def test_round_trip_through_the_batched_analysis(eng, hop, syn):
    import torch
    n, win = 1024, "hann"
    R = n // hop
    frames = [1, 0, R - 1, R, 2, 9, 37]
    pb = PcmBatch(np.random.default_rng(9900 + hop), hop, frames)
    eng.set_option("stft.window", 1)
    try:
        spec = eng.stft_half_batch(torch.from_numpy(pb.pcm).cuda(), pb.offs, hop=hop, pitch=520)
    finally:
        eng.set_option("stft.window", 0)
    ist = eng.istft(n_fft=n, hop=hop, layout="half", synthesis_window=win if syn == "same" else "none", analysis_window=win)
    o, f = ist.process_batch(spec, frames, pb.offs, want_f32=True)
    torch.cuda.synchronize()
    ist.close()
    o, f = o.cpu().numpy(), f.cpu().numpy()
    checked = 0
    for u, F in enumerate(frames):
        a = int(pb.offs[u])
        lo, hi = n - hop, F * hop                                # the samples every one of their R frames reached
        if F <= R - 1:
            assert hi <= lo                                      # an empty interior: nothing to compare (F = 0, 1, R - 1)
            continue
        want = pb.pcm[a + lo:a + hi]
        assert want.size == hi - lo > 0
        assert np.abs(f[a + lo:a + hi] - want).max() <= 1e-5 * np.abs(pb.utt(u)).max(), u
        assert np.abs(o[a + lo:a + hi].astype(np.int32) - want).max() <= 1, u
        checked += 1
    assert checked == sum(1 for F in frames if F >= R) >= 3       # F = R, 9 and 37 at the least
