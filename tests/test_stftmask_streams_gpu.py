"""Live streams on the fused STFT masking handle (jdsp_stftmask_streams_*, StftMask.open_streams / process_streams /
flush_streams / reset_streams): many output streams in one handle, advanced a ragged chunk each by one launch, with
the overlap-add tails carried from call to call.  Everything is held against the single-stream path -- a fresh
handle's process + flush of all of a stream's frames, which tests/test_stftmask_gpu.py pins to the FP64 restatement --
bit for bit, in int16 and in float32: over hops, mask kinds, launch geometries and cuts into chunks and calls; the
boundary geometries of the carried tail; the handle's own stream and the batch entry interleaved; the FP64 pass; the
host entries; the error paths."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_stftmask_gpu import BINS, HOPS, KINDS, N, cfg_of, mask_of, pcm_of, run, stream_combo  # noqa: E402
from test_stftmask_batch_gpu import Batch, run_batch  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_I = np.int16(-12345)
SENT_F = np.float32(-7777.5)
GAPS = [0, 2, 6]                 # full-scale samples between one chunk's span and the next chunk's
EMPTY = 10                       # full-scale samples where a chunk of no frames stands
N_STREAMS = 6                    # stream 5 is never fed


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def plan_of(R):
    """Four calls of (stream, frames) chunks; the streams total [23, 9, 4, 1, 2 R + 1] frames.  Between them: a chunk
    of 0 frames (stream 1, call 0), chunks of exactly one frame, at R = 4 chunks shorter than R - 1 (2 and 1 frames; at
    R = 2 the one of 0), stream 2 absent from call 1 between two calls that carry it (and stream 4 from call 2), a
    chunk of 11 frames -- longer than three runs at frames_per_wave 3 --, ids out of ascending order and in another
    order in every call."""
    return [[(2, 2), (0, 11), (4, 1), (1, 0)],
            [(1, 5), (4, R), (0, 1), (3, 1)],
            [(0, 3), (2, 1), (1, 1)],
            [(4, R), (1, 3), (2, 1), (0, 8)]]


class Streams:
    """Per stream its whole PCM and mask rows; a call's chunks are cut out of them where the stream stands."""

    def __init__(self, rng, kind, hop, totals, one_row=False, pitch=BINS):
        self.hop, self.kind, self.totals = hop, kind, list(totals)
        self.pcm = [pcm_of(rng, t, hop) if t else np.zeros(0, np.int16) for t in self.totals]
        self.row = mask_of(rng, kind, None, pitch) if one_row else None
        self.mask = [self.row if one_row else mask_of(rng, kind, max(t, 1), pitch) for t in self.totals]
        self.done = [0] * len(self.totals)
        self.got_i = [[] for _ in self.totals]
        self.got_f = [[] for _ in self.totals]

    def rewind(self):
        self.done = [0] * len(self.totals)
        self.got_i = [[] for _ in self.totals]
        self.got_f = [[] for _ in self.totals]

    def reference(self, eng, cfg, first=None):
        """per stream (int16, float32) of a fresh handle's process + flush of all its frames (from frame first[s] on)"""
        ref = []
        for s, t in enumerate(self.totals):
            a = first[s] if first else 0
            if t - a <= 0:
                z = N - self.hop
                ref.append((np.zeros(z, np.int16), np.zeros(z, np.float32)))
                continue
            rows = self.mask[s] if self.row is not None else self.mask[s][a:t]
            o, f, to, tf = run(eng, self.pcm[s][self.hop * a:], rows, t - a, **cfg)
            ref.append((np.concatenate([o, to]), np.concatenate([f, tf])))
        return ref

    def call(self, chunks):
        """The packed buffers of one call: (pcm, mask, ids, counts, sample_first); the gaps and the places of empty
        chunks are full scale, so reading one would show."""
        hop = self.hop
        parts, rows, first, at = [], [], [], 0
        for c, (s, f) in enumerate(chunks):
            at += at & 1
            first.append(at)
            if f:
                a = self.done[s]
                parts.append((at, self.pcm[s][hop * a: hop * (a + f - 1) + N]))
                if self.row is None:
                    rows.append(self.mask[s][a:a + f])
                at += hop * (f - 1) + N
            else:
                at += EMPTY
            at += GAPS[c % 3]
        pcm = np.full(at + (at & 1), 32767, np.int16)
        for a, p in parts:
            pcm[a:a + p.size] = p
        if self.row is not None:
            mask = self.row
        else:
            mask = np.concatenate(rows) if rows else self.mask[0][:1]
        return (pcm, np.ascontiguousarray(mask), np.array([s for s, _ in chunks], np.int64),
                np.array([f for _, f in chunks], np.int64), np.array(first, np.int64))

    def take(self, chunks, first, out_i, out_f, what):
        """a call's outputs to their streams; every sample outside the hop F_c ranges must hold the sentinel"""
        covered = np.zeros(out_i.size, bool)
        for (s, f), a in zip(chunks, first):
            a, b = int(a), int(a) + self.hop * f
            covered[a:b] = True
            self.got_i[s].append(out_i[a:b].copy())
            self.got_f[s].append(out_f[a:b].copy())
            self.done[s] += f
        assert np.all(out_i[~covered] == SENT_I), (what, "int16 outside the written ranges")
        assert np.all(out_f[~covered].view(np.int32) == SENT_F.view(np.int32)), (what, "float32 outside")

    def check(self, flush_i, flush_f, ref, what, streams=None):
        for s in (range(len(self.totals)) if streams is None else streams):
            gi = np.concatenate(self.got_i[s] + [flush_i[s]])
            gf = np.concatenate(self.got_f[s] + [flush_f[s]])
            assert np.array_equal(gi, ref[s][0]), (what, "stream", s, "int16")
            assert np.array_equal(gf.view(np.int32), ref[s][1].view(np.int32)), (what, "stream", s, "float32")


def feed(sm, st, chunks, what=None):
    """one process_streams call on the device path into sentinel-filled outputs, handed to the streams"""
    import torch
    pcm, mask, ids, counts, first = st.call(chunks)
    out = torch.full((pcm.size,), int(SENT_I), dtype=torch.int16, device="cuda")
    f32 = torch.full((pcm.size,), float(SENT_F), dtype=torch.float32, device="cuda")
    o, f = sm.process_streams(torch.from_numpy(pcm).cuda(), torch.from_numpy(mask).cuda(), ids, counts, first,
                              want_f32=True, out=out, out_f32=f32)
    torch.cuda.synchronize()
    st.take(chunks, first, o.cpu().numpy(), f.cpu().numpy(), what)


def flush_all(sm, n):
    import torch
    fi, ff = sm.flush_streams(np.arange(n), want_f32=True)
    if isinstance(fi, np.ndarray):                                 # no device call since open_streams: the host entry
        return fi, ff
    torch.cuda.synchronize()
    return fi.cpu().numpy(), ff.cpu().numpy()


# ---- 1. bit identity over cuts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", HOPS)
def test_bit_identical_over_cuts(eng, hop, kind):
    R = N // hop
    cfg = cfg_of(hop, kind, stream_combo(hop))
    st = Streams(np.random.default_rng(9000 + hop + len(kind)), kind, hop, [23, 9, 4, 1, 2 * R + 1, 0])
    plan = plan_of(R)
    assert [sum(f for c in plan for s, f in c if s == k) for k in range(N_STREAMS)] == st.totals
    ref = st.reference(eng, cfg)
    sm = eng.stft_mask(**cfg)
    sm.open_streams(N_STREAMS)
    for fpw in sorted({0, max(R - 1, 1), 3, 5, 64}):
        sm.set_option("frames_per_wave", fpw)
        st.rewind()
        for k, chunks in enumerate(plan):
            feed(sm, st, chunks, (hop, kind, fpw, "call", k))
        fi, ff = flush_all(sm, N_STREAMS)                          # the flush leaves every stream fresh for the next fpw
        st.check(fi, ff, ref, (hop, kind, "frames_per_wave", fpw))
        assert not fi[5].any() and not ff[5].view(np.int32).any(), "a stream never fed flushes to exact zeros"
    sm.close()


# ---- 2. boundary geometry of the carried tail (hop 256, R = 4) -----------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("frames,fpw", [
    ([4, 4, 4], 4),              # a run starts on a chunk's first frame: that wave loads the tail and has no halo
    ([5, 5], 3),                 # a run starts one frame into chunk 1: a halo of 1 < R - 1, so the tail is loaded by a
                                 # wave that does not own the chunk's first frame
    ([3, 3, 2], 4),              # chunk 1 (frames 3..5) is shorter than a run and its first and last frames belong to
                                 # different waves: the reader of its tail is not the writer
    ([0, 0, 5, 4, 0, 0], 3),     # the first and the last chunks are empty
], ids=["run-at-first-frame", "short-halo", "reader-is-not-writer", "empty-first-last"])
def test_boundary_geometry(eng, frames, fpw, kind):
    hop = 256
    cfg = cfg_of(hop, kind, stream_combo(hop))
    lead = 2                                                       # frames fed first, so the tails carried in are not zero
    st = Streams(np.random.default_rng(9100 + len(frames) + fpw), kind, hop, [lead + f for f in frames])
    ref = st.reference(eng, cfg)
    sm = eng.stft_mask(**cfg)
    sm.open_streams(len(frames))
    feed(sm, st, [(s, lead) for s in range(len(frames))], "lead")
    sm.set_option("frames_per_wave", fpw)
    feed(sm, st, list(enumerate(frames)), (frames, fpw))
    fi, ff = flush_all(sm, len(frames))
    st.check(fi, ff, ref, (frames, fpw))
    sm.close()


# ---- 3. independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_interleaved_with_own_stream_and_batch(eng, kind):
    import torch
    hop = 256
    cfg = cfg_of(hop, kind, stream_combo(hop))
    rng = np.random.default_rng(9200 + len(kind))
    st = Streams(rng, kind, hop, [7, 5, 6])
    ref = st.reference(eng, cfg)
    F = 9                                                          # the handle's own stream, in two calls
    own_pcm, own_mask = pcm_of(rng, F, hop), mask_of(rng, kind, F)
    o, f, to, tf = run(eng, own_pcm, own_mask, F, **cfg)
    b = Batch(rng, kind, hop, [3, 0, 5])
    bref = b.reference(eng, cfg)

    sm = eng.stft_mask(**cfg)
    sm.open_streams(3)
    d_pcm, d_mask = torch.from_numpy(own_pcm).cuda(), torch.from_numpy(own_mask).cuda()
    feed(sm, st, [(1, 2), (0, 4), (2, 1)], "call 0")
    o1, f1 = sm.process(d_pcm[:hop * 3 + N], d_mask[:4], 4, want_f32=True)
    feed(sm, st, [(2, 5), (0, 0)], "call 1")
    bo, bf = run_batch(sm, b)
    o2, f2 = sm.process(d_pcm[hop * 4:], d_mask[4:], F - 4, want_f32=True)
    feed(sm, st, [(0, 3), (1, 3)], "call 2")
    t2, tf2 = sm.flush(want_f32=True)
    fi, ff = flush_all(sm, 3)
    st.check(fi, ff, ref, "live streams")
    b.check(bo, bf, bref, SENT_I, SENT_F, "batch")
    assert np.array_equal(torch.cat([o1, o2, t2]).cpu().numpy(), np.concatenate([o, to])), "own stream int16"
    assert np.array_equal(torch.cat([f1, f2, tf2]).cpu().numpy().view(np.int32),
                          np.concatenate([f, tf]).view(np.int32)), "own stream float32"
    sm.close()


def test_reset_and_reserve_again(eng):
    hop, kind = 512, "real"
    cfg = cfg_of(hop, kind, stream_combo(hop))
    st = Streams(np.random.default_rng(9300), kind, hop, [5, 5, 5, 5, 5])
    whole = st.reference(eng, cfg)
    late = st.reference(eng, cfg, first=[3] * 5)                   # a fresh stream given frames 3 and 4 only
    sm = eng.stft_mask(**cfg)
    sm.open_streams(5)
    feed(sm, st, [(s, 3) for s in range(5)], "before the reset")
    sm.reset_streams([1, 3])
    for s in (1, 3):
        st.got_i[s], st.got_f[s] = [], []
    feed(sm, st, [(s, 2) for s in (4, 3, 2, 1, 0)], "after the reset")
    fi, ff = flush_all(sm, 5)
    st.check(fi, ff, whole, "streams 0, 2, 4 are as they were", streams=(0, 2, 4))
    st.check(fi, ff, late, "streams 1, 3 started again", streams=(1, 3))
    # reserve again: every stream fresh
    st.rewind()
    feed(sm, st, [(s, 3) for s in range(5)], "before the second reserve")
    sm.open_streams(5)
    fi, ff = flush_all(sm, 5)
    assert not fi.any() and not ff.view(np.int32).any()
    # ... and all of them at once
    feed(sm, st, [(s, 2) for s in range(5)], "before the reset of all")
    sm.reset_streams()
    fi, ff = flush_all(sm, 5)
    assert not fi.any() and not ff.view(np.int32).any()
    sm.close()


# ---- 4. the FP64 pass travels --------------------------------------------------------------------------------------
def test_fp64_pass_travels(eng):
    import torch
    import stftmask_fp32_ref as S
    c = S.cases()[S.index_of("notch_on_60dB-256-complex")]
    assert (S.criterion(c) > S.RHO).any(), "the plain-FP32 restatement must put a frame of this case over RHO"
    hop, kind, F = c["hop"], c["kind"], c["F"]
    cfg = cfg_of(hop, kind, c["combo"])
    one = eng.stft_mask(**cfg)
    c_pcm, c_mask = np.array(c["pcm"]), np.array(c["mask"])        # writable copies: the cases are shared, read-only
    o, f = one.process(torch.from_numpy(c_pcm).cuda(), torch.from_numpy(c_mask).cuda(), F, want_f32=True)
    n_one = one.frames_recomputed()
    to, tf = one.flush(want_f32=True)
    torch.cuda.synchronize()
    ref = (np.concatenate([o.cpu().numpy(), to.cpu().numpy()]), np.concatenate([f.cpu().numpy(), tf.cpu().numpy()]))
    one.close()
    st = Streams(np.random.default_rng(9400), kind, hop, [3, F])
    st.pcm[1], st.mask[1] = c_pcm, c_mask
    sm = eng.stft_mask(**cfg)
    sm.open_streams(2)
    counts = []
    for k, n in enumerate((1, 20, F - 21)):
        feed(sm, st, [(1, n)], ("cut", k))
        counts.append(sm.frames_recomputed())
    fi, ff = flush_all(sm, 2)
    st.check(fi, ff, [None, ref], "suppressing case", streams=(1,))
    print("frames recomputed: single stream %d, three calls %s" % (n_one, counts))
    assert n_one > 0 and sum(counts) == n_one
    sm.close()


def test_a_call_of_nothing_recomputed_no_frames(eng):
    """jdsp_stftmask_frames_recomputed answers for the LAST call: after a call that recomputed frames, every batch or
    streams call that has nothing to do -- no spans, no frames, no output to write, on the device entries; counts that
    are all zero on the host entries -- leaves the count at 0, not at the earlier call's figure."""
    import torch
    import stftmask_fp32_ref as S
    c = min((c for c in S.cases() if c["name"].startswith("notch")), key=lambda c: c["pcm"].size)
    hop, F = c["hop"], c["F"]
    pcm, mask = np.array(c["pcm"]), np.array(c["mask"])
    pitch = mask.shape[1]
    sm = eng.stft_mask(**cfg_of(hop, c["kind"], c["combo"]))
    sm.open_streams(2)
    d_pcm, d_mask = torch.from_numpy(pcm).cuda(), torch.from_numpy(mask).cuda()
    ids, first = np.array([1], np.int64), np.array([0], np.int64)
    ff, ff0 = np.array([0, F], np.int64), np.array([0, 0], np.int64)
    d_ids, d_first, d_ff = (torch.from_numpy(a).cuda() for a in (ids, first, ff))
    d_out = torch.zeros(pcm.size, dtype=torch.int16, device="cuda")
    h_out = np.zeros(pcm.size, np.int16)
    vp = lambda a: None if a is None else C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731

    def batch_dev(n, total, out):
        return sm._c("_batch_dev")(sm._h, vp(d_pcm), vp(d_mask), pitch, vp(d_first), vp(d_ff), n, total, vp(out), None)

    def streams_dev(n, total, out):
        return sm._c("_streams_dev")(sm._h, vp(d_pcm), vp(d_mask), pitch, vp(d_ids), vp(d_first), vp(d_ff), n, total,
                                     vp(out), None)

    nothing = [
        ("batch_dev, n_utts 0", lambda: batch_dev(0, F, d_out)),
        ("streams_dev, n_chunks 0", lambda: streams_dev(0, F, d_out)),
        ("batch_dev, n_frames_total 0", lambda: batch_dev(1, 0, d_out)),
        ("streams_dev, n_frames_total 0", lambda: streams_dev(1, 0, d_out)),
        ("batch_dev, both outputs NULL", lambda: batch_dev(1, F, None)),
        ("streams_dev, both outputs NULL", lambda: streams_dev(1, F, None)),
        ("host batch, all counts 0", lambda: sm._c("_batch")(sm._h, vp(pcm), pcm.size, vp(mask), pitch, vp(first), vp(ff0), 1,
                                                             vp(h_out), None)),
        ("host streams, all counts 0", lambda: sm._c("_streams")(sm._h, vp(pcm), pcm.size, vp(mask), pitch, vp(ids), vp(first),
                                                                 vp(ff0), 1, vp(h_out), None)),
    ]
    for what, call in nothing:
        sm.reset()
        sm.process(d_pcm, d_mask, F)
        n = sm.frames_recomputed()
        print("%s: %d frames recomputed before it" % (what, n))
        assert n > 0, "the notched tone must recompute frames"
        assert call() == 0, what
        after = sm.frames_recomputed()
        print("%s: %d after it" % (what, after))
        assert after == 0, what
    sm.close()


# ---- 5. the host entries -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_host_entries(eng, kind):
    hop = 256
    R = N // hop
    cfg = cfg_of(hop, kind, stream_combo(hop))
    st = Streams(np.random.default_rng(9500 + len(kind)), kind, hop, [23, 9, 4, 1, 2 * R + 1, 0])
    ref = st.reference(eng, cfg)
    sm = eng.stft_mask(**cfg)
    sm.open_streams(N_STREAMS)
    for k, chunks in enumerate(plan_of(R)):
        pcm, mask, ids, counts, first = st.call(chunks)
        if k == 1:                                                 # NULL outputs advance nothing
            rc = sm._c("_streams")(sm._h, pcm.ctypes.data_as(C.c_void_p), pcm.size, mask.ctypes.data_as(C.c_void_p), BINS,
                                   ids.ctypes.data_as(C.c_void_p), first.ctypes.data_as(C.c_void_p),
                                   np.concatenate([[0], np.cumsum(counts)]).astype(np.int64).ctypes.data_as(C.c_void_p),
                                   ids.size, None, None)
            assert rc == 0
        o, f = sm.process_streams(pcm, mask, ids, counts, first, want_f32=True)
        covered = np.zeros(pcm.size, bool)
        for (s, n), a in zip(chunks, first):
            covered[int(a):int(a) + hop * n] = True
        assert not o[~covered].any() and not f[~covered].view(np.int32).any(), "zero outside the written ranges"
        o, f = o.copy(), f.copy()
        o[~covered], f[~covered] = SENT_I, SENT_F
        st.take(chunks, first, o, f, ("host call", k))
    fi, ff = sm.flush_streams(np.arange(N_STREAMS), want_f32=True)
    assert isinstance(fi, np.ndarray)
    st.check(fi, ff, ref, "host entries")
    sm.close()


# ---- 6. errors -----------------------------------------------------------------------------------------------------
def test_errors(eng):
    import torch
    from jeicyboodsp_amd._lib import JdspError
    hop, kind = 256, "real"
    cfg = cfg_of(hop, kind, stream_combo(hop))
    st = Streams(np.random.default_rng(9600), kind, hop, [6, 6, 6])
    ref = st.reference(eng, cfg)
    sm = eng.stft_mask(**cfg)
    vp = lambda a: None if a is None else C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731

    pcm, mask, ids, counts, first = st.call([(0, 3), (1, 3), (2, 3)])
    ff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    d = {k: torch.from_numpy(v).cuda() for k, v in dict(pcm=pcm, mask=mask, ids=ids, first=first, ff=ff).items()}
    out = torch.zeros(pcm.size + 8, dtype=torch.int16, device="cuda")
    f32 = torch.zeros(pcm.size + 8, dtype=torch.float32, device="cuda")

    def dev(pcm_=None, mask_=None, pitch=BINS, ids_=None, first_=None, ff_=None, n=3, total=9, out_=None, f32_=None):
        g = lambda v, k: vp(d[k]) if v is None else v              # noqa: E731
        return sm._c("_streams_dev")(sm._h, g(pcm_, "pcm"), g(mask_, "mask"), pitch, g(ids_, "ids"), g(first_, "first"),
                                     g(ff_, "ff"), n, total, vp(out) if out_ is None else out_,
                                     vp(f32) if f32_ is None else f32_)

    def host(ids_=ids, first_=first, ff_=ff, n=3, pitch=BINS, n_samples=None):
        o = np.zeros(pcm.size, np.int16)
        return sm._c("_streams")(sm._h, vp(pcm), pcm.size if n_samples is None else n_samples, vp(mask), pitch,
                                 vp(np.ascontiguousarray(ids_, np.int64)), vp(np.ascontiguousarray(first_, np.int64)),
                                 vp(np.ascontiguousarray(ff_, np.int64)), n, vp(o), None)

    def text():
        from jeicyboodsp_amd._lib import lib
        return lib.jdsp_last_error(eng._h).decode()

    # before reserve: every entry
    eng._use_torch_stream()
    for rc in (dev(), host(), sm._c("_streams_reset_dev")(sm._h, None, 0),
               sm._c("_streams_flush_dev")(sm._h, vp(d["ids"]), vp(d["first"]), 3, vp(out), None),
               sm._c("_streams_flush")(sm._h, vp(ids), vp(first), 3, pcm.size, vp(np.zeros(pcm.size, np.int16)), None)):
        assert rc == -1 and "reserve" in text(), (rc, text())
    with pytest.raises(JdspError):
        sm.open_streams(0)
    sm.open_streams(3)
    feed(sm, st, [(0, 3), (1, 3), (2, 3)], "valid")

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    bad = [
        ("n_chunks > n_streams", lambda: dev(n=4)),
        ("n_chunks < 0", lambda: dev(n=-1)),
        ("n_frames_total < 0", lambda: dev(total=-1)),
        ("pcm misaligned", lambda: dev(pcm_=off(d["pcm"], 2))),
        ("mask misaligned", lambda: dev(mask_=off(d["mask"], 2))),
        ("ids misaligned", lambda: dev(ids_=off(d["ids"], 4))),
        ("sample_first misaligned", lambda: dev(first_=off(d["first"], 4))),
        ("frame_first misaligned", lambda: dev(ff_=off(d["ff"], 4))),
        ("out_i16 misaligned", lambda: dev(out_=off(out, 2))),
        ("out_f32 misaligned", lambda: dev(f32_=off(f32, 4))),
        ("mask_pitch 1", lambda: dev(pitch=1)),
        ("mask_pitch n/2", lambda: dev(pitch=N // 2)),
        ("host mask_pitch n/2", lambda: host(pitch=N // 2)),
        ("host n_chunks > n_streams", lambda: host(ids_=[0, 1, 2, 2], first_=list(first) + [0], ff_=list(ff) + [9], n=4)),
        ("host n_chunks < 0", lambda: host(n=-1)),
        ("host n_samples < 0", lambda: host(n_samples=-1)),
        ("host id out of range", lambda: host(ids_=[0, 3, 2])),
        ("host id negative", lambda: host(ids_=[0, -1, 2])),
        ("host duplicate id", lambda: host(ids_=[0, 2, 2])),
        ("host frame_first[0] != 0", lambda: host(ff_=[1, 3, 6, 9])),
        ("host decreasing frame_first", lambda: host(ff_=[0, 6, 3, 9])),
        ("host odd sample_first", lambda: host(first_=[first[0], first[1] + 1, first[2]])),
        ("host overlapping spans", lambda: host(first_=[first[0], first[1] - 2, first[2]])),
        ("host span past n_samples", lambda: host(n_samples=pcm.size - 8)),
        ("flush ids misaligned", lambda: sm._c("_streams_flush_dev")(sm._h, off(d["ids"], 4), vp(d["first"]), 2, vp(out), None)),
        ("flush n_ids > n_streams", lambda: sm._c("_streams_flush_dev")(sm._h, vp(d["ids"]), vp(d["first"]), 4, vp(out), None)),
        ("flush n_ids < 0", lambda: sm._c("_streams_flush_dev")(sm._h, vp(d["ids"]), vp(d["first"]), -1, vp(out), None)),
        ("reset ids misaligned", lambda: sm._c("_streams_reset_dev")(sm._h, off(d["ids"], 4), 2)),
        ("host flush duplicate id", lambda: sm._c("_streams_flush")(
            sm._h, vp(np.array([1, 1], np.int64)), vp(np.array([0, 1024], np.int64)), 2, 4096,
            vp(np.zeros(4096, np.int16)), None)),
        ("host flush id out of range", lambda: sm._c("_streams_flush")(
            sm._h, vp(np.array([1, 3], np.int64)), vp(np.array([0, 1024], np.int64)), 2, 4096,
            vp(np.zeros(4096, np.int16)), None)),
        ("host flush overlapping", lambda: sm._c("_streams_flush")(
            sm._h, vp(np.array([1, 2], np.int64)), vp(np.array([0, 700], np.int64)), 2, 4096,
            vp(np.zeros(4096, np.int16)), None)),
    ]
    for what, call in bad:
        rc = call()
        assert rc == -1 and text(), (what, rc)
    # NULL outputs, no chunks, no frames: nothing launched, nothing advanced
    assert dev(out_=C.c_void_p(None), f32_=C.c_void_p(None)) == 0
    assert dev(n=0, total=0) == 0
    # every stream is as the valid call left it
    feed(sm, st, [(2, 3), (0, 3), (1, 3)], "valid again")
    fi, ffl = flush_all(sm, 3)
    st.check(fi, ffl, ref, "after the rejected calls")
    sm.close()
