"""Live streams on the STFT synthesis handle (jdsp_istft_streams_*, Istft.open_streams / process_streams /
flush_streams / reset_streams): many output streams in one handle, advanced a ragged chunk of spectrum rows each by one
launch, with the overlap-add tails carried from call to call.  Everything is held against the single-stream path -- a
fresh handle's process + flush of all of a stream's rows, which tests/test_istft_gpu.py pins to the FP64 restatement --
bit for bit, in int16 and in float32: over all twelve (n, hop, layout) configurations, launch geometries and cuts into
chunks and calls; the boundary geometries of the carried tail; the handle's own stream and the batch entry interleaved;
the host entries; the error paths."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_istft_gpu import CONFIGS, rows, run  # noqa: E402
from test_istft_batch_gpu import Batch, cfg_of, run_batch  # noqa: E402
from test_stftmask_streams_gpu import EMPTY, GAPS, N_STREAMS, SENT_F, SENT_I, flush_all, plan_of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


class Streams:
    """Per stream all its spectrum rows; a call's chunks are cut out of them where the stream stands."""

    def __init__(self, rng, n, hop, layout, totals, pitch=None):
        self.n, self.hop, self.totals = n, hop, list(totals)
        self.bins = n // 2 + 1 if layout == "half" else n
        self.pitch = pitch or self.bins
        self.spec = [rows(rng, max(t, 1), n, self.pitch) for t in self.totals]
        self.rewind()

    def rewind(self):
        self.done = [0] * len(self.totals)
        self.got_i = [[] for _ in self.totals]
        self.got_f = [[] for _ in self.totals]

    def reference(self, eng, cfg, first=None):
        """per stream (int16, float32) of a fresh handle's process + flush of all its rows (from row first[s] on)"""
        ref = []
        for s, t in enumerate(self.totals):
            a = first[s] if first else 0
            if t - a <= 0:
                z = self.n - self.hop
                ref.append((np.zeros(z, np.int16), np.zeros(z, np.float32)))
                continue
            o, f, to, tf = run(eng, np.ascontiguousarray(self.spec[s][a:t]), **cfg)
            ref.append((np.concatenate([o, to]), np.concatenate([f, tf])))
        return ref

    def call(self, chunks):
        """One call: (spec rows, ids, counts, sample_first, n_samples); the output spans are packed with the gaps GAPS
        (in turn) behind them, and a chunk of no rows still owns EMPTY samples, which nothing may write."""
        parts, first, at = [], [], 0
        for c, (s, f) in enumerate(chunks):
            first.append(at)
            if f:
                parts.append(self.spec[s][self.done[s]:self.done[s] + f])
            at += (self.hop * f if f else EMPTY) + GAPS[c % 3]
        spec = np.concatenate(parts) if parts else self.spec[0][:1]
        return (np.ascontiguousarray(spec), np.array([s for s, _ in chunks], np.int64),
                np.array([f for _, f in chunks], np.int64), np.array(first, np.int64), at)

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


def feed(ist, st, chunks, what=None):
    """one process_streams call on the device path into sentinel-filled outputs, handed to the streams"""
    import torch
    spec, ids, counts, first, size = st.call(chunks)
    out = torch.full((size,), int(SENT_I), dtype=torch.int16, device="cuda")
    f32 = torch.full((size,), float(SENT_F), dtype=torch.float32, device="cuda")
    o, f = ist.process_streams(torch.from_numpy(spec).cuda(), ids, counts, first, n_samples=size, want_f32=True, out=out,
                               out_f32=f32)
    torch.cuda.synchronize()
    st.take(chunks, first, o.cpu().numpy(), f.cpu().numpy(), what)


# ---- 1. bit identity over cuts, all twelve instantiations ----------------------------------------------------------
@pytest.mark.parametrize("layout", ["full", "half"])
@pytest.mark.parametrize("n,hop", CONFIGS)
def test_bit_identical_over_cuts(eng, n, hop, layout):
    R = n // hop
    cfg = cfg_of(n, hop, layout)
    st = Streams(np.random.default_rng(9700 + n + hop + len(layout)), n, hop, layout, [23, 9, 4, 1, 2 * R + 1, 0])
    plan = plan_of(R)
    assert [sum(f for c in plan for s, f in c if s == k) for k in range(N_STREAMS)] == st.totals
    ref = st.reference(eng, cfg)
    ist = eng.istft(**cfg)
    ist.open_streams(N_STREAMS)
    for fpw in sorted({0, max(R - 1, 1), 3, 5, 64}):
        ist.set_option("frames_per_wave", fpw)
        st.rewind()
        for k, chunks in enumerate(plan):
            feed(ist, st, chunks, (n, hop, layout, fpw, "call", k))
        fi, ff = flush_all(ist, N_STREAMS)                         # the flush leaves every stream fresh for the next fpw
        st.check(fi, ff, ref, (n, hop, layout, "frames_per_wave", fpw))
        assert not fi[5].any() and not ff[5].view(np.int32).any(), "a stream never fed flushes to exact zeros"
    ist.close()


# ---- 2. boundary geometry of the carried tail (R = 4) --------------------------------------------------------------
@pytest.mark.parametrize("n,hop", [(1024, 256), (512, 128)])
@pytest.mark.parametrize("frames,fpw", [
    ([4, 4, 4], 4),              # a run starts on a chunk's first frame: that wave loads the tail and has no halo
    ([5, 5], 3),                 # a run starts one frame into chunk 1: a halo of 1 < R - 1, so the tail is loaded by a
                                 # wave that does not own the chunk's first frame
    ([3, 3, 2], 4),              # chunk 1 (frames 3..5) is shorter than a run and its first and last frames belong to
                                 # different waves: the reader of its tail is not the writer
    ([0, 0, 5, 4, 0, 0], 3),     # the first and the last chunks are empty
], ids=["run-at-first-frame", "short-halo", "reader-is-not-writer", "empty-first-last"])
def test_boundary_geometry(eng, frames, fpw, n, hop):
    lead = 2                                                       # rows fed first, so the tails carried in are not zero
    for layout in ("full", "half"):
        cfg = cfg_of(n, hop, layout)
        st = Streams(np.random.default_rng(9800 + len(frames) + fpw + n), n, hop, layout, [lead + f for f in frames])
        ref = st.reference(eng, cfg)
        ist = eng.istft(**cfg)
        ist.open_streams(len(frames))
        feed(ist, st, [(s, lead) for s in range(len(frames))], "lead")
        ist.set_option("frames_per_wave", fpw)
        feed(ist, st, list(enumerate(frames)), (frames, fpw, layout))
        fi, ff = flush_all(ist, len(frames))
        st.check(fi, ff, ref, (frames, fpw, layout))
        ist.close()


# ---- 3. independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop,layout", [(1024, 256, "half"), (512, 256, "full")])
def test_interleaved_with_own_stream_and_batch(eng, n, hop, layout):
    import torch
    cfg = cfg_of(n, hop, layout)
    rng = np.random.default_rng(9900 + n)
    st = Streams(rng, n, hop, layout, [7, 5, 6])
    ref = st.reference(eng, cfg)
    F = 9                                                          # the handle's own stream, in two calls
    own = rows(rng, F, n, st.bins)
    o, f, to, tf = run(eng, own, **cfg)
    b = Batch(rng, n, hop, layout, [3, 0, 5])
    bref = b.reference(eng, cfg)

    ist = eng.istft(**cfg)
    ist.open_streams(3)
    d_own = torch.from_numpy(own).cuda()
    feed(ist, st, [(1, 2), (0, 4), (2, 1)], "call 0")
    o1, f1 = ist.process(d_own[:4], want_f32=True)
    feed(ist, st, [(2, 5), (0, 0)], "call 1")
    bo, bf = run_batch(ist, b)
    o2, f2 = ist.process(d_own[4:], want_f32=True)
    feed(ist, st, [(0, 3), (1, 3)], "call 2")
    t2, tf2 = ist.flush(want_f32=True)
    fi, ff = flush_all(ist, 3)
    st.check(fi, ff, ref, "live streams")
    b.check(bo, bf, bref, SENT_I, SENT_F, "batch")
    assert np.array_equal(torch.cat([o1, o2, t2]).cpu().numpy(), np.concatenate([o, to])), "own stream int16"
    assert np.array_equal(torch.cat([f1, f2, tf2]).cpu().numpy().view(np.int32),
                          np.concatenate([f, tf]).view(np.int32)), "own stream float32"
    ist.close()


def test_reset_and_reserve_again(eng):
    n, hop, layout = 1024, 512, "half"
    cfg = cfg_of(n, hop, layout)
    st = Streams(np.random.default_rng(9950), n, hop, layout, [5, 5, 5, 5, 5])
    whole = st.reference(eng, cfg)
    late = st.reference(eng, cfg, first=[3] * 5)                   # a fresh stream given rows 3 and 4 only
    ist = eng.istft(**cfg)
    ist.open_streams(5)
    feed(ist, st, [(s, 3) for s in range(5)], "before the reset")
    ist.reset_streams([1, 3])
    for s in (1, 3):
        st.got_i[s], st.got_f[s] = [], []
    feed(ist, st, [(s, 2) for s in (4, 3, 2, 1, 0)], "after the reset")
    fi, ff = flush_all(ist, 5)
    st.check(fi, ff, whole, "streams 0, 2, 4 are as they were", streams=(0, 2, 4))
    st.check(fi, ff, late, "streams 1, 3 started again", streams=(1, 3))
    st.rewind()
    feed(ist, st, [(s, 3) for s in range(5)], "before the second reserve")
    ist.open_streams(5)                                            # reserve again: every stream fresh
    fi, ff = flush_all(ist, 5)
    assert not fi.any() and not ff.view(np.int32).any()
    feed(ist, st, [(s, 2) for s in range(5)], "before the reset of all")
    ist.reset_streams()
    fi, ff = flush_all(ist, 5)
    assert not fi.any() and not ff.view(np.int32).any()
    ist.close()


# ---- 5. the host entries -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop,layout", [(1024, 256, "full"), (512, 128, "half")])
def test_host_entries(eng, n, hop, layout):
    R = n // hop
    cfg = cfg_of(n, hop, layout)
    st = Streams(np.random.default_rng(9960 + n), n, hop, layout, [23, 9, 4, 1, 2 * R + 1, 0])
    ref = st.reference(eng, cfg)
    ist = eng.istft(**cfg)
    ist.open_streams(N_STREAMS)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
    for k, chunks in enumerate(plan_of(R)):
        spec, ids, counts, first, size = st.call(chunks)
        if k == 1:                                                 # NULL outputs advance nothing
            ff_ = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            assert ist._c("_streams")(ist._h, vp(spec), st.pitch, vp(ids), vp(first), vp(ff_), ids.size, size, None, None) == 0
        o, f = ist.process_streams(spec, ids, counts, first, n_samples=size, want_f32=True)
        covered = np.zeros(size, bool)
        for (s, m), a in zip(chunks, first):
            covered[int(a):int(a) + hop * m] = True
        assert not o[~covered].any() and not f[~covered].view(np.int32).any(), "zero outside the written ranges"
        o, f = o.copy(), f.copy()
        o[~covered], f[~covered] = SENT_I, SENT_F
        st.take(chunks, first, o, f, ("host call", k))
    fi, ff = ist.flush_streams(np.arange(N_STREAMS), want_f32=True)
    assert isinstance(fi, np.ndarray)
    st.check(fi, ff, ref, "host entries")
    ist.close()


# ---- 6. errors -----------------------------------------------------------------------------------------------------
def test_errors(eng):
    import torch
    from jeicyboodsp_amd._lib import JdspError, lib
    n, hop, layout = 1024, 256, "half"
    cfg = cfg_of(n, hop, layout)
    st = Streams(np.random.default_rng(9970), n, hop, layout, [6, 6, 6])
    ref = st.reference(eng, cfg)
    ist = eng.istft(**cfg)
    vp = lambda a: None if a is None else C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731
    text = lambda: lib.jdsp_last_error(eng._h).decode()            # noqa: E731

    spec, ids, counts, first, size = st.call([(0, 3), (1, 3), (2, 3)])
    ff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    d = {k: torch.from_numpy(v).cuda() for k, v in dict(spec=spec, ids=ids, first=first, ff=ff).items()}
    out = torch.zeros(size + 8, dtype=torch.int16, device="cuda")
    f32 = torch.zeros(size + 8, dtype=torch.float32, device="cuda")

    def dev(spec_=None, pitch=st.pitch, ids_=None, first_=None, ff_=None, n_=3, total=9, out_=None, f32_=None):
        g = lambda v, k: vp(d[k]) if v is None else v              # noqa: E731
        return ist._c("_streams_dev")(ist._h, g(spec_, "spec"), pitch, g(ids_, "ids"), g(first_, "first"), g(ff_, "ff"),
                                      n_, total, vp(out) if out_ is None else out_, vp(f32) if f32_ is None else f32_)

    def host(ids_=ids, first_=first, ff_=ff, n_=3, pitch=st.pitch, n_samples=size):
        o = np.zeros(size, np.int16)
        return ist._c("_streams")(ist._h, vp(spec), pitch, vp(np.ascontiguousarray(ids_, np.int64)),
                                  vp(np.ascontiguousarray(first_, np.int64)), vp(np.ascontiguousarray(ff_, np.int64)),
                                  n_, n_samples, vp(o), None)

    z = np.zeros(4096, np.int16)
    eng._use_torch_stream()
    for rc in (dev(), host(), ist._c("_streams_reset_dev")(ist._h, None, 0),
               ist._c("_streams_flush_dev")(ist._h, vp(d["ids"]), vp(d["first"]), 3, vp(out), None),
               ist._c("_streams_flush")(ist._h, vp(ids), vp(first), 3, size, vp(np.zeros(size, np.int16)), None)):
        assert rc == -1 and "reserve" in text(), (rc, text())
    with pytest.raises(JdspError):
        ist.open_streams(0)
    ist.open_streams(3)
    feed(ist, st, [(0, 3), (1, 3), (2, 3)], "valid")

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    bad = [
        ("n_chunks > n_streams", lambda: dev(n_=4)),
        ("n_chunks < 0", lambda: dev(n_=-1)),
        ("n_frames_total < 0", lambda: dev(total=-1)),
        ("row_pitch below the bins", lambda: dev(pitch=st.bins - 1)),
        ("spec misaligned", lambda: dev(spec_=off(d["spec"], 4))),
        ("ids misaligned", lambda: dev(ids_=off(d["ids"], 4))),
        ("sample_first misaligned", lambda: dev(first_=off(d["first"], 4))),
        ("frame_first misaligned", lambda: dev(ff_=off(d["ff"], 4))),
        ("out_i16 misaligned", lambda: dev(out_=off(out, 2))),
        ("out_f32 misaligned", lambda: dev(f32_=off(f32, 4))),
        ("host row_pitch below the bins", lambda: host(pitch=st.bins - 1)),
        ("host n_chunks > n_streams", lambda: host(ids_=[0, 1, 2, 2], first_=list(first) + [0], ff_=list(ff) + [9], n_=4)),
        ("host n_chunks < 0", lambda: host(n_=-1)),
        ("host n_samples < 0", lambda: host(n_samples=-1)),
        ("host id out of range", lambda: host(ids_=[0, 3, 2])),
        ("host id negative", lambda: host(ids_=[0, -1, 2])),
        ("host duplicate id", lambda: host(ids_=[0, 2, 2])),
        ("host frame_first[0] != 0", lambda: host(ff_=[1, 3, 6, 9])),
        ("host decreasing frame_first", lambda: host(ff_=[0, 6, 3, 9])),
        ("host odd sample_first", lambda: host(first_=[first[0], first[1] + 1, first[2]])),
        ("host overlapping spans", lambda: host(first_=[first[0], first[1] - 2, first[2]])),
        ("host span past n_samples", lambda: host(n_samples=size - 8)),
        ("flush ids misaligned", lambda: ist._c("_streams_flush_dev")(ist._h, off(d["ids"], 4), vp(d["first"]), 2, vp(out), None)),
        ("flush n_ids > n_streams", lambda: ist._c("_streams_flush_dev")(ist._h, vp(d["ids"]), vp(d["first"]), 4, vp(out), None)),
        ("flush n_ids < 0", lambda: ist._c("_streams_flush_dev")(ist._h, vp(d["ids"]), vp(d["first"]), -1, vp(out), None)),
        ("reset ids misaligned", lambda: ist._c("_streams_reset_dev")(ist._h, off(d["ids"], 4), 2)),
        ("host flush duplicate id", lambda: ist._c("_streams_flush")(
            ist._h, vp(np.array([1, 1], np.int64)), vp(np.array([0, 1024], np.int64)), 2, 4096, vp(z), None)),
        ("host flush id out of range", lambda: ist._c("_streams_flush")(
            ist._h, vp(np.array([1, 3], np.int64)), vp(np.array([0, 1024], np.int64)), 2, 4096, vp(z), None)),
        ("host flush overlapping", lambda: ist._c("_streams_flush")(
            ist._h, vp(np.array([1, 2], np.int64)), vp(np.array([0, 700], np.int64)), 2, 4096, vp(z), None)),
    ]
    for what, call in bad:
        rc = call()
        assert rc == -1 and text(), (what, rc)
    # NULL outputs, no chunks, no frames: nothing launched, nothing advanced
    assert dev(out_=C.c_void_p(None), f32_=C.c_void_p(None)) == 0
    assert dev(n_=0, total=0) == 0
    # every stream is as the valid call left it
    feed(ist, st, [(2, 3), (0, 3), (1, 3)], "valid again")
    fi, ffl = flush_all(ist, 3)
    st.check(fi, ffl, ref, "after the rejected calls")
    ist.close()
