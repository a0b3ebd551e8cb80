"""hipGraph capture and replay of the "_dev" entries (include/jdsp.h, "Graph capture").  The header makes capture part
of the ABI; this module captures every entry it names and replays it, by the three classes the header describes:

  S  stateless entries: a replay recomputes from what the buffers hold NOW.  Scalars and pointers are baked into the
     launch; buffer contents and the device-side offset and id arrays are read at replay.  One captured call, three
     replays with three contents (and three sets of offsets), each equal to an eager call on a fresh handle and fresh
     buffers, byte for byte, sentinels outside the written spans included.
  D  state that lives on the device only (jdsp_geq_*, jdsp_nlms_*, the live streams): every replay continues the
     streams.  The concatenated replays equal the restatement of the whole stream (equaliser, NLMS) or a fresh
     single-stream handle's process + flush (live streams), bit for bit.
  H  state that the host carries (OlaStream::cur, h->cur / h->calls): a captured call belongs to the position the
     handle had at capture.  A graph of consecutive calls replayed ONCE, there, between eager calls, equals the same
     calls made eagerly on a fresh handle, bit for bit.  A second replay is unsupported and is not tested.

Inside a capture only C entries run, through ctypes, on buffers allocated before it; every graph is one linear chain on
one stream (graph_replay_cases.capture).  Every handle is warm first: one eager call with the same scalars, the
matching reserve, a synchronise."""
import ctypes as C

import numpy as np
import pytest

import graph_replay_cases as G
from graph_replay_cases import dev_fill, dev_of, download, lib, ok, upload, vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def sync():
    import torch
    torch.cuda.synchronize()


def close(h):
    if h is not None:
        h.close()


# ---- class S -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.STATELESS))
def test_stateless_replay_equals_eager(eng, name):
    case = G.STATELESS[name]()
    # the yardstick: every content through an eager call on a fresh handle and fresh buffers
    want = []
    for content in case.contents:
        h = case.make(eng)
        B = case.buffers(content)
        case.reserve(eng, h)
        eng._use_torch_stream()
        ok(eng, case.call(eng, h, B), case.entry)
        sync()
        want.append(case.results(B))
        close(h)
    if case.verify:
        case.verify(want)
    # one capture, on a warm handle
    h = case.make(eng)
    B = case.buffers(case.contents[0])
    case.reserve(eng, h)
    eng._use_torch_stream()
    ok(eng, case.call(eng, h, B), case.entry + " (warm)")
    sync()
    g = G.capture(eng, lambda: ok(eng, case.call(eng, h, B), case.entry + " (captured)"))
    for i, content in enumerate(case.contents):
        for k, v in content.items():
            upload(B[k], v)
        for k in case.outs:
            B[k].fill_(G.FILL)
        G.replay(eng, g)
        got = case.results(B)
        for k in case.outs:
            assert got[k].tobytes() == want[i][k].tobytes(), \
                (name, "replay", i, k, "%d bytes differ from the eager call" % int((G.as_bytes(got[k]) != G.as_bytes(want[i][k])).sum()))
            assert not np.all(G.as_bytes(got[k]) == G.FILL), (name, i, k, "nothing was written")
        if case.outside:
            for k, keep in case.outside(content).items():
                assert np.all(G.as_bytes(got[k]).reshape(keep.size, -1)[keep.reshape(-1)] == G.FILL), \
                    (name, "replay", i, k, "written outside the spans")
    k = next(iter(case.outs))
    assert want[0][k].tobytes() != want[1][k].tobytes(), (name, "the contents must differ")
    close(h)


# ---- class D: equaliser and NLMS -----------------------------------------------------------------------------------
def test_geq_every_replay_continues_the_streams(eng):
    from test_streamfilter_gpu import geq_pool, geq_want
    n_streams, n, pitch, reps = 9, 13, 24, 4
    pool = geq_pool()
    g = eng.geq(n_streams)
    x = dev_of(np.full((n_streams, pitch), 999, np.int16))
    out, pre = dev_fill(n_streams * pitch * 2), dev_fill(n_streams * pitch * 8)

    def call():
        ok(eng, lib().jdsp_geq_process_dev(g._h, vp(x), n, pitch, vp(out), vp(pre)), "jdsp_geq_process_dev")

    eng._use_torch_stream()
    call()                                                             # warm; the reset takes its effect back
    g.reset()
    sync()
    graph = G.capture(eng, call)
    outs, pres = [], []
    for k in range(reps):
        buf = np.full((n_streams, pitch), 999, np.int16)
        buf[:, :n] = pool[:, k * n:(k + 1) * n]
        upload(x, buf)
        out.fill_(G.FILL)
        pre.fill_(G.FILL)
        G.replay(eng, graph)
        o, p = download(out, np.int16, (n_streams, pitch)), download(pre, np.float64, (n_streams, pitch))
        assert np.all(o[:, n:] == G.sentinel(np.int16)) and np.all(p[:, n:].view(np.int64) == G.sentinel(np.int64))
        outs.append(o[:, :n])
        pres.append(p[:, :n])
    w_out, w_pre, w_state = geq_want(7, reps * n)
    assert np.array_equal(np.concatenate(outs, axis=1), w_out)
    assert np.array_equal(np.concatenate(pres, axis=1), w_pre)
    assert np.array_equal(g.state(), w_state)
    g.close()


def test_nlms_every_replay_continues_the_streams(eng):
    import streamfilter_ref as R
    from test_streamfilter_gpu import nlms_pool
    n_streams, L, n, reps = 3, 64, 255, 4
    pitch = 256
    xs, rs = (a[:n_streams, :reps * n] for a in nlms_pool())
    f = eng.nlms(n_streams, L)
    x, r = dev_of(np.zeros((n_streams, pitch), np.int16)), dev_of(np.zeros((n_streams, pitch), np.int16))
    est, err, pre = dev_fill(n_streams * pitch * 2), dev_fill(n_streams * pitch * 2), dev_fill(n_streams * pitch * 8)

    def call():
        ok(eng, lib().jdsp_nlms_process_dev(f._h, vp(x), vp(r), n, pitch, vp(est), vp(err), vp(pre)), "jdsp_nlms_process_dev")

    eng._use_torch_stream()
    call()
    f.reset()
    sync()
    graph = G.capture(eng, call)
    got = [[], [], []]
    for k in range(reps):
        for t, src in ((x, xs), (r, rs)):
            buf = np.full((n_streams, pitch), 999, np.int16)
            buf[:, :n] = src[:, k * n:(k + 1) * n]
            upload(t, buf)
        for t in (est, err, pre):
            t.fill_(G.FILL)
        G.replay(eng, graph)
        for i, (t, dt) in enumerate(((est, np.int16), (err, np.int16), (pre, np.float64))):
            a = download(t, dt, (n_streams, pitch))
            assert np.all(G.as_bytes(a[:, n:]) == G.FILL), "written past the samples"
            got[i].append(a[:, :n])
    want = [R.nlms(xs[s], rs[s], L, order="device") for s in range(n_streams)]
    for i, what in enumerate(("estimate", "error", "precast")):
        assert np.array_equal(np.concatenate(got[i], axis=1), np.stack([w[i] for w in want])), what
    cf, kp = f.state()
    assert np.array_equal(cf, np.stack([w[3][0] for w in want])), "coefficients"
    assert np.array_equal(kp, np.stack([w[3][1] for w in want])), "keep"
    f.close()


# ---- class D: the live streams -------------------------------------------------------------------------------------
def live_cfg(kind, a, b):
    if kind == "stftmask":
        from test_stftmask_gpu import cfg_of, stream_combo
        return cfg_of(a, b, stream_combo(a))                           # a: hop, b: mask kind
    from test_istft_batch_gpu import cfg_of
    return cfg_of(1024 if a == 256 else 512, a, b)                     # a: hop, b: layout


LIVE = [("stftmask", 256, "real"), ("stftmask", 256, "complex"), ("stftmask", 512, "real"), ("stftmask", 512, "complex"),
        ("istft", 256, "full"), ("istft", 128, "half")]
LIVE_IDS = ["%s-%d-%s" % c for c in LIVE]


class Own:
    """the handle's own stream (process_dev / flush_dev, eagerly, through the wrappers) in two calls and a flush,
    interleaved with the replays: F = 9 frames, 4 and 5"""

    def __init__(self, eng, kind, cfg, h, seed):
        import torch
        rng = np.random.default_rng(seed)
        self.h, self.kind, F = h, kind, 9
        n, hop = cfg["n_fft"], cfg["hop"]
        if kind == "stftmask":
            from test_stftmask_gpu import mask_of, pcm_of, run
            pcm, mask = pcm_of(rng, F, hop), mask_of(rng, cfg["mask_kind"], F)
            o, f, to, tf = run(eng, pcm, mask, F, **cfg)
            d_pcm, d_mask = torch.from_numpy(pcm).cuda(), torch.from_numpy(mask).cuda()
            self.parts = [(d_pcm[:hop * 3 + n], d_mask[:4], 4), (d_pcm[hop * 4:], d_mask[4:], F - 4)]
        else:
            from test_istft_gpu import rows, run
            spec = rows(rng, F, n, n // 2 + 1 if cfg["layout"] == "half" else n)
            o, f, to, tf = run(eng, spec, **cfg)
            t = torch.from_numpy(spec).cuda()
            self.parts = [(t[:4],), (t[4:],)]
        self.want = (np.concatenate([o, to]), np.concatenate([f, tf]))
        self.got = []

    def step(self, i):
        self.got.append(self.h.process(*self.parts[i], want_f32=True))

    def finish(self):
        import torch
        self.got.append(self.h.flush(want_f32=True))
        sync()
        gi = torch.cat([g[0] for g in self.got]).cpu().numpy()
        gf = torch.cat([g[1] for g in self.got]).cpu().numpy()
        assert np.array_equal(gi, self.want[0]), "own stream int16"
        assert np.array_equal(gf.view(np.int32), self.want[1].view(np.int32)), "own stream float32"


def warm(eng, lv, chunks):
    """one eager delivery with the captured scalars and an eager flush, which leaves every stream fresh again"""
    eng._use_torch_stream()
    lv.load(chunks)
    lv.deliver()
    lv.flush()
    sync()


# six live streams at every configuration; ONE live stream at one configuration per handle
LIVE_RUNS = [(c, 6) for c in LIVE] + [(("stftmask", 256, "real"), 1), (("istft", 256, "full"), 1)]


@pytest.mark.parametrize("case,n_streams", LIVE_RUNS, ids=["%s-%d-%s-streams%d" % (c + (n,)) for c, n in LIVE_RUNS])
def test_live_streams_every_replay_continues_the_streams(eng, case, n_streams):
    """ONE captured delivery (n_chunks and n_frames_total fixed), replayed five times with other ids, other cuts and
    other offsets every time, then one captured flush: every stream equals a fresh single-stream handle's process +
    flush.  With n_streams = 1 this is the replayable form of the handle's own stream."""
    kind, a, b = case
    cfg = live_cfg(*case)
    plans = G.live_plan(cfg["n_fft"] // cfg["hop"], n_streams)
    h, st, lv, ref = G.live_case(eng, kind, cfg, n_streams, 9000 + a + len(b) + n_streams, G.totals_of(plans, n_streams))
    own = Own(eng, kind, cfg, h, 77 + a) if n_streams > 1 else None
    warm(eng, lv, plans[0])
    g, gf = G.capture(eng, lv.deliver), G.capture(eng, lv.flush)
    for k, chunks in enumerate(plans):
        first = lv.load(chunks)
        G.replay(eng, g)
        lv.take(chunks, first, (case, "replay", k))
        if own and k in (1, 3):
            own.step(k // 2)
    lv.f_i.fill_(G.FILL)
    lv.f_f.fill_(G.FILL)
    G.replay(eng, gf)
    fi, ff = lv.flushed()
    st.check(fi, ff, ref, case)
    if n_streams > 1:
        assert not fi[5].any() and not ff[5].view(np.int32).any(), "a stream never fed flushes to exact zeros"
        own.finish()
    h.close()


@pytest.mark.parametrize("case", LIVE, ids=LIVE_IDS)
def test_live_streams_captured_pair_and_reset(eng, case):
    """The captured pair of DESIGN 3.6: TWO consecutive deliveries and a reset of one listed stream in ONE graph,
    replayed twice; then a single delivery and the flush.  The stream that is reset starts again after each replay."""
    kind, a, b = case
    cfg = live_cfg(*case)
    R, hop = cfg["n_fft"] // cfg["hop"], cfg["hop"]
    plans, r = G.live_plan(R), 4
    totals = G.totals_of(plans, 6)
    h, st, lv, ref = G.live_case(eng, kind, cfg, 6, 9100 + a + len(b), totals)
    lv2 = G.Live(eng, kind, h, st, lv.n_chunks, lv.n_total, lv.pitch, lv.cap)
    upload(lv.r_ids, np.array([r], np.int64))
    warm(eng, lv, plans[0])
    warm(eng, lv2, plans[1])

    def pair():
        lv.deliver()
        lv2.deliver()
        lv.reset_one()

    g2, g1, gf = G.capture(eng, pair), G.capture(eng, lv.deliver), G.capture(eng, lv.flush)
    fed = [sum(f for c in plans[:k] for s, f in c if s == r) for k in range(6)]     # frames of stream r before delivery k
    for k in (0, 2):
        first = lv.load(plans[k])
        for s, f in plans[k]:
            st.done[s] += f                                            # the second delivery is cut where the first ends
        first2 = lv2.load(plans[k + 1])
        for s, f in plans[k]:
            st.done[s] -= f
        G.replay(eng, g2)
        lv.take(plans[k], first, (case, "delivery", k))
        lv2.take(plans[k + 1], first2, (case, "delivery", k + 1))
        if k == 2:                                                     # what stream r gave since the first replay's reset
            whole, st.totals[r] = st.totals[r], fed[4]
            mid = st.reference(eng, cfg, first=[fed[2] if s == r else t for s, t in enumerate(st.totals)])[r]
            st.totals[r] = whole
            n = hop * (fed[4] - fed[2])
            assert n > 0
            assert np.array_equal(np.concatenate(st.got_i[r]), mid[0][:n]), (case, "a fresh stream after the first reset")
            assert np.array_equal(np.concatenate(st.got_f[r]).view(np.int32), mid[1][:n].view(np.int32)), case
        st.got_i[r], st.got_f[r] = [], []                              # the reset: stream r starts again
    first = lv.load(plans[4])
    G.replay(eng, g1)
    lv.take(plans[4], first, (case, "delivery", 4))
    lv.f_i.fill_(G.FILL)
    lv.f_f.fill_(G.FILL)
    G.replay(eng, gf)
    fi, ff = lv.flushed()
    late = st.reference(eng, cfg, first=[fed[4] if s == r else t for s, t in enumerate(totals)])
    st.check(fi, ff, ref, (case, "streams that were not reset"), streams=[s for s in range(6) if s != r])
    st.check(fi, ff, late, (case, "the stream that was reset"), streams=(r,))
    h.close()


def test_stftmask_frames_recomputed_sums_over_back_to_back_replays(eng):
    """A captured delivery counts under the one call number it was captured with: three replays back to back give three
    times the figure of one eager call on the same input, which must be above 0 (a notched tone)."""
    import stftmask_fp32_ref as S
    from test_stftmask_gpu import cfg_of
    c = min((c for c in S.cases() if c["name"].startswith("notch")), key=lambda c: c["pcm"].size)
    pcm, mask, F = np.array(c["pcm"]), np.array(c["mask"]), c["F"]
    assert mask.ndim == 2 and mask.shape[0] >= F
    sm = eng.stft_mask(**cfg_of(c["hop"], c["kind"], c["combo"]))
    sm.open_streams(2)
    d = [dev_of(a) for a in (pcm, mask, np.array([1], np.int64), np.array([0], np.int64), np.array([0, F], np.int64))]
    out = dev_fill(pcm.size * 2)

    def deliver():
        ok(eng, sm._c("_streams_dev")(sm._h, vp(d[0]), vp(d[1]), mask.shape[1], vp(d[2]), vp(d[3]), vp(d[4]), 1, F, vp(out),
                                      None), "jdsp_stftmask_streams_dev")

    eng._use_torch_stream()
    deliver()
    one = sm.frames_recomputed()
    print("one eager call: %d of %d frames recomputed" % (one, F))
    assert one > 0, "the notched tone must recompute frames"
    ok(eng, sm._c("_streams_reset_dev")(sm._h, None, 0), "reset")
    deliver()                                                          # the call before the captured one: it zeroes the word
    ok(eng, sm._c("_streams_reset_dev")(sm._h, None, 0), "reset")      # that the captured call counts in
    sync()

    def body():
        deliver()
        ok(eng, sm._c("_streams_reset_dev")(sm._h, None, 0), "reset")  # the same input from a fresh stream, every replay

    g = G.capture(eng, body)
    for _ in range(3):
        g.replay()
    sync()
    three = sm.frames_recomputed()
    print("three replays back to back: %d" % three)
    assert three == 3 * one
    sm.close()


# ---- class H -------------------------------------------------------------------------------------------------------
class Ola(G.Carried):
    """jdsp_istft_process_dev / jdsp_stftmask_process_dev + _flush_dev on the handle's own stream"""

    def __init__(self, eng, kind, cfg, total, seed):
        super().__init__(eng)
        rng = np.random.default_rng(seed)
        self.kind, self.n, self.hop = kind, cfg["n_fft"], cfg["hop"]
        if kind == "stftmask":
            from test_stftmask_gpu import BINS, mask_of, pcm_of
            self.h, self.pitch = eng.stft_mask(**cfg), BINS
            self.pcm, self.rows = pcm_of(rng, total, self.hop), mask_of(rng, cfg["mask_kind"], total)
        else:
            from test_istft_gpu import rows
            self.h = eng.istft(**cfg)
            self.pitch = self.n // 2 + 1 if cfg["layout"] == "half" else self.n
            self.rows = rows(rng, total, self.n, self.pitch)

    def prepare(self, sizes):
        self.bufs, a = [], 0
        for f in sizes:
            b = {"rows": dev_of(self.rows[a:a + f]), "i": dev_fill(f * self.hop * 2), "f": dev_fill(f * self.hop * 4), "F": f}
            if self.kind == "stftmask":
                b["pcm"] = dev_of(self.pcm[self.hop * a:self.hop * (a + f - 1) + self.n])
            self.bufs.append(b)
            a += f
        self.tail = (dev_fill((self.n - self.hop) * 2), dev_fill((self.n - self.hop) * 4))

    def issue(self, k):
        b = self.bufs[k]
        if self.kind == "stftmask":
            rc = lib().jdsp_stftmask_process_dev(self.h._h, vp(b["pcm"]), vp(b["rows"]), self.pitch, b["F"], vp(b["i"]), vp(b["f"]))
        else:
            rc = lib().jdsp_istft_process_dev(self.h._h, vp(b["rows"]), self.pitch, b["F"], vp(b["i"]), vp(b["f"]))
        ok(self.eng, rc, "jdsp_%s_process_dev" % self.kind)

    def read(self, k, info):
        return [download(self.bufs[k]["i"], np.int16), download(self.bufs[k]["f"], np.float32)]

    def finish(self):
        ok(self.eng, self.h._c("_flush_dev")(self.h._h, vp(self.tail[0]), vp(self.tail[1])), "flush_dev")

    def read_finish(self):
        return [download(self.tail[0], np.int16), download(self.tail[1], np.float32)]

    def reset(self):
        self.h.reset()


class Blocks(G.Carried):
    """The block-stream handles: jdsp_denoise / jdsp_fastconv / jdsp_mvdr / jdsp_mvdrn _process_dev.  pcm: [planes, n]
    int16, every plane cut into the calls' blocks."""

    def __init__(self, eng, what, h, pcm, block, out_planes=1, reserve=None, getter=None):
        super().__init__(eng)
        self.what, self.h, self.pcm, self.block, self.out_planes = what, h, np.atleast_2d(pcm), block, out_planes
        self.reserve, self.getter = reserve, getter

    def prepare(self, sizes):
        if self.reserve:
            ok(self.eng, self.reserve(self.h._h, max(sizes)), self.what + " reserve")
        self.bufs, a = [], 0
        for nb in sizes:
            n = nb * self.block
            self.bufs.append({"in": [dev_of(p[a:a + n]) for p in self.pcm], "planes": dev_of(self.pcm[:, a:a + n]), "nb": nb,
                              "out": dev_fill(self.out_planes * n * 2), "pre": dev_fill(self.out_planes * n * 4)})
            a += n

    def issue(self, k):
        b, n_out, L = self.bufs[k], C.c_long(-1), lib()
        o, p, nb = vp(b["out"]), vp(b["pre"]), b["nb"]
        if self.what == "denoise":
            rc = L.jdsp_denoise_process_dev(self.h._h, vp(b["in"][0]), nb, o, p, C.byref(n_out))
        elif self.what == "fastconv":
            rc = L.jdsp_fastconv_process_dev(self.h._h, vp(b["in"][0]), nb, o, p, C.byref(n_out))
        elif self.what == "mvdr":
            rc = L.jdsp_mvdr_process_dev(self.h._h, vp(b["in"][0]), vp(b["in"][1]), nb, o, p, C.byref(n_out))
        else:
            rc = L.jdsp_mvdrn_process_dev(self.h._h, vp(b["planes"]), nb * self.block, nb, o, p, C.byref(n_out))
        ok(self.eng, rc, "jdsp_%s_process_dev" % self.what)
        assert 0 <= n_out.value <= nb
        return n_out.value

    def read(self, k, n_out):
        n = self.out_planes * n_out * self.block
        return [np.array([n_out]), download(self.bufs[k]["out"], np.int16)[:n], download(self.bufs[k]["pre"], np.float32)[:n]]

    def state(self):
        return self.getter(self.h) if self.getter else []

    def reset(self):
        self.h.reset()


def speech_blocks(seed, n_blocks, quiet_runs, block=512):
    """loud white blocks with quiet runs (sigma 45: non-voice), so that estimation events occur"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 3000, n_blocks * block)
    for b0, nb in quiet_runs:
        x[b0 * block:(b0 + nb) * block] = rng.normal(0, 45, nb * block)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def denoise_noise(h):
    noise = np.zeros(h.n_fft, np.float64)
    assert lib().jdsp_denoise_noise(h._h, noise.ctypes.data_as(C.c_void_p)) == 0
    return [noise]


def make_carried(eng, what):
    """a fresh handle of the kind `what` behind its Carried adapter, the same stream every time"""
    L = lib()
    if what.startswith("ola-"):
        _, kind, a, b = what.split("-")
        return Ola(eng, kind, live_cfg(kind, int(a), b), 24, 9200 + int(a))
    if what.startswith("denoise-"):
        mode = 0 if what.endswith("ss") else 1
        pcm = speech_blocks(9300 + mode, 40, [(1, 12), (20, 11)])
        return Blocks(eng, "denoise", eng.denoiser(mode), pcm, 512, reserve=L.jdsp_denoise_reserve, getter=denoise_noise)
    if what == "fastconv-1024-hrir":
        rng = np.random.default_rng(3)
        taps = np.stack([rng.normal(size=256) * np.exp(-np.arange(256) / 40.0), rng.normal(size=256) * np.exp(-np.arange(256) / 55.0)])
        fc = eng.fastconv(taps, 1024)
        assert fc.block == 769 and fc.hist_blocks == 1
        return Blocks(eng, "fastconv", fc, G.noise_i16(9400, 12 * 769, 2000.0), 769, out_planes=2, reserve=L.jdsp_fastconv_reserve)
    if what == "fastconv-8192":
        rng = np.random.default_rng(1)
        fc = eng.fastconv(rng.normal(size=7169) * np.exp(-np.arange(7169) / 1500.0) * 0.05, 8192)
        assert fc.block == 1024 and fc.hist_blocks == 7
        return Blocks(eng, "fastconv", fc, G.noise_i16(9401, 16 * 1024, 2000.0), 1024, reserve=L.jdsp_fastconv_reserve)
    from test_mvdr_multi_gpu import array_scene
    if what == "mvdr":
        pcm = array_scene(9500, 2, 20, quiet=((0, 6), (12, 4)))[0]
        return Blocks(eng, "mvdr", eng.mvdr(0.0), pcm, 512, getter=lambda h: [h.corr()])
    assert what == "mvdrn-4"
    pcm, _, delays = array_scene(9501, 4, 20, quiet=((0, 6), (12, 4)))
    return Blocks(eng, "mvdrn", eng.mvdr_multi(4, delays, 1e-3), pcm, 512)


# what, the calls of the stream, the calls captured into one graph: a capture across the start-up boundary (the OLA
# stream's first frames, denoise's first two blocks, fastconv's silent head calls < n_hist, MVDR's first block) and one
# in the steady state, for every handle
CARRIED = [
    ("ola-stftmask-256-real", [3, 1, 5, 2, 6, 7], (0, 3)), ("ola-stftmask-256-real", [3, 1, 5, 2, 6, 7], (2, 5)),
    ("ola-stftmask-512-complex", [1, 4, 2, 9, 8], (0, 2)), ("ola-stftmask-512-complex", [1, 4, 2, 9, 8], (1, 4)),
    ("ola-istft-256-full", [3, 1, 5, 2, 6, 7], (0, 3)), ("ola-istft-256-full", [3, 1, 5, 2, 6, 7], (2, 5)),
    ("ola-istft-128-half", [1, 4, 2, 9, 8], (0, 2)), ("ola-istft-128-half", [1, 4, 2, 9, 8], (1, 4)),
    ("denoise-ss", [1, 2, 3, 9, 5, 13, 7], (0, 3)), ("denoise-ss", [1, 2, 3, 9, 5, 13, 7], (3, 6)),
    ("denoise-wiener", [1, 2, 3, 9, 5, 13, 7], (0, 3)), ("denoise-wiener", [1, 2, 3, 9, 5, 13, 7], (3, 6)),
    ("fastconv-1024-hrir", [1, 2, 3, 4, 2], (0, 3)), ("fastconv-1024-hrir", [1, 2, 3, 4, 2], (2, 4)),
    ("fastconv-8192", [2, 3, 1, 4, 3, 2, 1], (1, 4)), ("fastconv-8192", [2, 3, 1, 4, 3, 2, 1], (4, 6)),
    ("mvdr", [1, 2, 3, 4, 6, 4], (0, 3)), ("mvdr", [1, 2, 3, 4, 6, 4], (2, 5)),
    ("mvdrn-4", [1, 2, 3, 4, 6, 4], (0, 3)), ("mvdrn-4", [1, 2, 3, 4, 6, 4], (2, 5)),
]


@pytest.mark.parametrize("what,sizes,graph", CARRIED, ids=["%s-calls%d-%d" % (w, g[0], g[1] - 1) for w, s, g in CARRIED])
def test_host_carried_graph_replayed_once_in_place(eng, what, sizes, graph):
    """Eager calls, ONE graph of two or three consecutive calls of unequal sizes replayed once where the handle stood at
    capture, eager calls again (and the flush): the whole output stream and the state getters equal the same calls made
    eagerly on a fresh handle, bit for bit.  The handle is warm: the same calls ran eagerly on it first (they size every
    workspace), then its reset.  That eager pass must equal the fresh handle's too -- the entries are reproducible from
    run to run, so no tolerance is needed anywhere in this test."""
    fresh = make_carried(eng, what)
    want, want_state = fresh.run(sizes)
    fresh.h.close()
    assert all(s.any() for s in want_state), (what, "the getters are still zero: no estimation event, the input is wrong")
    c = make_carried(eng, what)
    again, again_state = c.run(sizes)
    assert G.same_bytes(again, want) and G.same_bytes(again_state, want_state), (what, "two eager runs differ")
    c.reset()
    sync()
    got, got_state = c.run(sizes, graph)
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), \
            (what, "output", i, "%d bytes differ" % int((G.as_bytes(x) != G.as_bytes(y)).sum()))
    assert G.same_bytes(got_state, want_state), (what, "state getter")
    c.h.close()
