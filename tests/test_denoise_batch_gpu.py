"""Batched spectral subtraction / Wiener (jdsp_denoise_batch*, Denoiser.process_batch): a batch of ragged utterances,
each a fresh stream of the reference's main(), in one launch sequence.

The yardstick for every utterance is the CPU oracle's block-by-block state machine on the utterance ALONE
(oracle.denoise_trace), held to the bars of test_denoise_gpu.py: check_stream on the pre-cast samples and the int16
ones (1e-5 of the utterance's peak, +-1 LSB), VAD flags equal, the last estimate within TOL * max(noise, 1).  The
batch writes time-aligned: emitted block k of utterance u lies where its input block k + 1 lies, so the first and the
last block of a span are never written (a sentinel stays there on the device path, zero on the host path), and neither
is anything outside the spans."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_fp32_ref as R
from test_denoise_gpu import TOL, check_stream, speechlike
from test_denoise_periodic_gpu import check_blocks

pytestmark = pytest.mark.gpu

B = 512
SENT_I = np.int16(-12345)
SENT_F = np.float32(-7777.5)
SENT_N = np.float32(-3.25)
BOUNDARY = [0, 1, 2, 3, 0, 5, 12, 40, 333, 1, 70]


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def vp(a, off=0):
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr() + off)
    return C.c_void_p(a.ctypes.data + off)


def quiet(rng, n):
    """sigma 45 white: non-voice (speechlike's quiet stretches)"""
    return np.clip(np.rint(rng.normal(0, 45, n * B)), -32768, 32767).astype(np.int16)


def loud(rng, n):
    return np.clip(np.rint(rng.normal(0, 3000, n * B)), -32768, 32767).astype(np.int16)


_TRACES = {}


def trace_of(oracle, mode, pcm):
    """oracle.denoise_trace of one utterance alone, computed once per (mode, samples) and shared, read-only"""
    key = (mode, pcm.tobytes())
    if key not in _TRACES:
        t = oracle.denoise_trace(mode, pcm)
        for a in t:
            a.setflags(write=False)
        _TRACES[key] = t
    return _TRACES[key]


class Batch:
    """Utterances (int16 arrays of whole blocks, possibly empty) packed with `gap` samples behind every span; the gaps
    are full scale, so reading one would show."""

    def __init__(self, utts, gap=0, lead=0):
        self.utts = [np.ascontiguousarray(u, np.int16) for u in utts]
        self.counts = np.array([u.size // B for u in self.utts], np.int64)
        starts, pos = [], lead
        for u in self.utts:
            starts.append(pos)
            pos += u.size + gap
        self.sample_first = np.array(starts, np.int64)
        self.block_first = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.n_samples = pos
        self.pcm = np.full(max(pos, 1), 32767, np.int16)[:pos]
        for s, u in zip(starts, self.utts):
            self.pcm[s:s + u.size] = u
        self.n_utts, self.n_total = len(self.utts), int(self.block_first[-1])

    def run_host(self, d):
        return d.process_batch(self.pcm, self.counts, self.sample_first, want_precast=True, want_flags=True, want_noise=True)

    def run_dev(self, d, out=True, pre=True, flags=True, noise=True):
        """The device entry with sentinel-filled outputs (numpy arrays back; None where not asked for)."""
        import torch
        from jeicyboodsp_amd._lib import lib as L
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
        full = lambda n, v, dt: torch.full((max(n, 1),), v, dtype=dt, device="cuda")     # noqa: E731
        d_pcm, d_s, d_b = t(self.pcm if self.n_samples else np.zeros(1, np.int16)), t(self.sample_first), t(self.block_first)
        d_o = full(self.n_samples, int(SENT_I), torch.int16) if out else None
        d_p = full(self.n_samples, float(SENT_F), torch.float32) if pre else None
        d_f = full(self.n_total, 77, torch.uint8) if flags else None
        d_n = full(self.n_utts * 1024, float(SENT_N), torch.float32) if noise else None
        d.reserve_batch(self.n_total, self.n_utts)
        d.eng._use_torch_stream()
        rc = L.jdsp_denoise_batch_dev(d._h, vp(d_pcm), vp(d_s), vp(d_b), self.n_utts, self.n_total, vp(d_o), vp(d_p),
                                      vp(d_f), vp(d_n))
        assert rc == 0, L.jdsp_last_error(d.eng._h)
        torch.cuda.synchronize()
        back = lambda x, n: None if x is None else x.cpu().numpy()[:n]       # noqa: E731
        nl = back(d_n, self.n_utts * 1024)
        return (back(d_o, self.n_samples), back(d_p, self.n_samples), back(d_f, self.n_total),
                None if nl is None else nl.reshape(self.n_utts, 1024))

    def utt_results(self, res, u):
        """(out, precast, flags, noise_last) of utterance u: its whole span, its blocks' flags, its estimate"""
        out, pre, flags, noise = res
        s, n = int(self.sample_first[u]), self.utts[u].size
        f0, f1 = int(self.block_first[u]), int(self.block_first[u + 1])
        return out[s:s + n], pre[s:s + n], flags[f0:f1], noise[u]

    def check(self, oracle, mode, res, fill_i, fill_f, what):
        """Every utterance against the oracle on it alone; what no launch writes holds fill_i / fill_f."""
        out, pre, flags, noise = res
        covered = np.zeros(self.n_samples, bool)
        for u, x in enumerate(self.utts):
            nb = x.size // B
            o, p, f, nz = self.utt_results(res, u)
            s = int(self.sample_first[u])
            covered[s + B:s + max(nb - 1, 1) * B] = nb >= 3
            if nb == 0:
                assert not nz.any(), (what, u)
                continue
            o_out, o_pre, o_flags, noises, ver = trace_of(oracle, mode, x)
            assert np.array_equal(f.astype(np.int32), o_flags), (what, u)
            assert np.abs(nz - noises[-1]).max() <= TOL * max(noises[-1].max(), 1.0), (what, u)
            if noises.shape[0] == 1:
                assert not nz.any(), (what, u)                      # nothing latched: zeros, exactly
            if nb >= 3:
                check_stream(o[B:(nb - 1) * B], p[B:(nb - 1) * B], o_out, o_pre)
        assert np.all(out[~covered] == fill_i), what               # outside the spans, first and last blocks
        assert np.all(pre[~covered] == fill_f), what


# ---- 1. boundary sizes ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boundary_utts():
    return tuple(speechlike(500 + u, n) if n else np.zeros(0, np.int16) for u, n in enumerate(BOUNDARY))


@pytest.mark.parametrize("gap", [0, 2, 514])
@pytest.mark.parametrize("mode", [0, 1])
def test_boundary_sizes(eng, oracle, mode, gap):
    b = Batch(boundary_utts(), gap=gap)
    d = eng.denoiser(mode)
    b.check(oracle, mode, b.run_dev(d), SENT_I, SENT_F, "device, gap %d" % gap)
    b.check(oracle, mode, b.run_host(d), 0, 0.0, "host, gap %d" % gap)
    d.close()


def test_null_outputs_and_nothing_to_do(eng, oracle):
    from jeicyboodsp_amd._lib import lib as L
    b = Batch(boundary_utts()[5:9], gap=2, lead=16)
    d = eng.denoiser(0)
    whole = b.run_dev(d)
    b.check(oracle, 0, whole, SENT_I, SENT_F, "all four outputs")
    # one output at a time gives the same bits
    for i in range(4):
        only = b.run_dev(d, *[j == i for j in range(4)])
        assert [x is not None for x in only] == [j == i for j in range(4)]
        assert np.array_equal(only[i], whole[i]), i
    assert b.run_dev(d, False, False, False, False) == (None, None, None, None)
    # nothing to launch: no utterance, empty utterances, none with a third block
    assert L.jdsp_denoise_batch(d._h, None, 0, None, None, 0, None, None, None, None) == 0
    assert L.jdsp_denoise_batch_dev(d._h, None, None, None, 0, 0, None, None, None, None) == 0
    for utts in ([], [np.zeros(0, np.int16)] * 3, [speechlike(1, 2), np.zeros(0, np.int16), speechlike(2, 1), speechlike(3, 2)]):
        e = Batch(utts, gap=2)
        e.check(oracle, 0, e.run_dev(d), SENT_I, SENT_F, "short utterances, device")
        res = e.run_host(d)
        e.check(oracle, 0, res, 0, 0.0, "short utterances, host")
        assert d.frames_recomputed() == 0
    d.close()


# ---- 2. state must not cross an utterance boundary -------------------------------------------------------------------
def crossing_utts():
    """(utterances, {name: index}); the quiet stretches' flags are asserted against the oracle in the test"""
    rng = np.random.default_rng(20)
    utts = [
        np.concatenate([loud(rng, 5), quiet(rng, 9)]),          # 0 ends with 9 quiet blocks ...
        np.concatenate([quiet(rng, 9), loud(rng, 6)]),          # 1 ... and this one begins with 9: no latch in either
        np.concatenate([quiet(rng, 14), loud(rng, 6)]),         # 2 latches an estimate ...
        loud(rng, 12),                                          # 3 ... and this one is loud throughout: zero estimate
        np.concatenate([loud(rng, 4), quiet(rng, 5)]),          # 4 a quiet run of 5 comes in ...
        np.concatenate([quiet(rng, 10), loud(rng, 6)]),         # 5 ... exactly 10 quiet blocks: the latch is at block 9
    ]
    return utts


@pytest.mark.parametrize("mode", [0, 1])
def test_state_does_not_cross_an_utterance_boundary(eng, oracle, mode):
    utts = crossing_utts()
    tr = [trace_of(oracle, mode, x) for x in utts]
    flags = [t[2] for t in tr]
    # the scenario is what it says (the quiet stretches are Gaussian: their flags are the oracle's to decide)
    assert not flags[0][5:].any() and flags[0][:5].all() and not flags[1][:9].any() and flags[1][9:].all()
    assert tr[0][3].shape[0] == 1 and tr[1][3].shape[0] == 1           # nothing latched in either
    assert not flags[2][:14].any() and tr[2][3].shape[0] == 2 and np.abs(tr[2][3][-1]).max() > 100
    assert flags[3].all() and tr[3][3].shape[0] == 1
    assert not flags[4][4:].any() and not flags[5][:10].any() and flags[5][10:].all()
    assert tr[5][3].shape[0] == 2 and tr[5][4][8] == 0 and tr[5][4][9] == 1     # the latch at block 9 applies to block 9
    b = Batch(utts)
    d = eng.denoiser(mode)
    for res, fill in ((b.run_dev(d), (SENT_I, SENT_F)), (b.run_host(d), (0, 0.0))):
        b.check(oracle, mode, res, fill[0], fill[1], "crossing")
        noise = res[3]
        assert not noise[0].any() and not noise[1].any() and not noise[3].any() and not noise[4].any()
        assert noise[2].max() > 100 and noise[5].max() > 100
    d.close()


# ---- 3. independence, bit for bit ------------------------------------------------------------------------------------
INDEP = [3, 150, 17, 40, 5, 64, 33, 9, 100, 12, 71, 28]


def assert_same(b1, res1, u1, b2, res2, u2, what):
    for a, c, name in zip(b1.utt_results(res1, u1), b2.utt_results(res2, u2), ("out", "precast", "flags", "noise_last")):
        assert np.array_equal(a, c, equal_nan=True), (what, name, u1)


@pytest.mark.parametrize("mode", [0, 1])
def test_an_utterance_does_not_depend_on_its_place_in_the_batch(eng, oracle, mode):
    utts = [speechlike(700 + u, n) for u, n in enumerate(INDEP)]
    d = eng.denoiser(mode)
    whole = Batch(utts)
    ref = whole.run_dev(d)
    whole.check(oracle, mode, ref, SENT_I, SENT_F, "in order")
    # a seeded permutation, with gaps
    perm = np.random.default_rng(3).permutation(len(utts))
    assert not np.array_equal(perm, np.arange(len(utts)))
    pb = Batch([utts[i] for i in perm], gap=6, lead=2)
    pres = pb.run_dev(d)
    for k, i in enumerate(perm):
        assert_same(whole, ref, int(i), pb, pres, k, "permuted")
    # two calls, split at utterance 5
    for lo, hi in ((0, 5), (5, len(utts))):
        part = Batch(utts[lo:hi])
        res = part.run_dev(d)
        for u in range(lo, hi):
            assert_same(whole, ref, u, part, res, u - lo, "split")
    # the host entry
    hres = whole.run_host(d)
    for u in range(len(utts)):
        a, c = whole.utt_results(ref, u), whole.utt_results(hres, u)
        nb = INDEP[u]
        assert np.array_equal(a[0][B:(nb - 1) * B], c[0][B:(nb - 1) * B]) and np.array_equal(a[1][B:(nb - 1) * B], c[1][B:(nb - 1) * B])
        assert np.array_equal(a[2], c[2]) and np.array_equal(a[3], c[3])
    # every launch geometry the entry honours: the blocks a wave of the run kernel walks
    for k in (1, 2, 4, 8):
        d.set_option("blocks_per_wave", k)
        res = whole.run_dev(d)
        for u in range(len(utts)):
            assert_same(whole, ref, u, whole, res, u, "blocks_per_wave %d" % k)
    d.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_the_handles_own_stream_is_left_alone(eng, mode):
    pcm = speechlike(31, 60)
    alone = eng.denoiser(mode)
    want = [alone.process(pcm[:25 * B], want_precast=True), alone.process(pcm[25 * B:], want_precast=True)]
    want_noise = alone.noise()
    alone.close()
    d = eng.denoiser(mode)
    got = [d.process(pcm[:25 * B], want_precast=True)]
    b = Batch([speechlike(32, 30), speechlike(33, 4)], gap=2)
    b.run_dev(d)
    b.run_host(d)
    got.append(d.process(pcm[25 * B:], want_precast=True))
    for (o, p), (wo, wp) in zip(got, want):
        assert np.array_equal(o, wo) and np.array_equal(p, wp)
    assert np.array_equal(d.noise(), want_noise)
    d.close()


# ---- 4. against the per-utterance handle loop ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_against_the_per_utterance_handle_loop(eng, oracle, mode):
    utts = [speechlike(800 + u, n) for u, n in enumerate([40, 3, 130, 17, 64])]
    b = Batch(utts, gap=2)
    d = eng.denoiser(mode)
    res = b.run_dev(d)
    for u, x in enumerate(utts):
        nb = x.size // B
        d.reset()
        h_out, h_pre = d.process(x, want_precast=True)
        h_flags = d.vad_trace(nb, flags_only=True)
        o, p, f, nz = b.utt_results(res, u)
        o_pre = trace_of(oracle, mode, x)[1]
        peak = max(np.abs(o_pre).max(), 1.0)
        assert np.abs(p[B:(nb - 1) * B] - h_pre).max() < TOL * peak, u
        assert np.abs(o[B:(nb - 1) * B].astype(np.int32) - h_out.astype(np.int32)).max() <= 1, u
        assert np.array_equal(f, h_flags), u
        assert np.abs(nz - d.noise()).max() <= TOL * max(d.noise().max(), 1.0), u
    d.close()


# ---- 5. plan and walk edges ------------------------------------------------------------------------------------------
def edge_batches():
    return {
        # one utterance of 130 blocks over the concatenated block indices 64 and 128 (the flag walk's 64-block words)
        "straddle": [speechlike(900, 30), speechlike(901, 130), speechlike(902, 7)],
        # more than 64 events: an all-quiet utterance of 200 blocks, between two others
        "events": [speechlike(903, 5), speechlike(904, 200, pattern=[200]), speechlike(905, 11)],
        # 300 utterances of three blocks: every wave of the run kernel crosses utterances
        "short": [speechlike(1000 + u, 3, pattern=[1 + u % 3, 1]) for u in range(300)],
    }


@pytest.mark.parametrize("which", ["straddle", "events", "short"])
@pytest.mark.parametrize("mode", [0, 1])
def test_plan_and_walk_edges(eng, oracle, mode, which):
    utts = edge_batches()[which]
    if which == "events":
        f = trace_of(oracle, mode, utts[1])[2]
        assert (f == 0).sum() > 150                                 # well over 64 events in one utterance
    b = Batch(utts)
    if which == "straddle":
        assert b.block_first[1] < 64 and b.block_first[2] > 128
    d = eng.denoiser(mode)
    b.check(oracle, mode, b.run_dev(d), SENT_I, SENT_F, which)
    d.close()


# ---- 6. mode 0: the frames FP32 cannot hold --------------------------------------------------------------------------
def test_frames_fp32_cannot_hold(eng, oracle):
    ci = [c["name"] for c in R.cases()].index("tone_bin64_1024")
    c = R.cases()[ci]
    whites = [w for w in R.WHITE_STREAMS if w[:3] in ((512, 140, 40), (512, 9, 130))]
    assert len(whites) == 2 and c["n_fft"] == 1024 and c["periodic"]
    utts = [R.white_pcm(whites[0]), c["pcm"], R.white_pcm(whites[1])]
    # on the CPU: the periodic case lists at least one frame, and the white neighbours' restated counts are the recorded ones
    t = R.trace(ci, 0)
    assert int((R.criterion(R.stream_frames(c["pcm"], B), R.frame_noise(t)) > R.RHO).sum()) >= 1
    for w, x in zip(whites, (utts[0], utts[2])):
        tw = trace_of(oracle, 0, x)
        rho = R.criterion(R.stream_frames(x, B), R.frame_noise(tw))
        assert (int((rho > R.RHO).sum()),) == w[4] and int((rho > R.RHO / 2).sum()) == w[5]
    b = Batch(utts, gap=2)
    d = eng.denoiser(0)
    res = b.run_dev(d)
    n_batch = d.frames_recomputed()
    b.check(oracle, 0, res, SENT_I, SENT_F, "periodic between white")
    n_loop = 0
    for u, x in enumerate(utts):
        nb = x.size // B
        o_pre = trace_of(oracle, 0, x)[1]
        check_blocks(b.utt_results(res, u)[1][B:(nb - 1) * B], o_pre, B, "utterance %d" % u)
        d.reset()
        d.process(x)
        n_loop += d.frames_recomputed()
    print("frames recomputed: %d in the batch, %d in the handle loop" % (n_batch, n_loop))
    assert n_batch == n_loop and n_batch >= 1
    b.run_dev(d)
    assert d.frames_recomputed() == n_batch                        # the batch call's count when it was the last call
    d.close()
    w = eng.denoiser(1)
    b.check(oracle, 1, b.run_dev(w), SENT_I, SENT_F, "Wiener on the same batch")
    assert w.frames_recomputed() == 0
    w.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------------
def test_errors(eng, oracle):
    import torch
    from jeicyboodsp_amd._lib import lib as L
    utts = [speechlike(40, 6), speechlike(41, 14), speechlike(42, 3)]
    b = Batch(utts, gap=2)
    d = eng.denoiser(0)
    out = np.zeros(b.n_samples, np.int16)
    good_s, good_b, n = b.sample_first, b.block_first, b.n_utts

    def host(h=d, s=good_s, f=good_b, n_utts=n, n_samples=b.n_samples):
        s, f = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(f, np.int64)
        return L.jdsp_denoise_batch(h._h, vp(b.pcm), n_samples, vp(s), vp(f), n_utts, vp(out), None, None, None)

    def poke(a, i, dlt):
        a = a.copy()
        a[i] += dlt
        return a

    def failed(rc, what):
        assert rc == -1, what
        msg = L.jdsp_last_error(eng._h)
        assert msg and b"jdsp_denoise_batch" in msg, what

    assert host() == 0
    small = eng.denoiser(0, 512, 256)
    failed(host(h=small), "a (512, 256) handle")
    failed(L.jdsp_denoise_batch_reserve(small._h, 10, 1), "a (512, 256) handle, reserve")
    assert small.process(np.zeros(4 * 256, np.int16)).size == 2 * 256      # still usable
    small.close()
    for what, kw in {
        "negative n_utts": dict(n_utts=-1),
        "an odd sample_first": dict(s=poke(good_s, 1, 1)),
        "overlapping spans": dict(s=poke(good_s, 1, -4)),
        "a decreasing block_first": dict(f=[0, 6, 4, 9]),
        "block_first[0] != 0": dict(f=good_b + 1),
        "a negative sample_first": dict(s=poke(good_s, 0, -2)),
        "a last span past n_samples": dict(n_samples=b.n_samples - 4),
    }.items():
        failed(host(**kw), what)
    # the device entry: base pointers, counts and the reservation -- offsets on the device are the caller's contract
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()           # noqa: E731
    d_pcm, d_s, d_b = t(b.pcm), t(good_s), t(good_b)
    d_o = torch.zeros(b.n_samples + 16, dtype=torch.int16, device="cuda")
    d_p = torch.zeros(b.n_samples + 16, dtype=torch.float32, device="cuda")

    def dev(h, pcm=vp(d_pcm), s=vp(d_s), f=vp(d_b), n_utts=n, n_total=b.n_total, o=vp(d_o), p=None):
        eng._use_torch_stream()
        return L.jdsp_denoise_batch_dev(h._h, pcm, s, f, n_utts, n_total, o, p, None, None)

    fresh = eng.denoiser(0)
    failed(dev(fresh), "a _dev call with nothing reserved")
    fresh.reserve_batch(b.n_total - 1, n)
    failed(dev(fresh), "a _dev call beyond the reserved blocks")
    fresh.reserve_batch(b.n_total, n - 1)
    failed(dev(fresh), "a _dev call beyond the reserved utterances")
    fresh.reserve_batch(b.n_total, n)
    assert dev(fresh) == 0
    for what, kw in {
        "pcm not 16-aligned": dict(pcm=vp(d_pcm, 4)), "out not 16-aligned": dict(o=vp(d_o, 4)),
        "precast not 8-aligned": dict(p=vp(d_p, 4)), "sample_first not 8-aligned": dict(s=vp(d_s, 4)),
        "block_first not 8-aligned": dict(f=vp(d_b, 4)), "negative n_utts": dict(n_utts=-1),
        "negative n_blocks_total": dict(n_total=-1),
    }.items():
        failed(dev(fresh, **kw), what)
    torch.cuda.synchronize()
    # the handles are still usable, for the batch and for their own stream
    for h in (d, fresh):
        b.check(oracle, 0, b.run_dev(h), SENT_I, SENT_F, "after the errors")
        o_out, o_pre, *_ = trace_of(oracle, 0, utts[1])
        got, pre = h.process(utts[1], want_precast=True)
        check_stream(got, pre, o_out, o_pre)
        h.close()
