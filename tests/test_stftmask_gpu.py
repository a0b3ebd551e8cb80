"""Fused STFT masking (jdsp_stftmask, include/jdsp.h): an FP64 numpy restatement of the header's semantics (kept
here), the unfused composition stft -> multiply -> istft on the GPU, the pinned denoiser at a zero noise estimate,
bit-identity across call cuts, launch geometries and shards, the mask pitch rules, host against device, and the
error paths.

test_against_restatement prints |float32 - restatement| / (1e-5 P g) per case and the worst of each grid cell (run with
-s); the project's other FP32 outputs sit near 0.05 of that bar."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

N = 1024
BINS = N // 2 + 1
HOPS = [1024, 512, 256]
KINDS = ["real", "complex"]
# (analysis, synthesis, normalise)
COMBOS = [("hann", "hann", 1), ("hamming", "none", 0), ("none", "hamming", 1)]
LIMIT = 30000.0                  # no comparison near an int16 wrap point


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


# ---- the restatement (FP64) ----------------------------------------------------------------------------------------
def window(kind, n=N):
    if kind == "none":
        return np.ones(n)
    a, b = (0.5, 0.5) if kind == "hann" else (0.54, 0.46)
    return a - b * np.cos(2 * 3.141592 * np.arange(n) / (n - 1))


def gain(hop, ana, syn, normalise):
    if not normalise:
        return np.ones(hop)
    return 1.0 / (window(ana) * window(syn)).reshape(N // hop, hop).sum(axis=0)


def invertible(hop, combo):
    """jdsp_istft_create's rule: no entry of the WOLA sum below 1e-6 of its largest"""
    ana, syn, norm = combo
    den = (window(ana) * window(syn)).reshape(N // hop, hop).sum(axis=0)
    return not norm or den.min() >= 1e-6 * den.max()


def expect_rejected(eng, hop, kind, combo):
    from jeicyboodsp_amd._lib import JdspError
    with pytest.raises(JdspError) as ei:
        eng.stft_mask(**cfg_of(hop, kind, combo))
    assert ei.value.code == -1


def stream_combo(hop):
    """Hann / Hann with normalisation where it has an inverse (R > 1); at R = 1 a synthesis window alone (a gain of
    1 / (w_a w_s) would blow the frame edges of a masked signal past the int16 range)"""
    return ("hann", "hann", 1) if hop < N else ("none", "hamming", 1)


def restate(pcm, mask, F, hop, ana, syn, normalise):
    """Steps 1-5 of the header: (emitted F*hop samples, tail N-hop samples, peak P of the un-normalised overlap-added
    signal, gain g[hop]) in FP64.  mask: [F, >= BINS] rows or one row [>= BINS]."""
    pcm = np.asarray(pcm, np.float64)
    frames = np.stack([pcm[hop * f: hop * f + N] for f in range(F)]) * window(ana)
    X = np.fft.fft(frames, axis=1)[:, :BINS]
    M = np.asarray(mask, np.complex128)
    M = M[None, :BINS] if M.ndim == 1 else M[:F, :BINS]
    Y = M * X
    Y[:, 0] = (M[:, 0].real * X[:, 0]).real                    # Im of M[0], M[n/2] ignored; the frame is real
    Y[:, N // 2] = (M[:, N // 2].real * X[:, N // 2]).real
    H = np.concatenate([Y, np.conj(Y[:, N // 2 - 1:0:-1])], axis=1)
    y = np.real(np.fft.ifft(H, axis=1)) * window(syn)
    s = np.zeros(hop * F + N - hop)
    for f in range(F):
        s[hop * f: hop * f + N] += y[f]
    P = np.abs(s).max()
    g = gain(hop, ana, syn, normalise)
    s = s * np.resize(g, s.size)
    assert np.abs(s).max() < LIMIT, np.abs(s).max()
    return s[:hop * F], s[hop * F:], P, g


def cast_i16(v):
    """oracle/jdsp_oracle.c cast_i16: truncate toward zero, low 16 bits"""
    return (np.trunc(np.asarray(v, np.float64)).astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)


def pcm_of(rng, F, hop, sigma=3000.0):
    return np.clip(np.rint(rng.normal(0, sigma, hop * (F - 1) + N)), -32768, 32767).astype(np.int16)


def mask_of(rng, kind, F, pitch=BINS):
    """real: uniform in [0, 1.5); complex: |M| < 1.5, random phase.  F = None: one row."""
    shape = (pitch,) if F is None else (F, pitch)
    mag = rng.uniform(0.0, 1.5, shape)
    if kind == "real":
        return np.minimum(mag.astype(np.float32), np.float32(1.4999999))
    m = (mag * 0.9999 * np.exp(2j * np.pi * rng.uniform(size=shape))).astype(np.complex64)
    assert np.abs(m).max() < 1.5
    return m


def cfg_of(hop, kind, combo):
    ana, syn, norm = combo
    return dict(n_fft=N, hop=hop, analysis_window=ana, synthesis_window=syn, normalise=norm, mask_kind=kind)


def run(eng, pcm, mask, F, fpw=0, **cfg):
    """one call + flush on the device path -> (int16, float32, int16 tail, float32 tail) as numpy"""
    import torch
    sm = eng.stft_mask(**cfg)
    sm.set_option("frames_per_wave", fpw)
    o, f = sm.process(torch.from_numpy(pcm).cuda(), torch.from_numpy(mask).cuda(), F, want_f32=True)
    to, tf = sm.flush(want_f32=True)
    torch.cuda.synchronize()
    sm.close()
    return o.cpu().numpy(), f.cpu().numpy(), to.cpu().numpy(), tf.cpu().numpy()


def bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ---- 1. the restatement over the grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "%s-%s-%d" % c)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", HOPS)
def test_against_restatement(eng, hop, kind, combo):
    R = N // hop
    if not invertible(hop, combo):                                 # Hann / Hann at R = 1
        return expect_rejected(eng, hop, kind, combo)
    worst = 0.0
    for F in sorted({1, 2, R, 37}):
        rng = np.random.default_rng(1000 * hop + 10 * F + len(kind))
        pcm, mask = pcm_of(rng, F, hop), mask_of(rng, kind, F)
        em, tail, P, g = restate(pcm, mask, F, hop, *combo)
        want = np.concatenate([em, tail])
        tol = 1e-5 * P * np.resize(g, want.size)
        for fpw in sorted({max(R - 1, 1), 3, 7}):
            o, f, to, tf = run(eng, pcm, mask, F, fpw, **cfg_of(hop, kind, combo))
            got_f = np.concatenate([f, tf]).astype(np.float64)
            got_i = np.concatenate([o, to])
            ratio = float(np.max(np.abs(got_f - want) / tol))
            worst = max(worst, ratio)
            print("stftmask hop %d %s %s F %d fpw %d: max |err| / (1e-5 P g) = %.4f" % (hop, kind, combo, F, fpw, ratio))
            assert np.all(np.abs(got_f - want) <= tol), (F, fpw, ratio)
            assert np.array_equal(got_i, cast_i16(got_f.astype(np.float32))), (F, fpw)   # the GPU's own float, bit for bit
            d = got_i.astype(np.int64) - cast_i16(want).astype(np.int64)
            assert np.all(np.abs(d) <= 1), (F, fpw, np.abs(d).max())                   # every sample, no exclusions
    print("stftmask hop %d %s %s: worst ratio %.4f" % (hop, kind, combo, worst))


# ---- 2. the unfused composition on the GPU -------------------------------------------------------------------------
@pytest.mark.parametrize("combo", [("hann", "hann", 1), ("hamming", "none", 0)], ids=lambda c: "%s-%s-%d" % c)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", HOPS)
def test_against_unfused_composition(eng, hop, kind, combo):
    import torch
    ana, syn, norm = combo
    if not invertible(hop, combo):
        return expect_rejected(eng, hop, kind, combo)
    F = 37
    rng = np.random.default_rng(2000 + hop + len(kind))
    pcm, mask = pcm_of(rng, F, hop), mask_of(rng, kind, F)
    _, _, P, g = restate(pcm, mask, F, hop, *combo)
    o, f, to, tf = run(eng, pcm, mask, F, **cfg_of(hop, kind, combo))
    m = mask.astype(np.complex64)
    m[:, 0] = m[:, 0].real                                         # Im of M[0], M[n/2] is ignored by definition
    m[:, N // 2] = m[:, N // 2].real
    half = hop == 512 and ana == "hamming"                        # the half-spectrum analysis is Hamming at hop 512
    d_pcm = torch.from_numpy(pcm).cuda()
    if half:
        spec = eng.stft_half(d_pcm, F, pitch=BINS)
        spec *= torch.from_numpy(m).cuda()
    else:
        eng.set_option("stft.window", 1 if ana == "hann" else 0)
        try:
            spec = eng.stft(d_pcm, F, N, hop)
        finally:
            eng.set_option("stft.window", 0)
        full = np.concatenate([m, np.conj(m[:, N // 2 - 1:0:-1])], axis=1)
        spec *= torch.from_numpy(full).cuda()
    ist = eng.istft(n_fft=N, hop=hop, layout="half" if half else "full", synthesis_window=syn,
                    analysis_window=ana if norm else "none")
    uo, uf = ist.process(spec, want_f32=True)
    uto, utf = ist.flush(want_f32=True)
    torch.cuda.synchronize()
    ist.close()
    want_f = np.concatenate([uf.cpu().numpy(), utf.cpu().numpy()]).astype(np.float64)
    want_i = np.concatenate([uo.cpu().numpy(), uto.cpu().numpy()]).astype(np.int64)
    got_f = np.concatenate([f, tf]).astype(np.float64)
    got_i = np.concatenate([o, to]).astype(np.int64)
    tol = 2e-5 * P * np.resize(g, got_f.size)                      # both sides within 1e-5 P g of the same truth
    ratio = float(np.max(np.abs(got_f - want_f) / tol))
    print("stftmask vs unfused hop %d %s %s: max |diff| / (2e-5 P g) = %.4f" % (hop, kind, combo, ratio))
    assert np.all(np.abs(got_f - want_f) <= tol), ratio
    assert np.abs(got_i - want_i).max() <= 1


# ---- 3. the denoiser at a zero noise estimate ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_matches_denoiser_on_a_loud_stream(eng, kind):
    import torch
    rng = np.random.default_rng(5)
    nb = 40
    x = np.clip(np.rint(rng.normal(0, 3000.0, nb * 512)), -32768, 32767).astype(np.int16)
    d = eng.denoiser(0)
    den = d.apply(x, np.zeros(N))
    d.close()
    assert den.size == (nb - 2) * 512
    # alignment as tests/test_istft_gpu.py::test_matches_denoiser_on_a_loud_stream: frame f = blocks [f, f + 1], the
    # denoiser's output is frames 1.. of the synthesis
    F = nb - 1
    ones = np.ones(BINS, np.float32 if kind == "real" else np.complex64)
    em, _, _, _ = restate(x, ones, F, 512, "hamming", "none", 0)
    sm = eng.stft_mask(n_fft=N, hop=512, analysis_window="hamming", synthesis_window="none", normalise=0, mask_kind=kind)
    o = sm.process(torch.from_numpy(x).cuda(), torch.from_numpy(ones).cuda(), F).cpu().numpy()
    sm.close()
    assert np.abs(o[512:512 + den.size].astype(np.int32) - den).max() <= 1


# ---- 4. bit-identity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", HOPS)
def test_cuts_geometries_and_shards_bit_identical(eng, hop, kind):
    import torch
    from jeicyboodsp_amd import sharding
    R = N // hop
    F = 61
    rng = np.random.default_rng(4000 + hop + len(kind))
    h_pcm, h_mask = pcm_of(rng, F, hop), mask_of(rng, kind, F, pitch=BINS + 3)
    restate(h_pcm, h_mask, F, hop, *stream_combo(hop))             # the magnitude guard
    pcm, mask = torch.from_numpy(h_pcm).cuda(), torch.from_numpy(h_mask).cuda()
    sm = eng.stft_mask(**cfg_of(hop, kind, stream_combo(hop)))
    o1, f1 = sm.process(pcm, mask, F, want_f32=True)
    t1, tf1 = sm.flush(want_f32=True)

    def same(parts, fparts, t2, tf2, what):
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts), o1), what
        assert torch.equal(bits(torch.cat(fparts)), bits(f1)), what
        assert torch.equal(t2, t1) and torch.equal(bits(tf2), bits(tf1)), what

    # one stream cut into calls at arbitrary frame counts; the caller presents the overlap again
    cuts = [1, 0, 1, 1, 3, 7, 0, 2, 11, 5]
    cuts.append(F - sum(cuts))
    parts, fparts, j = [], [], 0
    for c in cuts:
        o, f = sm.process(pcm[hop * j:], mask[j:j + c], c, want_f32=True)
        parts.append(o.clone())
        fparts.append(f.clone())
        j += c
    same(parts, fparts, *sm.flush(want_f32=True), what=("cuts", cuts))
    # every launch geometry
    for fpw in sorted({max(R - 1, 1), 3, 7}):
        sm.set_option("frames_per_wave", fpw)
        o, f = sm.process(pcm, mask, F, want_f32=True)
        same([o], [f], *sm.flush(want_f32=True), what=("frames_per_wave", fpw))
    sm.set_option("frames_per_wave", 0)
    # shards
    for world in (1, 2, 3, 8):
        parts, fparts = [], []
        for rank in range(world):
            r = sharding.stftmask_sharded(sm, pcm, mask, F, world, rank, want_f32=True)
            if r is not None:
                parts.append(r[0].clone())
                fparts.append(r[1].clone())
        same(parts, fparts, *sm.flush(want_f32=True), what=("world", world))   # the last rank holds the stream's tail
    sm.close()


@pytest.mark.parametrize("kind", KINDS)
def test_short_calls_at_short_runs_bit_identical(eng, kind):
    """Call cuts and launch geometry together at hop 256 (R = 4): calls of 1, R - 2, R - 1 frames and the rest at runs of
    R - 1, R and 5 frames -- a call shorter than the halo, a call that ends inside a wave's halo, and the tail written by
    a wave other than wave 0 -- against one call at the default geometry, bit for bit"""
    import torch
    hop = 256
    R = N // hop
    F = 13
    rng = np.random.default_rng(4100 + len(kind))
    h_pcm, h_mask = pcm_of(rng, F, hop), mask_of(rng, kind, F)
    restate(h_pcm, h_mask, F, hop, *stream_combo(hop))             # the magnitude guard
    pcm, mask = torch.from_numpy(h_pcm).cuda(), torch.from_numpy(h_mask).cuda()
    sm = eng.stft_mask(**cfg_of(hop, kind, stream_combo(hop)))
    o1, f1 = sm.process(pcm, mask, F, want_f32=True)
    t1, tf1 = sm.flush(want_f32=True)
    cuts = [1, R - 2, R - 1]
    cuts.append(F - sum(cuts))
    for fpw in (R - 1, R, 5):
        sm.set_option("frames_per_wave", fpw)
        parts, fparts, j = [], [], 0
        for c in cuts:
            o, f = sm.process(pcm[hop * j:], mask[j:j + c], c, want_f32=True)
            parts.append(o.clone())
            fparts.append(f.clone())
            j += c
        t2, tf2 = sm.flush(want_f32=True)
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts), o1), fpw
        assert torch.equal(bits(torch.cat(fparts)), bits(f1)), fpw
        assert torch.equal(t2, t1) and torch.equal(bits(tf2), bits(tf1)), fpw
    sm.close()


# ---- 5. mask pitch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", HOPS)
def test_mask_pitch(eng, hop, kind):
    F = 23
    rng = np.random.default_rng(5000 + hop + len(kind))
    pcm = pcm_of(rng, F, hop)
    combo = ("hamming", "hamming", 1) if hop < N else ("none", "hamming", 1)
    cfg = cfg_of(hop, kind, combo)
    # pitch 0 = the same row at every frame
    row = mask_of(rng, kind, None)
    restate(pcm, row, F, hop, *combo)
    a = run(eng, pcm, row, F, **cfg)
    b = run(eng, pcm, np.ascontiguousarray(np.broadcast_to(row, (F, BINS))), F, **cfg)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u,
                              v.view(np.int32) if v.dtype == np.float32 else v)
    # a padded pitch = the dense one
    dense = mask_of(rng, kind, F)
    _, _, P, g = restate(pcm, dense, F, hop, *combo)
    padded = np.full((F, 520), 99, dense.dtype)
    padded[:, :BINS] = dense
    a = run(eng, pcm, dense, F, **cfg)
    b = run(eng, pcm, padded, F, **cfg)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u,
                              v.view(np.int32) if v.dtype == np.float32 else v)
    if kind == "real":
        # a REAL mask = the COMPLEX mask with zero imaginary parts, within the bar
        c = run(eng, pcm, dense.astype(np.complex64), F, **cfg_of(hop, "complex", combo))
        got = np.concatenate([a[1], a[3]]).astype(np.float64)
        other = np.concatenate([c[1], c[3]]).astype(np.float64)
        assert np.all(np.abs(got - other) <= 1e-5 * P * np.resize(g, got.size))
        assert np.abs(np.concatenate([a[0], a[2]]).astype(np.int64) - np.concatenate([c[0], c[2]])).max() <= 1
    else:
        # the imaginary parts of M[0] and M[n/2] do not change a bit
        poked = dense.copy()
        poked[:, 0] += 1j * 0.7
        poked[:, N // 2] -= 1j * 1.1
        c = run(eng, pcm, poked, F, **cfg)
        for u, v in zip(a, c):
            assert np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u,
                                  v.view(np.int32) if v.dtype == np.float32 else v)


# ---- 6. host and device --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", HOPS)
def test_host_path_and_null_outputs(eng, hop, kind):
    import torch
    F = 20
    rng = np.random.default_rng(6000 + hop + len(kind))
    pcm, mask = pcm_of(rng, F, hop), mask_of(rng, kind, F, pitch=520)
    restate(pcm, mask, F, hop, *stream_combo(hop))
    sm = eng.stft_mask(**cfg_of(hop, kind, stream_combo(hop)))
    oh, fh = sm.process(pcm, mask, F, want_f32=True)
    th, tfh = sm.flush(want_f32=True)
    d_pcm, d_mask = torch.from_numpy(pcm).cuda(), torch.from_numpy(mask).cuda()
    od, fd = sm.process(d_pcm, d_mask, F, want_f32=True)
    td, tfd = sm.flush(want_f32=True)
    assert np.array_equal(oh, od.cpu().numpy()) and np.array_equal(th, td.cpu().numpy())
    assert np.array_equal(fh.view(np.int32), fd.cpu().numpy().view(np.int32))
    assert np.array_equal(tfh.view(np.int32), tfd.cpu().numpy().view(np.int32))
    # both outputs NULL: the stream advances, and what follows matches the uncut run -- on both paths
    k = 7
    assert sm.process(d_pcm, d_mask[:k], k, write=False) is None
    o2, f2 = sm.process(d_pcm[hop * k:], d_mask[k:], F - k, want_f32=True)
    t2 = sm.flush()
    assert torch.equal(o2, od[hop * k:]) and torch.equal(bits(f2), bits(fd[hop * k:])) and torch.equal(t2, td)
    assert sm.process(pcm, mask[:k], k, write=False) is None
    o3 = sm.process(pcm[hop * k:], mask[k:], F - k)
    t3 = sm.flush()
    assert np.array_equal(o3, oh[hop * k:]) and np.array_equal(t3, th)
    sm.close()
    # the host entries' device buffers: one stream in calls of 5 frames (sizes them), 20 (exceeds them) and 3 (reuses
    # them) on a fresh handle, against the device path's single call
    F = 28
    pcm, mask = pcm_of(rng, F, hop), mask_of(rng, kind, F, pitch=520)
    sm = eng.stft_mask(**cfg_of(hop, kind, stream_combo(hop)))
    od, fd = sm.process(torch.from_numpy(pcm).cuda(), torch.from_numpy(mask).cuda(), F, want_f32=True)
    td = sm.flush()
    od, fd, td = od.cpu().numpy(), fd.cpu().numpy(), td.cpu().numpy()
    parts = [sm.process(pcm[hop * a:], mask[a:b], b - a, want_f32=True) for a, b in ((0, 5), (5, 25), (25, 28))]
    assert np.array_equal(np.concatenate([o for o, _ in parts]), od)
    assert np.array_equal(np.concatenate([f for _, f in parts]).view(np.int32), fd.view(np.int32))
    sm.reset()                               # after growth: the partial sums are gone, the stream replays in one call
    oh, fh = sm.process(pcm, mask, F, want_f32=True)
    assert np.array_equal(oh, od) and np.array_equal(fh.view(np.int32), fd.view(np.int32))
    assert np.array_equal(sm.flush(), td)
    sm.close()
    eng.stft_mask(**cfg_of(hop, kind, stream_combo(hop))).close()      # after a grown handle is gone


# ---- 7. errors -----------------------------------------------------------------------------------------------------
def test_errors(eng):
    import ctypes as C
    import torch
    from jeicyboodsp_amd._lib import JdspError, lib as L
    for bad in (dict(n_fft=512, hop=256), dict(n_fft=1024, hop=128), dict(analysis_window=2), dict(synthesis_window=-2),
                dict(mask_kind=2), dict(n_fft=1024, hop=1024, analysis_window="hann", synthesis_window="none", normalise=1)):
        with pytest.raises(JdspError) as ei:
            eng.stft_mask(**bad)
        assert ei.value.code == -1, bad
        assert L.jdsp_last_error(eng._h), bad
    F = 4
    pcm = torch.zeros(512 * (F + 1) + 8, dtype=torch.int16, device="cuda")
    out = torch.zeros(F * 512 + 8, dtype=torch.int16, device="cuda")
    f32 = torch.zeros(F * 512 + 8, dtype=torch.float32, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    for kind, dtype, elem in (("real", torch.float32, 4), ("complex", torch.complex64, 8)):
        sm = eng.stft_mask(n_fft=1024, hop=512, mask_kind=kind)
        mask = torch.ones((F + 1, 520), dtype=dtype, device="cuda")
        call = lambda *a: L.jdsp_stftmask_process_dev(sm._h, *a)  # noqa: E731
        for pitch in (1, 256, 512):
            assert call(p(pcm), p(mask), pitch, F, p(out), None) == -1                   # a pitch in 1..n/2
        assert call(p(pcm, 2), p(mask), 520, F, p(out), None) == -1                       # pcm not 4-aligned
        assert call(p(pcm), p(mask, elem // 2), 520, F, p(out), None) == -1               # mask not element-aligned
        assert call(p(pcm), p(mask), 520, F, p(out, 2), None) == -1                       # int16 out not 4-aligned
        assert call(p(pcm), p(mask), 520, F, None, p(f32, 4)) == -1                       # float out not 8-aligned
        assert call(p(pcm), p(mask), 520, -1, p(out), None) == -1                         # negative n_frames
        assert b"jdsp_stftmask" in L.jdsp_last_error(eng._h)
        assert call(None, None, 520, 0, None, None) == 0                                  # zero frames
        assert L.jdsp_stftmask_flush_dev(sm._h, p(out, 2), None) == -1
        assert L.jdsp_stftmask_samples_out(sm._h, 7) == 7 * 512
        with pytest.raises(JdspError):
            sm.set_option("no_such_option", 1)
        # the handle is still usable, and nothing of the above advanced its stream
        o = sm.process(pcm[:512 * (F + 1)], mask[:F], F)
        t = sm.flush()
        torch.cuda.synchronize()
        assert o.numel() == F * 512 and t.numel() == 512 and not bool(o.any()) and not bool(t.any())
        sm.close()
