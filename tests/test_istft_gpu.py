"""STFT synthesis (jdsp_istft, include/jdsp.h): the compiled reference's IFFTProcess, an FP64 numpy restatement of the
header's semantics (kept here), call cuts, round trips through the analysis, the pinned denoiser, Hermitian handling,
a full-size batch, sharding and the error paths."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

CONFIGS = [(1024, 1024), (1024, 512), (1024, 256), (512, 512), (512, 256), (512, 128)]
WINDOWS = ["none", "hamming", "hann"]


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


# ---- the restatement (FP64) ----------------------------------------------------------------------------------------
def window(kind, n):
    if kind == "none":
        return np.ones(n)
    a, b = (0.5, 0.5) if kind == "hann" else (0.54, 0.46)
    return a - b * np.cos(2 * 3.141592 * np.arange(n) / (n - 1))


def wola_den(n, hop, syn, ana):
    """sum_r w_a[i + r hop] w_s[i + r hop] (ones without an analysis window)"""
    if ana == "none":
        return np.ones(hop)
    p = window(ana, n) * window(syn, n)
    return p.reshape(n // hop, hop).sum(axis=0)


def hermitian(spec, n, layout):
    spec = np.asarray(spec, np.complex128)
    if layout == "full":
        x = spec[:, :n]
        return (x + np.conj(x[:, (-np.arange(n)) % n])) / 2
    x = spec[:, :n // 2 + 1].copy()
    x[:, 0] = x[:, 0].real
    x[:, n // 2] = x[:, n // 2].real
    return np.concatenate([x, np.conj(x[:, n // 2 - 1:0:-1])], axis=1)


def restate(spec, n, hop, layout="full", syn="none", ana="none"):
    """(emitted F*hop samples, tail n-hop samples, frame peak) in FP64"""
    h = hermitian(spec, n, layout)
    y = np.real(np.fft.ifft(h, axis=1)) * window(syn, n)
    F = y.shape[0]
    s = np.zeros(hop * F + n - hop)
    for f in range(F):
        s[hop * f: hop * f + n] += y[f]
    g = 1.0 / wola_den(n, hop, syn, ana)
    s *= np.resize(g, s.size)
    return s[:hop * F], s[hop * F:], (np.abs(y).max() if F else 0.0), g


def cast_i16(v):
    """oracle/jdsp_oracle.c cast_i16: truncate toward zero, low 16 bits"""
    return (np.trunc(np.asarray(v, np.float64)).astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)


def wrap_diff(a, b):
    return ((a.astype(np.int64) - b.astype(np.int64) + 32768) % 65536) - 32768


def rows(rng, F, n, pitch=None, scale=3000.0):
    pitch = pitch or n
    x = (rng.normal(size=(F, pitch)) + 1j * rng.normal(size=(F, pitch))) * scale * np.sqrt(n) / 2
    return x.astype(np.complex64)


def run(eng, spec, want_f32=True, **cfg):
    import torch
    ist = eng.istft(**cfg)
    t = torch.from_numpy(spec).cuda()
    o, f = ist.process(t, want_f32=True)
    to, tf = ist.flush(want_f32=True)
    torch.cuda.synchronize()
    ist.close()
    return o.cpu().numpy(), f.cpu().numpy(), to.cpu().numpy(), tf.cpu().numpy()


# ---- 1. the compiled reference itself ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 1024])
def test_pinned_to_reference_ifftprocess(eng, n):
    import oracle_lib
    ref = oracle_lib.load_ref(n)
    if ref is None:
        pytest.skip("oracle/_ref is absent")
    rng = np.random.default_rng(n)
    spec = rows(rng, 4, n)
    o, f, _, _ = run(eng, spec, n_fft=n, hop=n)
    for k in range(4):
        want = ref.ifft_process(spec[k].astype(np.complex128)).real
        err = np.abs(f[k * n:(k + 1) * n] - want).max() / np.abs(want).max()
        assert err < 1e-5, (k, err)


# ---- 2. the restatement over every configuration ------------------------------------------------------------------
def check_against_restatement(o, f, to, tf, spec, n, hop, layout, syn, ana):
    em, tail, peak, g = restate(spec, n, hop, layout, syn, ana)
    want = np.concatenate([em, tail])
    got_f = np.concatenate([f, tf]).astype(np.float64)
    got_i = np.concatenate([o, to])
    tol = 1e-5 * peak * np.resize(g, want.size)
    assert np.all(np.abs(got_f - want) <= tol), np.max(np.abs(got_f - want) / tol)
    assert np.array_equal(got_i, cast_i16(got_f.astype(np.float32)))            # the GPU's own float, bit for bit
    frac = np.abs(want - np.rint(want))
    clear = frac > 1e-3                                                         # away from integers (and wrap points)
    d = wrap_diff(got_i, cast_i16(want))
    assert np.all(np.abs(d[clear]) <= 1), np.abs(d[clear]).max()


@pytest.mark.parametrize("n,hop", CONFIGS)
@pytest.mark.parametrize("layout", ["full", "half"])
def test_against_restatement(eng, n, hop, layout):
    from jeicyboodsp_amd._lib import JdspError
    rng = np.random.default_rng(n + hop)
    F = 37
    pitch = n if layout == "full" else n // 2 + 1 + 3
    for syn in WINDOWS:
        for ana in WINDOWS:
            den = wola_den(n, hop, syn, ana)
            spec = rows(rng, F, n, pitch)
            if den.min() < 1e-6 * den.max():
                with pytest.raises(JdspError) as ei:
                    eng.istft(n_fft=n, hop=hop, layout=layout, synthesis_window=syn, analysis_window=ana)
                assert ei.value.code == -1
                continue
            o, f, to, tf = run(eng, spec, n_fft=n, hop=hop, layout=layout, synthesis_window=syn, analysis_window=ana)
            check_against_restatement(o, f, to, tf, spec, n, hop, layout, syn, ana)


@pytest.mark.parametrize("n,hop", [(1024, 512), (512, 128)])
@pytest.mark.parametrize("level", [40000.0, 100000.0])
def test_wrap_like_the_oracle_cast(eng, n, hop, level):
    rng = np.random.default_rng(int(level) + n)
    spec = rows(rng, 24, n, scale=level / 2)                    # pre-cast values well past +-32,768
    o, f, to, tf = run(eng, spec, n_fft=n, hop=hop)
    em, _, _, _ = restate(spec, n, hop)
    assert np.abs(em).max() > 32768 * 1.1
    check_against_restatement(o, f, to, tf, spec, n, hop, "full", "none", "none")


# ---- 3. call cuts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop", CONFIGS)
def test_call_cuts_bit_identical(eng, n, hop):
    import torch
    rng = np.random.default_rng(3 * n + hop)
    F = 61
    spec = torch.from_numpy(rows(rng, F, n)).cuda()
    ist = eng.istft(n_fft=n, hop=hop, synthesis_window="hann")
    o1, f1 = ist.process(spec, want_f32=True)
    t1, tf1 = ist.flush(want_f32=True)
    cuts = [0, 1, 0, 1, 1, 3, 7, 0, 2, 11, 5]
    cuts.append(F - sum(cuts))
    parts, fparts, j = [], [], 0
    for c in cuts:
        o, f = ist.process(spec[j:j + c], want_f32=True)
        parts.append(o.clone())
        fparts.append(f.clone())
        j += c
    t2, tf2 = ist.flush(want_f32=True)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(parts), o1) and torch.equal(torch.cat(fparts).view(torch.int32), f1.view(torch.int32))
    assert torch.equal(t1, t2) and torch.equal(tf1.view(torch.int32), tf2.view(torch.int32))
    ist.close()


@pytest.mark.parametrize("n,hop", CONFIGS)
def test_launch_geometry_bit_identical(eng, n, hop):
    """frames_per_wave changes the runs, the halos and which wave writes the tail -- never a bit of the output"""
    import torch
    from jeicyboodsp_amd._lib import JdspError
    R = n // hop
    rng = np.random.default_rng(5 * n + hop)
    F = 203
    spec = torch.from_numpy(rows(rng, F, n)).cuda()
    ist = eng.istft(n_fft=n, hop=hop, synthesis_window="hamming", analysis_window="hamming" if R > 1 else "none")
    got = []
    for fpw in (0, max(R - 1, 1), 4, 7, 22, 64, 1000):
        ist.set_option("frames_per_wave", fpw)
        o, f = ist.process(spec[:150], want_f32=True)
        o2, f2 = ist.process(spec[150:], want_f32=True)
        t = ist.flush()
        got.append((torch.cat([o, o2, t]), torch.cat([f, f2]).view(torch.int32)))
    torch.cuda.synchronize()
    for o, f in got[1:]:
        assert torch.equal(o, got[0][0]) and torch.equal(f, got[0][1])
    if R > 2:
        with pytest.raises(JdspError):
            ist.set_option("frames_per_wave", R - 2)
    with pytest.raises(JdspError):
        ist.set_option("no_such_option", 1)
    ist.close()


@pytest.mark.parametrize("n,hop,layout", [(1024, 256, "half"), (512, 128, "full")])
def test_short_calls_at_short_runs_bit_identical(eng, n, hop, layout):
    """Call cuts and launch geometry together: calls of 1, R - 2, R - 1 frames and the rest at runs of R - 1, R and 5
    frames -- a call shorter than the halo, a call that ends inside a wave's halo, and the tail written by a wave other
    than wave 0 -- against one call at the default geometry, bit for bit"""
    import torch
    R = n // hop
    F = 13
    rng = np.random.default_rng(7 * n + hop)
    pitch = n if layout == "full" else n // 2 + 1
    spec = torch.from_numpy(rows(rng, F, n, pitch)).cuda()
    ist = eng.istft(n_fft=n, hop=hop, layout=layout, synthesis_window="hann", analysis_window="hann")
    o1, f1 = ist.process(spec, want_f32=True)
    t1, tf1 = ist.flush(want_f32=True)
    cuts = [1, R - 2, R - 1]
    cuts.append(F - sum(cuts))
    for fpw in (R - 1, R, 5):
        ist.set_option("frames_per_wave", fpw)
        parts, fparts, j = [], [], 0
        for c in cuts:
            o, f = ist.process(spec[j:j + c], want_f32=True)
            parts.append(o.clone())
            fparts.append(f.clone())
            j += c
        t2, tf2 = ist.flush(want_f32=True)
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts), o1), fpw
        assert torch.equal(torch.cat(fparts).view(torch.int32), f1.view(torch.int32)), fpw
        assert torch.equal(t2, t1) and torch.equal(tf2.view(torch.int32), tf1.view(torch.int32)), fpw
    ist.close()


# ---- 4. round trip through the analysis ----------------------------------------------------------------------------
def pcm_of(rng, n, sigma=3000.0):
    return np.clip(np.rint(rng.normal(0, sigma, n)), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("n,hop", [(1024, 512), (1024, 256), (512, 256), (512, 128)])
@pytest.mark.parametrize("win", ["hamming", "hann"])
@pytest.mark.parametrize("syn", ["none", "same"])
def test_round_trip(eng, n, hop, win, syn):
    import torch
    rng = np.random.default_rng(n + hop)
    F = 50
    pcm = pcm_of(rng, hop * (F - 1) + n)
    eng.set_option("stft.window", 1 if win == "hann" else 0)
    try:
        spec = eng.stft(torch.from_numpy(pcm).cuda(), F, n, hop)
    finally:
        eng.set_option("stft.window", 0)
    ist = eng.istft(n_fft=n, hop=hop, synthesis_window=win if syn == "same" else "none", analysis_window=win)
    o, f = ist.process(spec, want_f32=True)
    torch.cuda.synchronize()
    ist.close()
    o, f = o.cpu().numpy()[n - hop:], f.cpu().numpy()[n - hop:]
    want = pcm[n - hop:F * hop]
    assert np.abs(f - want).max() <= 1e-5 * np.abs(pcm).max()
    assert np.abs(o.astype(np.int32) - want).max() <= 1


@pytest.mark.parametrize("pitch", [513, 576])
def test_round_trip_half_spectrum(eng, pitch):
    import torch
    rng = np.random.default_rng(pitch)
    F = 40
    pcm = pcm_of(rng, 512 * (F + 1))
    spec = eng.stft_half(torch.from_numpy(pcm).cuda(), F, pitch=pitch)
    ist = eng.istft(n_fft=1024, hop=512, layout="half", analysis_window="hamming")
    o, f = ist.process(spec, want_f32=True)
    torch.cuda.synchronize()
    ist.close()
    o, f = o.cpu().numpy()[512:], f.cpu().numpy()[512:]
    want = pcm[512:F * 512]
    assert np.abs(f - want).max() <= 1e-5 * np.abs(pcm).max()
    assert np.abs(o.astype(np.int32) - want).max() <= 1


# ---- 5. the pinned denoiser ---------------------------------------------------------------------------------------
def test_matches_denoiser_on_a_loud_stream(eng, oracle):
    import torch
    rng = np.random.default_rng(5)
    nb = 40
    x = pcm_of(rng, nb * 512)                      # energy far above 700 in every block: the estimate stays zero
    d = eng.denoiser(0)
    den = d.process(x)
    d.close()
    o_den, _ = oracle.denoise_stream(0, x)
    assert den.size == o_den.size == (nb - 2) * 512
    # alignment (SS:211-216, 260-263): the first call only stashes its block, frame f = blocks [f, f + 1] is emitted by
    # call f + 1, and calls 1 and 2 emit nothing -- so the denoiser's output is frames 1.. of the synthesis
    F = nb - 1
    spec = eng.stft(torch.from_numpy(x).cuda(), F, 1024, 512)
    ist = eng.istft(n_fft=1024, hop=512)
    o = ist.process(spec).cpu().numpy()
    ist.close()
    assert np.abs(o[512:512 + den.size].astype(np.int32) - den).max() <= 1
    assert np.abs(o[512:512 + den.size].astype(np.int32) - o_den).max() <= 1


# ---- 6. Hermitian semantics ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 1024])
def test_hermitian_semantics(eng, n):
    rng = np.random.default_rng(6 + n)
    spec = rows(rng, 9, n)
    mirror = np.conj(spec[:, (-np.arange(n)) % n])
    sym = np.empty_like(spec)
    sym.real = np.float32(0.5) * (spec.real + mirror.real)
    sym.imag = np.float32(0.5) * (spec.imag + mirror.imag)
    a = run(eng, spec, n_fft=n, hop=n // 2)
    b = run(eng, sym, n_fft=n, hop=n // 2)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.int16 if u.dtype == np.int16 else np.int32),
                              v.view(np.int16 if v.dtype == np.int16 else np.int32))
    half = np.ascontiguousarray(spec[:, :n // 2 + 1])
    poked = half.copy()
    poked[:, 0] += 1j * 1234.5
    poked[:, n // 2] -= 1j * 777.0
    a = run(eng, half, n_fft=n, hop=n // 2, layout="half")
    b = run(eng, poked, n_fft=n, hop=n // 2, layout="half")
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


# ---- 7. full size --------------------------------------------------------------------------------------------------
def test_full_size_65536_frames(eng):
    import torch
    F, n, hop = 65536, 1024, 512
    gen = torch.Generator(device="cuda").manual_seed(7)
    spec = torch.randn((F, n), dtype=torch.complex64, device="cuda", generator=gen) * 3000.0 * np.sqrt(n)
    ist = eng.istft(n_fft=n, hop=hop)
    o, f = ist.process(spec, want_f32=True)
    torch.cuda.synchronize()
    assert o.numel() == F * hop and bool(torch.isfinite(f).all())
    for fr in range(1, F, 97):
        pair = spec[fr - 1:fr + 1].cpu().numpy()
        em, _, peak, _ = restate(pair, n, hop)
        got = f[fr * hop:(fr + 1) * hop].cpu().numpy().astype(np.float64)
        assert np.abs(got - em[hop:]).max() <= 1e-5 * peak, fr
    ist.close()


# ---- 8. sharding ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop", [(1024, 512), (1024, 256), (512, 128)])
def test_sharded_equals_single_call(eng, n, hop):
    import torch
    from jeicyboodsp_amd import sharding
    rng = np.random.default_rng(8 + hop)
    F = 101
    spec = torch.from_numpy(rows(rng, F, n)).cuda()
    ist = eng.istft(n_fft=n, hop=hop, synthesis_window="hamming", analysis_window="hamming")
    o1, f1 = ist.process(spec, want_f32=True)
    t1 = ist.flush()
    for world in (2, 3, 8):
        parts, fparts = [], []
        for rank in range(world):
            r = sharding.istft_sharded(ist, spec, F, world, rank, want_f32=True)
            if r is not None:
                parts.append(r[0].clone())
                fparts.append(r[1].clone())
        t2 = ist.flush()                       # the last rank's handle holds the stream's tail
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts), o1), world
        assert torch.equal(torch.cat(fparts).view(torch.int32), f1.view(torch.int32)), world
        assert torch.equal(t1, t2), world
    ist.close()


# ---- 9. errors -----------------------------------------------------------------------------------------------------
def test_errors(eng):
    import ctypes as C
    import torch
    from jeicyboodsp_amd._lib import JdspError, lib as L
    for bad in (dict(n_fft=2048, hop=1024), dict(n_fft=1024, hop=384), dict(n_fft=512, hop=64), dict(n_fft=1024, hop=0),
                dict(layout=2), dict(synthesis_window=2), dict(analysis_window=-2),
                dict(n_fft=1024, hop=1024, synthesis_window="hann", analysis_window="hann")):
        with pytest.raises(JdspError) as ei:
            eng.istft(**bad)
        assert ei.value.code == -1, bad
    ist = eng.istft(n_fft=1024, hop=512, layout="half")
    spec = torch.zeros((4, 600), dtype=torch.complex64, device="cuda")
    out = torch.zeros(4 * 512 + 8, dtype=torch.int16, device="cuda")
    f32 = torch.zeros(4 * 512 + 8, dtype=torch.float32, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    assert L.jdsp_istft_process_dev(ist._h, p(spec), 512, 4, p(out), None) == -1            # pitch below 513
    assert L.jdsp_istft_process_dev(ist._h, p(spec, 4), 600, 3, p(out), None) == -1        # spectrum not 8-aligned
    assert L.jdsp_istft_process_dev(ist._h, p(spec), 600, 4, p(out, 2), None) == -1         # int16 out not 4-aligned
    assert L.jdsp_istft_process_dev(ist._h, p(spec), 600, 4, None, p(f32, 4)) == -1         # float out not 8-aligned
    assert L.jdsp_istft_process_dev(ist._h, None, 600, 0, None, None) == 0                  # zero frames
    assert L.jdsp_istft_process_dev(ist._h, p(spec), 600, -1, None, None) == -1
    assert L.jdsp_istft_samples_out(ist._h, 7) == 7 * 512
    ist.close()
    full = eng.istft(n_fft=512, hop=256)
    assert L.jdsp_istft_process_dev(full._h, p(spec), 511, 1, None, None) == -1             # FULL: pitch below n_fft
    full.close()
    # two handles stay independent
    rng = np.random.default_rng(9)
    a_spec = torch.from_numpy(rows(rng, 12, 1024)).cuda()
    b_spec = torch.from_numpy(rows(rng, 12, 1024)).cuda()
    alone = eng.istft(n_fft=1024, hop=256)
    ra = torch.cat([alone.process(a_spec[:5]), alone.process(a_spec[5:]), alone.flush()])
    alone.reset()
    rb = torch.cat([alone.process(b_spec), alone.flush()])
    ha, hb = eng.istft(n_fft=1024, hop=256), eng.istft(n_fft=1024, hop=256)
    xa = [ha.process(a_spec[:5])]
    xb = [hb.process(b_spec[:7])]
    xa.append(ha.process(a_spec[5:]))
    xb.append(hb.process(b_spec[7:]))
    xa.append(ha.flush())
    xb.append(hb.flush())
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(xa), ra) and torch.equal(torch.cat(xb), rb)
    for h in (alone, ha, hb):
        h.close()


def test_host_path_matches_device_path(eng):
    import torch
    rng = np.random.default_rng(10)
    spec = rows(rng, 20, 1024, pitch=520)
    ist = eng.istft(n_fft=1024, hop=512, layout="half", synthesis_window="hann")
    oh, fh = ist.process(spec, want_f32=True)
    th = ist.flush()
    od, fd = ist.process(torch.from_numpy(spec).cuda(), want_f32=True)
    td = ist.flush()
    assert np.array_equal(oh, od.cpu().numpy()) and np.array_equal(fh, fd.cpu().numpy()) and np.array_equal(th, td.cpu().numpy())
    ist.close()
    # the host entries' device buffers: one stream in calls of 5 frames (sizes them), 20 (exceeds them) and 3 (reuses
    # them) on a fresh handle, against the device path's single call
    ist = eng.istft(n_fft=1024, hop=512, layout="half", synthesis_window="hann")
    spec = rows(rng, 28, 1024, pitch=520)
    od, fd = ist.process(torch.from_numpy(spec).cuda(), want_f32=True)
    td = ist.flush()
    od, fd, td = od.cpu().numpy(), fd.cpu().numpy(), td.cpu().numpy()
    parts = [ist.process(spec[a:b], want_f32=True) for a, b in ((0, 5), (5, 25), (25, 28))]
    assert np.array_equal(np.concatenate([o for o, _ in parts]), od)
    assert np.array_equal(np.concatenate([f for _, f in parts]), fd)
    ist.reset()                              # after growth: the partial sums are gone, the stream replays in one call
    oh, fh = ist.process(spec, want_f32=True)
    assert np.array_equal(oh, od) and np.array_equal(fh, fd) and np.array_equal(ist.flush(), td)
    ist.close()
    eng.istft(n_fft=1024, hop=512, layout="half", synthesis_window="hann").close()     # after a grown handle is gone
