"""GPU parity: every launch geometry of the STFT analysis kernels against the CPU oracle.

The analysis kernels take their geometry from the batch size, the CU count, the pointer alignment, the hop and the
"stft.*" options of jdsp_set_option.  Every case here runs one such geometry and compares ALL frames and ALL bins
with oracle.stft on the same PCM, relative to the frame's peak, at the project's tolerances (FP32 1e-5, FP64 1e-12,
FP32 against FP64 1e-5, FP64 against the reference's FFTProcess fixture 1e-9).

Outputs are never allocated by the wrapper: every buffer is made here with three guard rows past n_frames and is
prefilled with a NaN of a known bit pattern.  After the call the rows [0, n_frames) must hold no NaN (a wave that
skipped a frame cannot hide behind a stale row of the caching allocator) and the guard rows, and the columns a kernel
promises not to touch, must still hold the pattern bit for bit (a write past the end shows without a fault).
The PCM is seeded noise (sigma 3000), different for every case, and the samples a batch needs end exactly where the
tensor handed to the library ends.

  1  stft1024_anyhop_kernel / stft512_kernel across n_frames = 32 n_cu, where they go to two frames per wave
  2  stft1024_hop512_kernel<K>, K = 1..4, with and without the read pass, and the read pass's own grid
  3  the five FP64 kernels: stft1024_f64_v2_kernel<DW, LOOP> and stft1024_f64_kernel, at every run length
  4  the slab loop of jdsp_stft_i16_f64_dev
  5  stft1024_hop512_half_kernel at every row pitch, the columns past 512 untouched
  6  the pinned-host pipeline at 512 points, at a generic hop, with its device buffers regrown between calls
"""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL32 = 1e-5            # FP32 paths against the oracle, and FP32 against FP64
TOL64 = 1e-12           # FP64 paths against the oracle
TOL_GOLDEN = 1e-9       # FP64 against the reference's FFTProcess (its truncated PI: ~1e-11)
GUARD = 3               # rows past n_frames in every output buffer
NAN32 = 0x7FC0BEEF                  # quiet NaNs with a payload no kernel produces
NAN64 = 0x7FF8DEADBEEF0001

STFT_DEFAULTS = {"stft.frames_per_wave": 0, "stft.read_pass_wg_per_cu": 0, "stft.read_pass": -1, "stft.f64_kernel": 0,
                 "stft.f64_frames_per_wave": 0, "stft.window": 0}

_LARGEST = {"fp32": 0.0, "fp64": 0.0, "fp32_vs_fp64": 0.0, "fp64_vs_fftprocess": 0.0}


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()
    print("\nlargest relative error seen (of the frame peak): " +
          ", ".join("%s %.3e" % kv for kv in sorted(_LARGEST.items())))


@contextlib.contextmanager
def _options(eng, **kw):
    """Sets "stft.<name>" options for the body and puts all six back to their defaults afterwards."""
    try:
        for name, value in kw.items():
            eng.set_option("stft." + name, value)
        yield
    finally:
        for name, value in STFT_DEFAULTS.items():
            eng.set_option(name, value)


def _pcm(n, *seed):
    rng = np.random.default_rng(list(seed))
    return np.clip(np.rint(rng.normal(0.0, 3000.0, n)), -32768, 32767).astype(np.int16)


def _dev(pcm, off=0):
    """A device copy of pcm whose last sample is the last of its tensor; `off` samples in front of it move the
    pointer 2 * off bytes off a 16-byte boundary."""
    import torch
    t = torch.from_numpy(np.concatenate([np.zeros(off, np.int16), pcm])).cuda()
    assert t.data_ptr() % 16 == 0
    return t[off:]


def _bits(t):
    import torch
    r = torch.view_as_real(t)
    return r.view(torch.int32 if r.dtype == torch.float32 else torch.int64)


def _pattern(t):
    import torch
    return NAN32 if t.dtype == torch.complex64 else NAN64


def _nan_rows(n_frames, cols, dtype, device="cuda", pinned=False):
    """[n_frames + GUARD, cols] of `dtype`, every word the NaN pattern."""
    import torch
    t = torch.empty((n_frames + GUARD, cols), dtype=dtype, device=device)
    if pinned:
        t = t.pin_memory()
    _bits(t).fill_(_pattern(t))
    return t


def _assert_written(t, n_frames, cols=None):
    """Rows [0, n_frames) x columns [0, cols) hold no NaN; the rest of the buffer is the prefill, bit for bit."""
    import torch
    nan_rows = torch.isnan(torch.view_as_real(t[:n_frames, :cols])).flatten(1).any(dim=1).nonzero().flatten()
    assert nan_rows.numel() == 0, "%d of %d rows not (wholly) written, first %s" % (
        nan_rows.numel(), n_frames, nan_rows[:12].tolist())
    b, pat = _bits(t), _pattern(t)
    touched = (b[n_frames:] != pat).flatten(1).any(dim=1).nonzero().flatten()
    assert touched.numel() == 0, "guard rows written: %s" % (touched + n_frames).tolist()
    if cols is not None and cols < t.shape[1]:
        assert bool((b[:n_frames, cols:] == pat).all()), "columns past %d written" % cols


def _rel_err(got, want):
    peak = np.abs(want).max(axis=1, keepdims=True)
    peak[peak == 0] = 1.0
    return float((np.abs(got - want) / peak).max())


def _check(kind, got, want, tol):
    err = _rel_err(np.asarray(got, np.complex128), want)
    _LARGEST[kind] = max(_LARGEST[kind], err)
    assert err < tol, err


def _host(t, n_frames, cols=None):
    return t[:n_frames, :cols].cpu().numpy().astype(np.complex128)


def _same_bits(a, b):
    import torch
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _stft32(eng, d, n_frames, n_fft=1024, hop=512):
    """The FP32 analysis into a guarded NaN buffer; returns the whole buffer."""
    import torch
    out = _nan_rows(n_frames, n_fft, torch.complex64)
    eng.stft(d, n_frames, n_fft, hop, out=out)
    torch.cuda.synchronize()
    _assert_written(out, n_frames)
    return out


def _stft64(eng, d, n_frames, hop):
    import torch
    out = _nan_rows(n_frames, 1024, torch.complex128)
    eng.stft_f64(d, n_frames, hop, out=out)
    torch.cuda.synchronize()
    _assert_written(out, n_frames)
    return out


# ---- 1. generic-hop 1024 and 512-point kernels across their threshold ---------------------------------------------
# (n_fft, hop, samples the PCM pointer is off 16 bytes): the last one is hop 512 on the generic path
GENERIC = [(1024, 160, 0), (1024, 333, 0), (1024, 1024, 0), (512, 256, 0), (512, 100, 0), (1024, 512, 1)]


@pytest.mark.parametrize("delta", [-1, 0, 3])
@pytest.mark.parametrize("n_fft,hop,off", GENERIC)
def test_generic_hop_kernels_across_the_two_frames_per_wave_threshold(eng, oracle, n_fft, hop, off, delta):
    """stft1024_anyhop_kernel and stft512_kernel give a wave two frames from n_frames = 2 * n_cu * 16 on: one frame
    below the threshold, at it, and three above (an odd count: the last wave has one frame).  Every frame against
    the oracle; the frames around the threshold recomputed as a batch of seven, which runs at one frame per wave,
    must come out with the same bits (the same kernel, the same arithmetic)."""
    thr = 32 * eng.n_cu
    n = thr + delta
    pcm = _pcm(hop * (max(n, thr + 3) - 1) + n_fft, 1, n_fft, hop, off, delta + 1)
    need = hop * (n - 1) + n_fft
    d = _dev(pcm[:need], off)
    assert d.data_ptr() % 16 == 2 * off
    out = _stft32(eng, d, n, n_fft, hop)
    _check("fp32", _host(out, n), oracle.stft(pcm[:need], n, n_fft, hop), TOL32)
    lo = thr - 4
    seven = _stft32(eng, _dev(pcm[hop * lo: hop * (lo + 6) + n_fft], off), 7, n_fft, hop)
    hi = min(n, thr + 3)
    assert hi - lo >= 3
    assert _same_bits(out[lo:hi], seven[:hi - lo])


# ---- 2. hop-512 fast path: frames per wave x read pass ----------------------------------------------------------------
HOP512_FRAMES = [1, 2, 3, 7, 8, 9, 4099, 1013]          # 1013 and 4099: multiples of neither 3 nor 8
_hop512_cache = {}


def _hop512_case(oracle, n):
    """(pcm on the device, oracle spectrum) of the n-frame hop-512 case; the same PCM for every geometry of one n."""
    if n not in _hop512_cache:
        pcm = _pcm(512 * (n + 1), 2, n)
        _hop512_cache[n] = (pcm, oracle.stft(pcm, n))
    pcm, want = _hop512_cache[n]
    return _dev(pcm), want


@pytest.mark.parametrize("n", HOP512_FRAMES)
@pytest.mark.parametrize("rp", [0, 1])
@pytest.mark.parametrize("fpw", [0, 1, 2, 3, 4, 5])
def test_hop512_every_frames_per_wave_with_and_without_the_read_pass(eng, oracle, fpw, rp, n):
    """stft1024_hop512_kernel<K> for K = 1, 2, 3, 4 ("stft.frames_per_wave"; 0 and 5 take the default), alone and
    behind the read pass, at batches that end inside a wave and inside the grid's round-up to eight blocks."""
    d, want = _hop512_case(oracle, n)
    assert d.data_ptr() % 16 == 0
    with _options(eng, frames_per_wave=fpw, read_pass=rp):
        out = _stft32(eng, d, n)
    _check("fp32", _host(out, n), want, TOL32)


@pytest.mark.parametrize("n", [4099, 1013])
def test_hop512_frames_per_wave_and_read_pass_do_not_change_a_bit(eng, oracle, n):
    d, _ = _hop512_case(oracle, n)
    outs = {}
    for fpw in (0, 1, 2, 3, 4, 5):
        for rp in (0, 1):
            with _options(eng, frames_per_wave=fpw, read_pass=rp):
                outs[fpw, rp] = _stft32(eng, d, n)
    first = outs[0, 0]
    differ = [k for k, v in outs.items() if not _same_bits(first, v)]
    assert not differ, differ


@pytest.mark.parametrize("n", [9, 4099])
@pytest.mark.parametrize("wg", [1, 4, 64])
def test_hop512_read_pass_grid_does_not_change_a_bit(eng, oracle, wg, n):
    """"stft.read_pass_wg_per_cu": the read pass's workgroups per CU, with the pass forced on."""
    d, want = _hop512_case(oracle, n)
    with _options(eng, read_pass=0):
        off = _stft32(eng, d, n)
    with _options(eng, read_pass=1, read_pass_wg_per_cu=wg):
        out = _stft32(eng, d, n)
    _check("fp32", _host(out, n), want, TOL32)
    assert _same_bits(out, off)


# ---- 3. FP64: all five kernels ---------------------------------------------------------------------------------------
# (hop, samples off 16 bytes, DW): DW = one dword per lane and row (pointer 4-byte aligned and hop even)
F64_INPUTS = [(512, 0, True), (160, 0, True), (333, 0, False), (1, 0, False), (512, 1, False)]
F64_FRAMES = 300
F64_RUNS = [0, 2, 3, 7, 16, 4096]                       # "stft.f64_frames_per_wave" of the default kernel
_f64_cache = {}


def _f64_case(oracle, hop, off):
    if (hop, off) not in _f64_cache:
        pcm = _pcm(hop * (F64_FRAMES - 1) + 1024, 3, hop, off)
        _f64_cache[hop, off] = (pcm, oracle.stft(pcm, F64_FRAMES, 1024, hop))
    pcm, want = _f64_cache[hop, off]
    return _dev(pcm, off), want


def _assert_dw(d, hop, dw):
    assert (d.data_ptr() % 4 == 0 and hop % 2 == 0) == dw


@pytest.mark.parametrize("fpw", F64_RUNS)
@pytest.mark.parametrize("hop,off,dw", F64_INPUTS)
def test_fp64_default_kernel_one_frame_per_wave_and_looping(eng, oracle, hop, off, dw, fpw):
    """stft1024_f64_v2_kernel<DW, LOOP>: LOOP from a run of 2 on (the next frame's samples are taken before this
    frame's stores), runs that do not divide 300, and one wave walking the whole batch (4096)."""
    d, want = _f64_case(oracle, hop, off)
    _assert_dw(d, hop, dw)
    with _options(eng, f64_kernel=0, f64_frames_per_wave=fpw):
        out = _stft64(eng, d, F64_FRAMES, hop)
    _check("fp64", _host(out, F64_FRAMES), want, TOL64)


@pytest.mark.parametrize("fpw", [0, 1, 5])
@pytest.mark.parametrize("hop,off,dw", F64_INPUTS)
def test_fp64_round2_kernel(eng, oracle, hop, off, dw, fpw):
    """stft1024_f64_kernel behind "stft.f64_kernel" = 1."""
    d, want = _f64_case(oracle, hop, off)
    with _options(eng, f64_kernel=1, f64_frames_per_wave=fpw):
        out = _stft64(eng, d, F64_FRAMES, hop)
    _check("fp64", _host(out, F64_FRAMES), want, TOL64)


def test_fp64_round2_kernel_automatic_run_of_four(eng, oracle):
    """"stft.f64_kernel" = 1 makes the batch one round of 4,096 waves: 3 * 4096 + 11 frames is a run of four, the last
    wave ragged, in the XCD-contiguous frame order."""
    n = 3 * 4096 + 11
    pcm = _pcm(512 * (n + 1), 3, n)
    with _options(eng, f64_kernel=1, f64_frames_per_wave=0):
        out = _stft64(eng, _dev(pcm), n, 512)
    _check("fp64", _host(out, n), oracle.stft(pcm, n), TOL64)


@pytest.mark.parametrize("kernel,fpw", [(1, 0), (1, 5), (0, 3)])
def test_fp64_kernels_match_reference_fftprocess_golden(eng, golden_dir, kernel, fpw):
    g = np.load(os.path.join(golden_dir, "stft_1024.npz"), allow_pickle=False)
    pcm, hop, want = g["pcm"], int(g["hop"]), g["spec"]
    n = want.shape[0]
    assert n > fpw                                     # the looping configuration loops
    with _options(eng, f64_kernel=kernel, f64_frames_per_wave=fpw):
        out = _stft64(eng, _dev(pcm[:hop * (n - 1) + 1024]), n, hop)
    _check("fp64_vs_fftprocess", _host(out, n), want, TOL_GOLDEN)


@pytest.mark.parametrize("hop,off,dw", F64_INPUTS)
def test_fp64_default_kernel_runs_give_the_same_bits(eng, oracle, hop, off, dw):
    """Within "stft.f64_kernel" = 0 and one DW value, the run length only changes which wave computes a frame."""
    d, _ = _f64_case(oracle, hop, off)
    outs = {}
    for fpw in F64_RUNS:
        with _options(eng, f64_kernel=0, f64_frames_per_wave=fpw):
            outs[fpw] = _stft64(eng, d, F64_FRAMES, hop)
    first = outs[0][:F64_FRAMES]
    peak = first.abs().amax(dim=1, keepdim=True)
    diff = {fpw: float(((o[:F64_FRAMES] - first).abs() / peak).max()) for fpw, o in outs.items()}
    print("fp64 hop %d off %d: largest difference from one frame per wave, of the frame peak: %s" % (hop, off, diff))
    differ = [fpw for fpw, o in outs.items() if not _same_bits(first, o[:F64_FRAMES])]
    assert not differ, (differ, diff)


@pytest.mark.parametrize("hop,off,dw", F64_INPUTS)
def test_fp32_analysis_against_the_fp64_analysis(eng, oracle, hop, off, dw):
    d, _ = _f64_case(oracle, hop, off)
    f64 = _stft64(eng, d, F64_FRAMES, hop)
    f32 = _stft32(eng, d, F64_FRAMES, 1024, hop)
    _check("fp32_vs_fp64", _host(f32, F64_FRAMES), _host(f64, F64_FRAMES), TOL32)


# ---- 4. FP64 slab loop -----------------------------------------------------------------------------------------------
def test_fp64_slab_loop_gives_the_bits_of_one_launch(eng, oracle):
    """jdsp_stft_i16_f64_dev cuts a hop-512 batch behind the read pass into slabs of 65,536 frames: 65,536 + 1,027
    frames are two slabs with "stft.read_pass" = -1 and one launch with 0."""
    import torch
    n = 65536 + 1027
    pcm = _pcm(512 * (n + 1), 4)
    d = _dev(pcm)
    try:
        with _options(eng, read_pass=-1):
            slabs = _stft64(eng, d, n, 512)
        with _options(eng, read_pass=0):
            one = _stft64(eng, d, n, 512)
        assert torch.equal(_bits(slabs), _bits(one))
        for lo, hi in ((65536 - 300, 65536 + 300), (n - 300, n)):
            want = oracle.stft(pcm[512 * lo: 512 * (hi + 1)], hi - lo)
            _check("fp64", slabs[lo:hi].cpu().numpy(), want, TOL64)
    finally:
        slabs = one = d = None
        torch.cuda.empty_cache()


# ---- 5. half spectrum ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 1001])
@pytest.mark.parametrize("pitch", [513, 514, 520, 1024])
def test_half_spectrum_every_row_pitch(eng, oracle, pitch, n):
    """stft1024_hop512_half_kernel: bins 0..512 at row pitches that put odd rows 8 bytes off (513) and that do not;
    the columns past 512 and the guard rows stay untouched."""
    import torch
    pcm = _pcm(512 * (n + 1), 5, pitch, n)
    d = _dev(pcm)
    half = _nan_rows(n, pitch, torch.complex64)
    eng.stft_half(d, n, out=half, pitch=pitch)
    torch.cuda.synchronize()
    _assert_written(half, n, 513)
    _check("fp32", _host(half, n, 513), oracle.stft(pcm, n)[:, :513], TOL32)
    # and against the full-spectrum kernel: a different twiddle factorisation for some bins of the odd rows of an odd
    # pitch, the same arithmetic everywhere else
    with _options(eng, read_pass=0):
        full = _stft32(eng, d, n)
    ref, got = full[:n, :513], half[:n, :513]
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    assert err < 2e-6, err
    assert _same_bits(got[0::2, :512], ref[0::2, :512])


# ---- 6. pinned-host pipeline -----------------------------------------------------------------------------------------
def test_pinned_pipeline_512_points_generic_hop_and_regrown_buffers(oracle):
    """stft_pipelined keeps four device buffers sized for the last configuration: (512, 256) first, then (1024, 160)
    needs larger spectrum buffers, then (1024, 512) larger PCM buffers.  Five chunks of 4,096 frames and one of five;
    the same bits as the pageable-host path, every frame against the oracle."""
    import torch
    import jeicyboodsp_amd
    eng = jeicyboodsp_amd.Engine(0)
    try:
        n = 5 * 4096 + 5
        for n_fft, hop in ((512, 256), (1024, 160), (1024, 512)):
            pcm = _pcm(hop * (n - 1) + n_fft, 6, n_fft, hop)
            pin_in = torch.from_numpy(pcm).pin_memory()
            pin_out = _nan_rows(n, n_fft, torch.complex64, device="cpu", pinned=True)
            assert pin_in.is_pinned() and pin_out.is_pinned()
            eng.stft(pin_in.numpy(), n_fft=n_fft, hop=hop, out=pin_out.numpy()[:n])
            _assert_written(pin_out, n)
            plain = _nan_rows(n, n_fft, torch.complex64, device="cpu")
            eng.stft(pcm, n_fft=n_fft, hop=hop, out=plain.numpy()[:n])
            _assert_written(plain, n)
            assert torch.equal(_bits(pin_out), _bits(plain)), (n_fft, hop)
            _check("fp32", pin_out[:n].numpy(), oracle.stft(pcm, n, n_fft, hop), TOL32)
    finally:
        eng.close()
