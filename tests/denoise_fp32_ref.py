"""CPU restatement of one spectral-subtraction / Wiener frame in single precision (not a test module).

  chain64(frames, noise, mode)                 window, transform, gain, inverse transform on complex128 (numpy's FFT)
  chain32(frames, noise, mode)                 the same on complex64 throughout, one frame per transform
  chain32_paired(fa, fb, na, nb, mode)         two frames in ONE complex transform, as the 512-point kernels pack them:
                                               z = a + j b,  A[k] = (Z[k] + conj Z[N-k]) / 2,  B[k] = -j (Z[k] - conj Z[N-k]) / 2
  criterion(frames, noise, e_pair=None)        the kernels' per-frame figure rho (denoise_kernels.hip, phase_unsafe)

The single-precision transform is a textbook radix-2 (decimation in time, table twiddles rounded to FP32, every
butterfly rounded to complex64), for both frame sizes: NOT the kernels' three radix-8 passes and even/odd split.  Both
round to about 2^-23 sqrt(E) per bin (mfcc_fp32_ref.py pins that constant for the radix-8 passes), which is all the
mechanism needs, and the radix-2 runs batched over a stream's frames.  Its figures are a floor for the device, not an
estimate of it.

Spectral subtraction computes Y = (|X| - N) e^{j phase(X)} with no clamp at zero (SS:233-242).  Where |X[k]| is far
below N[k] the output is -N[k] e^{j phase}: its size is N[k] however small X[k] is, and its direction is the phase of
X[k] -- which a single-precision transform leaves arbitrary once |X[k]| is at the transform's own rounding.  White
noise never gets there; an exactly periodic frame has hundreds of such bins after the Hamming window.

The module also holds the seeded int16 input families and the one list of streams that the CPU test
(test_denoise_fp32_ref_cpu.py) and the device test (test_denoise_periodic_gpu.py) share.
"""
import functools

import numpy as np

import mfcc_fp32_ref as mref

F32 = np.float32
FS = 16000.0
TOL = 1e-5                       # the project's bar: of the peak, before the cast
# The kernels' threshold on rho (JDSP_PHASE_RHO in denoise_kernels.hip): rho predicts a frame's error relative to its own
# output, and half the project's bar is what one of the two frames of a block may use.  Over every frame of cases() and
# of the white streams of test_denoise_gpu.py, in every restated form, the smallest rho of a frame whose
# single-precision error exceeds half its bar is 1.02e-5 at 1024 points and 9.9e-6 at 512: a margin of two
# (test_denoise_fp32_ref_cpu.py asserts 1.9; profiles/r11_denoise_periodic.txt has the table).
RHO = 5.0e-6
# bins 0 and n/2 are real: they count only under REAL_BIN_K times the transform's rounding, where their sign can flip
REAL_BIN_K = 16.0


@functools.lru_cache(maxsize=None)
def _oracle():
    import oracle_lib
    return oracle_lib.load_oracle()


# ---- the chain ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def window(n):
    """The reference's Hamming window (SS:226: its own PI), FP64."""
    return 0.54 - 0.46 * np.cos(2 * 3.141592 * np.arange(n) / (n - 1))


@functools.lru_cache(maxsize=None)
def _bitrev(n):
    bits = n.bit_length() - 1
    idx = np.arange(n)
    rev = np.zeros(n, np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    return rev


def fft_r2(z, ctype=np.complex64):
    """Textbook radix-2 transform along the last axis, every twiddle and butterfly rounded to `ctype`."""
    z = np.asarray(z, ctype)
    n = z.shape[-1]
    lead = z.shape[:-1]
    z = z[..., _bitrev(n)]
    m = 2
    while m <= n:
        w = np.exp(-2j * np.pi * np.arange(m // 2) / m).astype(ctype)
        z = z.reshape(lead + (n // m, m))
        a = z[..., : m // 2]
        b = (z[..., m // 2:] * w).astype(ctype)
        z = np.concatenate([(a + b).astype(ctype), (a - b).astype(ctype)], axis=-1).reshape(lead + (n,))
        m *= 2
    assert z.dtype == ctype
    return z


def ifft_r2(Z, ctype=np.complex64):
    """Unnormalised inverse transform through the forward one."""
    return np.conj(fft_r2(np.conj(Z).astype(ctype), ctype))


def _gain(X, noise, mode, rtype):
    """SS:233-242 / WF:196-213 on a spectrum of real type rtype; X == 0 -> phase 0 -> (-N, 0) in mode 0."""
    p = (X.real * X.real + X.imag * X.imag).astype(rtype)
    n = noise.astype(rtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == 0:
            g = (rtype(1) - (n / np.sqrt(p)).astype(rtype)).astype(rtype)
            Y = (X * g).astype(X.dtype)
            Y = np.where(p == 0, (-n).astype(X.dtype), Y)
        else:
            r = np.minimum(rtype(1), ((n * n) / p).astype(rtype))
            Y = (X * (rtype(1) - r).astype(rtype)).astype(X.dtype)
    return Y


def chain64(frames, noise, mode):
    """[f, n] int16 frames, [f, n] noise estimates -> [f, n] float64 samples, numpy's complex128 transform."""
    n = frames.shape[-1]
    X = np.fft.fft(frames.astype(np.float64) * window(n), axis=-1)
    return np.fft.ifft(_gain(X, noise, mode, np.float64), axis=-1).real


def chain64_r2(frames, noise, mode):
    """The same with the radix-2 above on complex128: the restatement's own arithmetic at double precision."""
    n = frames.shape[-1]
    X = fft_r2(frames.astype(np.float64) * window(n), np.complex128)
    return ifft_r2(_gain(X, noise, mode, np.float64), np.complex128).real / n


def spectrum32(frames):
    n = frames.shape[-1]
    x = (frames.astype(F32) * window(n).astype(F32)).astype(F32)
    return fft_r2(x, np.complex64)


def chain32(frames, noise, mode):
    """One frame per transform, complex64 throughout."""
    n = frames.shape[-1]
    Y = _gain(spectrum32(frames), noise, mode, F32)
    y = ifft_r2(Y, np.complex64).real * F32(1.0 / n)
    assert y.dtype == F32
    return y.astype(np.float64)


def pair_spectra32(fa, fb):
    """(A, B): the two frames' complex64 spectra out of one transform of a + j b."""
    n = fa.shape[-1]
    w = window(n).astype(F32)
    z = ((fa.astype(F32) * w) + np.complex64(1j) * (fb.astype(F32) * w)).astype(np.complex64)
    Z = fft_r2(z, np.complex64)
    Zm = np.conj(np.roll(Z[..., ::-1], 1, axis=-1))           # conj Z[N - k], Z[N] = Z[0]
    A = ((Z + Zm) * F32(0.5)).astype(np.complex64)
    B = ((Z - Zm) * np.complex64(-0.5j)).astype(np.complex64)
    return A, B


def chain32_paired(fa, fb, na, nb, mode, void=None):
    """Two frames per transform, forward and inverse, complex64 throughout: (ya, yb)."""
    n = fa.shape[-1]
    A, B = pair_spectra32(fa, fb)
    Ya, Yb = _gain(A, na, mode, F32), _gain(B, nb, mode, F32)
    if void is not None:                                      # a slot with no frame in it: nothing goes back in
        Ya = np.where(void[0][:, None], np.complex64(0), Ya)
        Yb = np.where(void[1][:, None], np.complex64(0), Yb)
    y = ifft_r2((Ya + np.complex64(1j) * Yb).astype(np.complex64), np.complex64) * F32(1.0 / n)
    return y.real.astype(np.float64), y.imag.astype(np.float64)


def rho_of(X, noise, energy, mode=0):
    """The kernels' figure from a complex64 spectrum, its noise estimate and the energy sum x^2 of the windowed samples
    that shared the transform: rho^2 = 2^-46 E sum (1 + (N / |X|)^2) / sum |Y|^2 -- rounding of 2^-23 sqrt(E) per bin,
    passed on along X as it is and across X times N / |X|, over the frame's own output (Parseval).  inf where a bin is
    exactly zero under a non-zero estimate; 0 for an all-zero transform (exact)."""
    p = (X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2)
    nz = noise.astype(np.float64)
    n = X.shape[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        q2 = 1.0 + np.where(p == 0, np.where(nz == 0, 0.0, np.inf), nz * nz / p)
        if mode == 1:                                             # Wiener: no amplifier, (1 + 2 r) eps at most per bin
            q2 = (1.0 + 2.0 * np.minimum(1.0, nz * nz / p)) ** 2
        # bins 0 and n/2 of a real frame are real: rounding cannot turn them, only flip their sign, and only when
        # they are at the rounding itself (REAL_BIN_K eps)
        real_ok = p[..., [0, n // 2]] >= (REAL_BIN_K ** 2 * 2.0 ** -46) * np.asarray(energy)[..., None]
        if mode == 0:
            q2[..., [0, n // 2]] = np.where(real_ok, 0.0, q2[..., [0, n // 2]])
        Y = _gain(X, noise, mode, F32)
        out = (Y.real.astype(np.float64) ** 2 + Y.imag.astype(np.float64) ** 2).sum(axis=-1)
        r2 = 2.0 ** -46 * energy * q2.sum(axis=-1) / out
    r2 = np.where(energy == 0, 0.0, np.where(np.isnan(r2), np.inf, r2))
    return np.sqrt(r2)


def frame_energy(frames):
    n = frames.shape[-1]
    return ((frames.astype(np.float64) * window(n)) ** 2).sum(axis=-1)


def criterion(frames, noise, e_pair=None):
    """rho per frame, one frame per transform (e_pair: the energy that shared the transform, if not the frame's own)."""
    return rho_of(spectrum32(frames), noise, frame_energy(frames) if e_pair is None else e_pair)


# ---- a stream through the chain ------------------------------------------------------------------------------------------
def stream_frames(pcm, block):
    """Frames 1 .. nb-1 of a stream: frame b = [block b-1, block b] (frame 0 is only stashed, SS:211-216)."""
    x = np.asarray(pcm, np.int16).reshape(-1, block)
    return np.concatenate([x[:-1], x[1:]], axis=1)


def overlap_add(y, block):
    """[f, 2 block] frames 1 .. nb-1 -> the pre-cast stream of blocks 2 .. nb-1 (SS:248-263)."""
    return (y[:-1, block:] + y[1:, :block]).ravel()


def frame_noise(trace):
    """The estimate each of the frames 1 .. nb-1 is subtracted with: main() estimates first (SS:98-110)."""
    _, _, _, noises, ver = trace
    return noises[ver[1:]]


def pairings(n_frames):
    """The two ways consecutive frames can share transforms: (0,1)(2,3).. and (1,2)(3,4)..; a frame left over runs with
    a silent partner.  Index -1 = silence."""
    out = []
    for first in (0, 1):
        idx = list(range(n_frames))
        if first:
            idx = [-1] + idx
        if len(idx) % 2:
            idx.append(-1)
        out.append(np.array(idx).reshape(-1, 2))
    return out


def stream32_paired(frames, noise, mode, pairs):
    """The stream's frames through chain32_paired in the given pairing -> [f, n] like chain32."""
    n = frames.shape[-1]
    fz = np.concatenate([frames, np.zeros((1, n), np.int16)])
    nz = np.concatenate([noise, np.zeros((1, n))])
    ya, yb = chain32_paired(fz[pairs[:, 0]], fz[pairs[:, 1]], nz[pairs[:, 0]], nz[pairs[:, 1]], mode,
                            void=(pairs[:, 0] < 0, pairs[:, 1] < 0))
    y = np.zeros((frames.shape[0] + 1, n))
    y[pairs[:, 0]] = ya
    y[pairs[:, 1]] = yb
    return y[:-1]


def criterion_paired(frames, noise, pairs, mode=0):
    n = frames.shape[-1]
    fz = np.concatenate([frames, np.zeros((1, n), np.int16)])
    nz = np.concatenate([noise, np.zeros((1, n))])
    A, B = pair_spectra32(fz[pairs[:, 0]], fz[pairs[:, 1]])
    e = frame_energy(fz[pairs[:, 0]]) + frame_energy(fz[pairs[:, 1]])
    r = np.zeros(frames.shape[0] + 1)
    r[pairs[:, 0]] = rho_of(A, nz[pairs[:, 0]], e, mode)
    r[pairs[:, 1]] = rho_of(B, nz[pairs[:, 1]], e, mode)
    return r[:-1]


def frame_bars(o_pre, block, n_frames):
    """Per frame 1 .. nb-1: TOL x the largest |oracle sample| of the (emitted) blocks the frame adds into -- never more
    than the per-block bar of either (block_bars), so two frames at half of it keep a block within its bar."""
    pk = np.abs(o_pre.reshape(-1, block)).max(axis=1)              # blocks 2 .. nb-1
    pk = np.concatenate([[0.0], pk, [0.0]])                        # blocks 1 .. nb
    return TOL * np.maximum(np.maximum(pk[:-1], pk[1:])[:n_frames], 1e-300)


def block_bars(o_pre, block):
    """Per emitted block: TOL x the largest |oracle sample| over the block and its two neighbours (the blocks that share
    a frame with it)."""
    pk = np.abs(o_pre.reshape(-1, block)).max(axis=1)
    pad = np.concatenate([[0.0], pk, [0.0]])
    return TOL * np.maximum(np.maximum(pad[:-2], pad[1:-1]), pad[2:])


# ---- input families: n samples, int16 through clip(rint(.)) ------------------------------------------------------------------
def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def white(rng, n, sigma=3000.0):
    return _i16(rng.normal(0.0, sigma, n))


def tone_on_bin(rng, n, n_fft, k, amp):
    """Exactly k cycles per n_fft samples: every frame cut from it at a multiple of the hop is exactly periodic."""
    return _i16(amp * np.sin(2 * np.pi * k * np.arange(n) / n_fft))


def tone_off_bin(rng, n, n_fft, k, amp):
    return _i16(amp * np.sin(2 * np.pi * k * np.arange(n) / n_fft + 0.3))


def two_tones_on_bin(rng, n, n_fft, k1, k2, a1, a2):
    t = np.arange(n)
    return _i16(a1 * np.sin(2 * np.pi * k1 * t / n_fft) + a2 * np.sin(2 * np.pi * k2 * t / n_fft + 1.0))


def square(rng, n, period, amp):
    """+amp for half a period, -amp for the other half; the period divides the frame."""
    return _i16(np.where((np.arange(n) // (period // 2)) % 2 == 0, amp, -amp))


def tone_on_bin_dithered(rng, n, n_fft, k, amp, sigma):
    return _i16(amp * np.sin(2 * np.pi * k * np.arange(n) / n_fft) + rng.normal(0.0, sigma, n))


def lowpass(rng, n, amp):
    return mref.lowpass_noise(rng, n, FS, 1000.0, amp, -60.0)


def highpass(rng, n, amp):
    return mref.highpass_noise(rng, n, FS, 3000.0, amp, -60.0)


def dc_plus_small(rng, n, dc=12000.0, sigma=50.0):
    return _i16(dc + rng.normal(0.0, sigma, n))


def impulse_train(rng, n, period, amp):
    x = np.zeros(n)
    x[period // 3::period] = amp
    return _i16(x)


def vowel(rng, n, amp, f0=137.0):
    return mref.vowel(rng, n, FS, f0, amp)


def quiet_lead(rng, n_blocks, block):
    """The non-voice lead-in of the other denoise tests: sigma 45 white (speechlike), sign-alternating at 256-sample
    blocks (speechlike256: the reference's ZCR threshold of 200 calls anything else voice)."""
    if block == 512:
        return _i16(rng.normal(0.0, 45.0, n_blocks * block))
    alt = np.where(np.arange(block) % 2 == 0, 1.0, -1.0)
    return _i16(((np.abs(rng.normal(0.0, 45.0, (n_blocks, block))) + 14.0) * alt).ravel())


# ---- the case list -------------------------------------------------------------------------------------------------------
LEAD = 14            # blocks: the noise estimate latches at the tenth quiet block in a row (SS:189)
# Amplitudes: the Hamming window at half overlap adds to 1.08, so 30000 is the largest round level whose output stays
# inside the (short) range; a +-32768 / 32767 square would leave it (35,389), and out-of-range conversion is a
# different subject, so the square runs at +-30000 too.
_STREAMS = (
    # name, periodic (mode 0 must miss +-1 LSB in FP32), stretches: (family, blocks, args for 1024, args for 512)
    ("white", False, (("white", 6, (3000.0,), (3000.0,)), ("white", 5, (300.0,), (300.0,)), ("white", 4, (6000.0,), (6000.0,)))),
    ("tone_bin64", True, (("tone_on_bin", 5, (64, 30000.0), (32, 30000.0)), ("tone_on_bin", 5, (64, 3000.0), (32, 3000.0)),
                          ("tone_on_bin", 5, (64, 20.0), (32, 20.0)))),
    ("tone_bin100", True, (("tone_on_bin", 5, (100, 30000.0), (50, 30000.0)), ("tone_on_bin", 4, (100, 3000.0), (50, 3000.0)),
                           ("tone_on_bin", 6, (100, 20.0), (50, 20.0)))),
    ("tone_off_bin", False, (("tone_off_bin", 5, (64.37, 30000.0), (32.37, 30000.0)), ("tone_off_bin", 5, (64.37, 3000.0), (32.37, 3000.0)),
                             ("tone_off_bin", 5, (100.5, 20.0), (50.5, 20.0)))),
    ("two_tones", True, (("two_tones_on_bin", 5, (32, 200, 9000.0, 7000.0), (16, 100, 9000.0, 7000.0)),
                         ("two_tones_on_bin", 5, (32, 200, 900.0, 700.0), (16, 100, 900.0, 700.0)),
                         ("two_tones_on_bin", 5, (7, 311, 14000.0, 14000.0), (7, 155, 14000.0, 14000.0)))),
    ("square", False, (("square", 5, (64, 30000.0), (64, 30000.0)), ("square", 5, (16, 20000.0), (16, 20000.0)),
                       ("square", 5, (256, 300.0), (128, 300.0)))),
    ("dithered", False, (("tone_on_bin_dithered", 5, (64, 30000.0, 0.3), (32, 30000.0, 0.3)),
                         ("tone_on_bin_dithered", 5, (64, 30000.0, 1.0), (32, 30000.0, 1.0)),
                         ("tone_on_bin_dithered", 5, (100, 3000.0, 0.3), (50, 3000.0, 0.3)))),
    ("coloured", False, (("lowpass", 5, (6000.0,), (6000.0,)), ("highpass", 5, (6000.0,), (6000.0,)), ("lowpass", 5, (200.0,), (200.0,)))),
    ("dc_impulse", False, (("dc_plus_small", 5, (), ()), ("impulse_train", 5, (300, 30000.0), (300, 30000.0)),
                           ("dc_plus_small", 5, (-20000.0, 5.0), (-20000.0, 5.0)))),
    ("vowel", False, (("vowel", 6, (6000.0,), (6000.0,)), ("vowel", 5, (900.0, 211.0), (900.0, 211.0)), ("vowel", 4, (90.0,), (90.0,)))),
)
# 512-point frames, two per transform: a quiet periodic stretch directly after and directly before a loud white one,
# stretches of odd length so that the boundary falls on either side of a pair
_BOUNDARY = (
    ("pair_tone20_white", True, (("white", 5, None, (3000.0,)), ("tone_on_bin", 5, None, (32, 20.0)), ("white", 3, None, (3000.0,)),
                                 ("tone_on_bin", 4, None, (50, 20.0)))),
    ("pair_square_white", False, (("white", 4, None, (6000.0,)), ("square", 5, None, (64, 40.0)), ("white", 5, None, (6000.0,)),
                                  ("tone_on_bin", 3, None, (32, 3000.0)))),
)
TAIL_WHITE = 6


def _build(name, periodic, stretches, n_fft, seed):
    block = n_fft // 2
    rng = np.random.default_rng([1911, n_fft, seed])
    parts, spans, b = [quiet_lead(rng, LEAD, block)], [], LEAD
    for fam, nb, a1024, a512 in stretches:
        args = a1024 if n_fft == 1024 else a512
        f = globals()[fam]
        x = f(rng, nb * block, n_fft, *args) if "on_bin" in fam or fam == "tone_off_bin" else f(rng, nb * block, *args)
        parts.append(x)
        spans.append((fam, b, b + nb))
        b += nb
    parts.append(white(rng, TAIL_WHITE * block, 3000.0))
    n_tail = TAIL_WHITE
    if name == "square":
        # The int16 extremes: one last block of a -32768 / 32767 square.  A stream's last block is only ever the second
        # half of its last frame, whose second half is never emitted, so the extremes go through the unpacking, the
        # window and the transform and shape an emitted block without any sample leaving the cast's range.
        parts.append(np.where((np.arange(block) // 32) % 2 == 0, 32767, -32768).astype(np.int16))
        n_tail += 1
    pcm = np.concatenate(parts)
    assert pcm.dtype == np.int16 and pcm.size == (b + n_tail) * block
    return dict(name="%s_%d" % (name, n_fft), n_fft=n_fft, block=block, periodic=periodic, pcm=pcm, spans=tuple(spans))


@functools.lru_cache(maxsize=None)
def cases():
    """Every stream of the periodic-input tests: dicts {name, n_fft, block, periodic, pcm, spans}; spans = (family, first
    block, one past the last) of each stretch.  The same list, in the same order, whoever asks."""
    out = []
    for n_fft in (1024, 512):
        for i, (name, periodic, stretches) in enumerate(_STREAMS):
            out.append(_build(name, periodic, stretches, n_fft, i))
    for i, (name, periodic, stretches) in enumerate(_BOUNDARY):
        out.append(_build(name, periodic, stretches, 512, 100 + i))
    return tuple(out)


# ---- the white streams of test_denoise_gpu.py ------------------------------------------------------------------------------
_PH = [40, 3, 25, 1, 90, 2, 11, 5]
_P256 = [13, 5, 2, 3, 11, 4, 1, 1, 16, 14]
# (block, seed, blocks, pattern, frames with rho > RHO in each restated form, largest count of frames with rho > RHO / 2
# over the forms): what the criterion makes of every speechlike / speechlike256 stream that test names with fixed
# arguments, mode 0, measured with this module.  The CPU test asserts the counts exactly, the device test that
# frames_recomputed stays within the last column: a drift of the criterion on white input fails a test.  Not listed:
# the randomly drawn streams of test_random_streams_and_call_cuts and the 65,536-block batches.
WHITE_STREAMS = (
    (512, 101, 1, None, (0,), 0), (512, 102, 2, None, (0,), 0), (512, 103, 3, None, (0,), 0), (512, 105, 5, None, (0,), 0),
    (512, 140, 40, None, (0,), 0), (512, 433, 333, None, (0,), 0), (512, 5, 123, None, (0,), 0), (512, 5, 206, None, (0,), 0),
    (512, 9, 130, None, (0,), 3), (512, 7, 64, [3, 2, 5, 1], (0,), 0), (512, 9, 60, [14, 2, 25, 3, 16], (0,), 1),
    (512, 77, 9500, _PH, (12,), 71),
    (512, 963, 70, [64, 6], (0,), 1), (512, 964, 71, [65, 6], (0,), 0), (512, 965, 72, [66, 6], (0,), 0),
    (512, 966, 73, [67, 6], (0,), 0), (512, 4990, 4097, [4091, 6], (6,), 36), (512, 5001, 4108, [4102, 6], (6,), 25),
    (512, 5004, 4111, [4105, 6], (7,), 30), (512, 5100, 4207, [4201, 6], (2,), 23),
    (256, 301, 1, _P256, (0, 0, 0), 0), (256, 302, 2, _P256, (0, 0, 0), 0), (256, 303, 3, _P256, (0, 0, 0), 0),
    (256, 306, 6, _P256, (0, 0, 0), 0), (256, 307, 7, _P256, (0, 0, 0), 0), (256, 308, 8, _P256, (0, 0, 0), 0),
    (256, 315, 15, _P256, (0, 0, 1), 3), (256, 380, 80, _P256, (2, 6, 6), 10), (256, 967, 667, _P256, (5, 44, 42), 70),
    (256, 77, 97, _P256, (0, 1, 0), 6), (256, 77, 206, _P256, (0, 3, 0), 12), (256, 77, 9500, _PH, (64, 358, 360), 1254),
)


def white_pcm(w):
    from test_denoise_gpu import speechlike, speechlike256
    block, seed, n_blocks, pattern = w[:4]
    return (speechlike if block == 512 else speechlike256)(seed, n_blocks, pattern=pattern)


def white_id(w):
    return "%d-%d-%d" % w[:3]


@functools.lru_cache(maxsize=None)
def trace(case_index, mode):
    """oracle.denoise_trace of a case, computed once and shared (read-only)."""
    c = cases()[case_index]
    t = _oracle().denoise_trace(mode, c["pcm"], block=c["block"])
    for a in t:
        a.setflags(write=False)
    return t
