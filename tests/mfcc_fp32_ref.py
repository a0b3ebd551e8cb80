"""CPU restatement of the MFCC kernels' single-precision front end (not a test module).

  single(cfg, frame)    one frame per transform, as mfcc_kernel / mfcc_x2_kernel compute it
  paired(cfg, a, b)     two frames in ONE complex transform, as mfcc512_pair_mags packs them:
                        z = a + j b,  A[k] = (Z[k] + conj Z[N-k]) / 2,  B[k] = -j (Z[k] - conj Z[N-k]) / 2

Both run pre-emphasis (x[0] = 0, x[i] = s[i] - preemph s[i-1]), the Hamming window, the zero-padded transform and |X|
in FP32 (the transform on complex64, never upcast), then the FP64 oracle's MelFilterBank, DCT and Liftering.  What
they differ by is what the packing costs: the partner's transform rounding, about 6e-8 sqrt(E_partner) per bin, lands
in this frame's bins, and ln() of a mel channel divides it by the channel's own sum.

The module also holds the seeded input families of the coloured-frame tests and the one case list the CPU test
(test_mfcc_fp32_ref_cpu.py) and the device test (test_mfcc_coloured_gpu.py) share.  A flat spectrum is the one input on
which the leak cannot show; these are the ones on which it does.
"""
import functools

import numpy as np

F32 = np.float32
PARTNER_AMP = 9000.0
LEVELS_DB = (0, 10, 20, 30, 35)
KINDS = ("vowel120", "vowel180", "lowpass", "highpass", "tone", "white")
PARTNERS = ("white", "vowel180")
N_SEEDS = 4
BASE_SEED = 2810
# Draws replaced on the CPU, (frame length, kind, dB, partner, slot, seed) -> the draw taken: the first whose two frames,
# each ALONE in the FP32 chain above, are within 3.5e-6 of the oracle in the configuration that uses that frame length
# (test_mfcc_fp32_ref_cpu.py holds all of them to 4e-6).  Narrow low mel channels under the pre-emphasis are where FP32
# itself runs out: a few draws of every family leave one of them 90 dB under the frame's peak.
_BUMP = {
    (400, 3, 35, 0, 0, 3): 1, (400, 4, 20, 1, 0, 1): 1, (400, 4, 30, 0, 0, 3): 1, (512, 0, 0, 1, 1, 0): 1, (512, 0,
    30, 0, 0, 1): 1, (512, 0, 30, 1, 1, 2): 1, (512, 0, 35, 1, 1, 0): 1, (512, 1, 35, 1, 0, 1): 1, (512, 2, 10, 0,
    0, 0): 1, (512, 2, 10, 0, 1, 1): 1, (512, 2, 10, 1, 1, 3): 1, (512, 3, 10, 1, 0, 1): 2, (512, 3, 30, 0, 0, 0):
    1, (512, 4, 30, 0, 1, 1): 1, (512, 4, 30, 0, 1, 2): 1, (512, 4, 30, 1, 0, 1): 1, (512, 4, 30, 1, 1, 0): 1, (512,
    4, 30, 1, 1, 3): 1, (512, 4, 35, 0, 0, 3): 1, (512, 4, 35, 0, 1, 3): 1, (512, 4, 35, 1, 1, 1): 1, (1024, 0, 0,
    0, 0, 1): 3, (1024, 0, 0, 0, 0, 3): 2, (1024, 0, 0, 0, 1, 1): 2, (1024, 0, 0, 0, 1, 2): 2, (1024, 0, 0, 0, 1,
    3): 1, (1024, 0, 0, 1, 0, 1): 1, (1024, 0, 0, 1, 1, 0): 3, (1024, 0, 10, 0, 0, 1): 3, (1024, 0, 10, 1, 0, 2): 2,
    (1024, 0, 10, 1, 1, 0): 3, (1024, 0, 10, 1, 1, 2): 1, (1024, 0, 20, 0, 0, 3): 1, (1024, 0, 20, 0, 1, 0): 1,
    (1024, 0, 20, 0, 1, 1): 1, (1024, 0, 20, 1, 0, 1): 1, (1024, 0, 30, 1, 1, 1): 1, (1024, 0, 35, 1, 0, 0): 1,
    (1024, 1, 0, 0, 1, 1): 1, (1024, 1, 0, 0, 1, 2): 2, (1024, 1, 0, 1, 0, 0): 1, (1024, 1, 0, 1, 0, 1): 1, (1024,
    1, 0, 1, 1, 2): 1, (1024, 1, 10, 1, 0, 0): 1, (1024, 1, 10, 1, 0, 1): 1, (1024, 1, 20, 1, 1, 2): 1, (1024, 1,
    35, 1, 1, 0): 1, (1024, 2, 10, 1, 0, 3): 1, (1024, 2, 35, 1, 0, 1): 3, (1024, 2, 35, 1, 1, 0): 1, (1024, 3, 0,
    0, 1, 2): 1, (1024, 3, 0, 1, 1, 0): 2, (1024, 3, 10, 1, 0, 3): 1, (1024, 3, 20, 0, 1, 2): 2, (1024, 3, 20, 1, 0,
    3): 1, (1024, 3, 30, 0, 0, 1): 1, (1024, 3, 35, 1, 0, 0): 1, (1024, 3, 35, 1, 0, 1): 2, (1024, 3, 35, 1, 1, 0):
    1, (1024, 3, 35, 1, 1, 3): 1, (1024, 4, 0, 1, 0, 0): 4, (1024, 4, 0, 1, 1, 1): 2, (1024, 4, 10, 0, 0, 2): 1,
    (1024, 4, 10, 1, 1, 0): 2, (1024, 4, 20, 0, 1, 2): 1, (1024, 4, 20, 0, 1, 3): 1, (1024, 4, 30, 0, 0, 0): 1,
    (1024, 4, 30, 0, 0, 3): 1, (1024, 4, 30, 0, 1, 2): 1, (1024, 4, 30, 1, 0, 1): 1, (1024, 4, 30, 1, 0, 2): 1,
    (1024, 4, 30, 1, 1, 3): 1, (1024, 4, 35, 0, 0, 3): 2, (1024, 4, 35, 0, 1, 3): 1, (1024, 4, 35, 1, 1, 2): 1,
    (1024, 5, 0, 1, 0, 1): 1, (1024, 5, 0, 1, 1, 0): 1, (1024, 5, 0, 1, 1, 3): 1, (1024, 5, 20, 1, 1, 1): 1, (1024,
    5, 20, 1, 1, 2): 1, (1024, 5, 30, 1, 0, 1): 1, (1024, 5, 30, 1, 0, 3): 2,
}


@functools.lru_cache(maxsize=None)
def _oracle():
    import oracle_lib
    return oracle_lib.load_oracle()


# ---- the FP32 chain --------------------------------------------------------------------------------------------------
def fft32(z):
    """Forward transform of a complex64 vector IN single precision."""
    z = np.ascontiguousarray(z, np.complex64)
    r = np.fft.fft(z)
    if r.dtype != np.complex64:                     # a numpy that upcasts: torch's CPU transform keeps the type
        import torch
        r = torch.fft.fft(torch.from_numpy(z)).numpy()
    assert r.dtype == np.complex64, r.dtype
    return r


# ---- the kernels' own transform: three plain FP32 radix-8 passes (wave_fft512.h) -------------------------------------------
# numpy's complex64 transform rounds to about 2.5e-8 of its output's rms per bin.  A plain FP32 transform -- the
# kernels' three radix-8 passes with table twiddles, restated here pass for pass, or any textbook radix-2 -- rounds to
# about 1.0e-7: the constant the pair kernel's criterion (mfcc_leak_redo, 2^-23) rests on, and the reason the figures
# of single() and paired() are a floor for the device, not an estimate of it.
_S = F32(0.70710678118654752440)


def _mj(a):
    return (a.imag - 1j * a.real).astype(np.complex64)             # -j a


def _dft8(v):
    """8-point DFT along axis 0 of a complex64 array, in the kernels' butterfly order (dft8)."""
    a0, a4 = v[0] + v[4], v[0] - v[4]
    a1, d1 = v[1] + v[5], v[1] - v[5]
    a2, d2 = v[2] + v[6], v[2] - v[6]
    a3, d3 = v[3] + v[7], v[3] - v[7]
    p5, p7 = d1 + _mj(d1), d3 - _mj(d3)                             # (1 - j) d1, (1 + j) d3
    b0, b2 = a0 + a2, a0 - a2
    b1, d13 = a1 + a3, a1 - a3
    b4, b6 = a4 + _mj(d2), a4 - _mj(d2)
    u, w = p5 - p7, p5 + p7
    us = (u.real * _S + 1j * (u.imag * _S)).astype(np.complex64)
    ws = _mj((w.real * _S + 1j * (w.imag * _S)).astype(np.complex64))
    out = np.stack([b0 + b1, b4 + us, b2 + _mj(d13), b6 + ws, b0 - b1, b4 - us, b2 - _mj(d13), b6 - ws])
    assert out.dtype == np.complex64
    return out


_T1 = np.stack([np.exp(-2j * np.pi * np.arange(64) * k / 512) for k in range(8)]).astype(np.complex64)     # [k1][l]
_T2 = np.stack([np.exp(-2j * np.pi * np.arange(8) * c / 64) for c in range(8)]).astype(np.complex64)       # [c][b]


def fft32_radix8(z):
    """512-point forward transform as wave_fft512 computes it: n = 64 r + l, k = k1 + 8 c + 64 d."""
    z = np.ascontiguousarray(z, np.complex64).reshape(8, 64)                                   # [r][l]
    A = (_dft8(z) * _T1).astype(np.complex64).reshape(8, 8, 8)                                 # [k1][a][b]
    B = (_dft8(np.moveaxis(A, 1, 0)) * _T2[:, None, :]).astype(np.complex64)                   # [c][k1][b]
    Zd = _dft8(np.moveaxis(B, 2, 0))                                                           # [d][c][k1]
    d, c, k1 = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    Z = np.empty(512, np.complex64)
    Z[(k1 + 8 * c + 64 * d).ravel()] = Zd.ravel()
    return Z


@functools.lru_cache(maxsize=None)
def _window(win_len):
    return _oracle().hamming(win_len).astype(F32)


def front(cfg, frame):
    """int16 frame [win_len] -> pre-emphasised, windowed, zero-padded FP32 [n_fft]"""
    s = np.asarray(frame).astype(F32)
    assert s.size == cfg.win_len
    x = np.zeros(cfg.n_fft, F32)
    x[1:cfg.win_len] = s[1:] - F32(cfg.preemph) * s[:-1]
    x[:cfg.win_len] *= _window(cfg.win_len)
    assert x.dtype == F32
    return x


def tail(cfg, mag):
    """FP32 |X| [n_bins] -> the oracle's mel filterbank + ln, DCT, lifter (FP64)"""
    o = _oracle()
    assert mag.dtype == F32
    return o.liftering(cfg, o.dct(cfg, o.mel_filterbank(cfg, mag.astype(np.float64))))[0]


def single(cfg, frame):
    Z = fft32(front(cfg, frame))
    return tail(cfg, np.abs(Z[:cfg.n_bins]))


def pair_spectra(cfg, a, b, transform=fft32):
    """(A, B, E_a, E_b): the two separated complex64 spectra [n_fft] and the frames' energies sum x^2"""
    xa, xb = front(cfg, a), front(cfg, b)
    Z = transform(xa + np.complex64(1j) * xb)
    Zm = np.conj(np.roll(Z[::-1], 1))               # conj Z[N - k], Z[N] = Z[0]
    A = (Z + Zm) * F32(0.5)
    B = (Z - Zm) * np.complex64(-0.5j)
    assert A.dtype == np.complex64 and B.dtype == np.complex64
    return A, B, float(np.sum(xa.astype(np.float64) ** 2)), float(np.sum(xb.astype(np.float64) ** 2))


def paired(cfg, a, b, transform=fft32):
    A, B, _, _ = pair_spectra(cfg, a, b, transform)
    return tail(cfg, np.abs(A[:cfg.n_bins])), tail(cfg, np.abs(B[:cfg.n_bins]))


def want(cfg, frame):
    """The FP64 oracle's vector of one frame."""
    return _oracle().mfcc_frames(cfg, np.ascontiguousarray(frame, np.int16), 1)[0]


def rel(got, ref):
    """The project's figure: largest |got - want| over the vector's peak."""
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---- input families: one frame of n samples at rate fs, int16 through clip(rint(.)) --------------------------------------
def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def white(rng, n, sigma):
    return _i16(rng.normal(0.0, sigma, n))


def vowel(rng, n, fs, f0, amp, tilt=-12.0, noise=1.0):
    """Harmonics of f0 up to 0.975 of Nyquist, random phases, `tilt` dB per octave, over white noise of `noise` LSB."""
    t = np.arange(n)
    x = np.zeros(n)
    k = 1
    while k * f0 < 0.975 * fs / 2:
        x += amp * k ** (tilt / 6.02) * np.sin(2 * np.pi * k * f0 * t / fs + rng.uniform(0, 2 * np.pi))
        k += 1
    return _i16(x + rng.normal(0.0, noise, n))


def _shaped_noise(rng, n, fs, stop, amp, stop_db):
    X = np.fft.rfft(rng.normal(0.0, 1.0, n))
    f = np.fft.rfftfreq(n, 1.0 / fs)
    X[stop(f)] *= 10.0 ** (stop_db / 20.0)
    x = np.fft.irfft(X, n)
    return _i16(amp * x / x.std())


def lowpass_noise(rng, n, fs, cut, amp, stop_db):
    """White noise with everything above `cut` Hz taken down by stop_db in the rfft domain, scaled to rms amp."""
    return _shaped_noise(rng, n, fs, lambda f: f > cut, amp, stop_db)


def highpass_noise(rng, n, fs, cut, amp, stop_db):
    return _shaped_noise(rng, n, fs, lambda f: f < cut, amp, stop_db)


def tone(rng, n, fs, f, amp):
    return _i16(amp * np.sin(2 * np.pi * f * np.arange(n) / fs + rng.uniform(0, 2 * np.pi)))


# ---- the case list ---------------------------------------------------------------------------------------------------
def quiet_frame(kind, rng, n, fs, amp):
    """One frame of `kind` at level amp.  Cut-offs and the tone range are given for 16 kHz and scale with the rate."""
    s = fs / 16000.0
    if kind == "vowel120":
        return vowel(rng, n, fs, 120.0, amp, noise=0.5)
    if kind == "vowel180":
        return vowel(rng, n, fs, 180.0, amp)
    if kind == "lowpass":
        return lowpass_noise(rng, n, fs, 1000.0 * s, amp, -60.0)
    if kind == "highpass":
        return highpass_noise(rng, n, fs, 3000.0 * s, amp, -60.0)
    if kind == "tone":
        return tone(rng, n, fs, rng.uniform(200.0, 7000.0) * s, amp)
    if kind == "white":
        return white(rng, n, amp)
    raise ValueError(kind)


def loud_frame(partner, rng, n, fs):
    return white(rng, n, PARTNER_AMP) if partner == "white" else vowel(rng, n, fs, 180.0, PARTNER_AMP)


@functools.lru_cache(maxsize=None)
def cases(n=400, fs=16000.0):
    """Every pair of the coloured-frame tests: 6 kinds x 5 levels x 2 partners x 2 slots x 4 seeds = 480 dicts
    {kind, db, partner, slot, seed, a, b}; a and b are the int16 frames of transform slots a and b, the quiet one in
    `slot`.  The same list, in the same order, whoever asks."""
    out = []
    for ik, kind in enumerate(KINDS):
        for db in LEVELS_DB:
            for ip, partner in enumerate(PARTNERS):
                for slot in (0, 1):
                    for seed in range(N_SEEDS):
                        rng = np.random.default_rng([BASE_SEED, ik, db, ip, slot, seed, _BUMP.get((n, ik, db, ip, slot, seed), 0)])
                        quiet = quiet_frame(kind, rng, n, fs, PARTNER_AMP * 10.0 ** (-db / 20.0))
                        loud = loud_frame(partner, rng, n, fs)
                        a, b = (quiet, loud) if slot == 0 else (loud, quiet)
                        out.append(dict(kind=kind, db=db, partner=partner, slot=slot, seed=seed, a=a, b=b))
    return tuple(out)


def frames_of(case_list):
    """[2 len, n] int16: a0, b0, a1, b1, ... -- frames 2 j and 2 j + 1 are pair j"""
    return np.stack([f for c in case_list for f in (c["a"], c["b"])])
