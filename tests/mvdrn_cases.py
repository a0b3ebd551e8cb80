"""The scenes white noise does not reach, for the n-microphone MVDR (jdsp_mvdrn_*, include/jdsp.h): the scenes, two
numpy restatements of oracle/jdsp_oracle.c's orc_mvdrn_stream2 and the bars.  No GPU import: tests/test_mvdrn_hard_cpu.py
shows on the CPU that every scene is sized for the bar and sees what `white` cannot, tests/test_mvdrn_hard_gpu.py holds
the kernels to the bar on them.

Bars (the header's): precast within 1e-5 of the utterance's own finite peak, int16 within 1 LSB, finite masks equal, all
against the C oracle.  With loading 0 an emitted block in front of the utterance's n_mics-th estimation frame is left
out (`held`): R_k is rank deficient there and both sides are non-finite or meaningless.  The count comes from the
oracle's VAD flags, never from an output."""
import numpy as np

from mvdrn_batch_cases import TOL                      # the bar, and mvdrn_batch_cases.check the check, are the batch tests'

FS = 16000.0
N_BLOCKS = 30                       # blocks of 512 samples (60 of 256 on an n_fft = 512 handle)
# (first block, blocks) of 512 without the source.  Nine blocks in front, not eight: block 0 is never an estimation
# frame, so nine give the eight frames that make R_k regular on 8 microphones before the first loud block, and a
# loading-0 case leaves out blocks 1 .. n_mics - 1 only (eight would leave out 18 of the 29, up to the second pause).
QUIET = ((0, 9), (18, 5))
LOADINGS = [1e-3, 1e-6, 0.0, 1.0]
N_MICS = [3, 8]
MAX_LEFT_OUT = {2: 3, 3: 3, 7: 10, 8: 10}      # emitted blocks a loading-0 case may leave out (of 29, or of 59)

SIGNAL_SCENES = ["white", "coherent", "hum", "lowpassed", "dc", "near", "loud_interferer", "gain_mismatch", "quiet_mic0"]
STEERING = ["steering_none", "steering_plus", "steering_frac", "steering_far"]
SCENES = SIGNAL_SCENES + STEERING
NEW_SCENES = SCENES[1:]


def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _loud(n):
    loud = np.ones(n)
    for b0, nb in QUIET:
        loud[b0 * 512:(b0 + nb) * 512] = 0
    return loud


def _delayed(x, samples):
    """x delayed by a fractional number of samples (circular, through the spectrum of the whole signal)"""
    f = np.fft.rfftfreq(x.size)
    return np.fft.irfft(np.fft.rfft(x) * np.exp(-2j * np.pi * f * samples), x.size)


def steering_delays(name, n_mics):
    m = np.arange(n_mics)
    return {"steering_none": None, "steering_zero": np.zeros(n_mics), "steering_plus": m / FS,
            "steering_frac": m * m * 0.37 / FS, "steering_far": -40.0 * m / FS}[name]


def scene(name, n_mics, seed=1):
    """(pcm int16 [n_mics, 512 N_BLOCKS], delays_s or None, src).  The source is white, one sample later per
    microphone (1.25 in `near`), steered at except in steering_*, and silent in QUIET; src is the clean source as
    microphone 0 hears it.
      white            today's scene (tests/test_mvdr_multi_gpu.py): interferer sd 30 at -2 samples, sensor noise sd 20
      coherent         an integer interferer of sd 50 at -2 samples and +-1 LSB of noise: R_k close to rank 1
      hum              a 50 Hz sine of amplitude 60, its phase 3 samples per microphone, and noise of sd 3
      lowpassed        sensor noise of sd 150 through a 32-tap moving average: tr(R_k) falls by orders over the bins
      dc               an offset of 10 + 5 m on microphone m and noise of sd 1: bin 0 against the rest
      near             an interferer of sd 50 at 1.0 sample per microphone, steering and source at 1.25, noise of sd
                       2: large weights at low bins
      loud_interferer  an interferer of sd 45 in the pauses that carries sd 20000 (clipped) under a source of sd 300,
                       noise of sd 4
      gain_mismatch    odd microphones at gain 1e-2 with noise sd 0.4, even ones at gain 1 with noise sd 50
      quiet_mic0       microphone 0: source and noise of sd 1; the others: an interferer of sd 3000 all the time
      steering_*       white's signals under other delays_s (steering_delays)
    Three noise floors are higher than first drawn (hum 0.5, near 1, loud_interferer 2): with those, plain FP32 alone
    took 0.52 to 5.1 of the bar at 8 microphones and loading 1e-6 or 0 (tests/test_mvdrn_hard_cpu.py holds it under 0.5),
    so the scenes were mis-sized for the bar, not the bar for the scenes."""
    M, n = n_mics, N_BLOCKS * 512
    rng = np.random.default_rng(seed)
    loud = _loud(n)
    m = np.arange(M)
    delays = -m / FS
    sigma = {"gain_mismatch": 6000.0, "loud_interferer": 300.0}.get(name, 3000.0)
    src = rng.normal(0, sigma, n)
    if name == "near":
        S = np.stack([_delayed(src, 1.25 * i) for i in m]) * loud
        delays = -1.25 * m / FS
    else:
        S = np.stack([np.roll(src, i) for i in m]) * loud
    if name == "white" or name.startswith("steering_"):
        interf = rng.normal(0, 30, n)
        x = S + rng.normal(0, 20, (M, n)) + np.stack([np.roll(interf, -2 * i) for i in m])
        if name != "white":
            delays = steering_delays(name, M)
    elif name == "coherent":
        interf = np.rint(rng.normal(0, 50, n))
        x = np.rint(S) + np.stack([np.roll(interf, -2 * i) for i in m]) + rng.integers(-1, 2, (M, n))
    elif name == "hum":
        t = np.arange(n)
        x = S + np.stack([60 * np.sin(2 * np.pi * 50 * (t + 3 * i) / FS) for i in m]) + rng.normal(0, 3, (M, n))
    elif name == "lowpassed":
        z = rng.normal(0, 150, (M, n + 31))
        x = S + np.stack([np.convolve(z[i], np.ones(32) / 32, "valid") for i in m])
    elif name == "dc":
        x = S + (10 + 5 * m)[:, None] + rng.normal(0, 1, (M, n))
    elif name == "near":
        interf = rng.normal(0, 50, n)
        x = S + np.stack([np.roll(interf, i) for i in m]) + rng.normal(0, 2, (M, n))
    elif name == "loud_interferer":
        interf = rng.normal(0, 1, n)
        x = S + np.stack([np.roll(interf, -2 * i) for i in m]) * np.where(loud > 0, 20000.0, 45.0) + rng.normal(0, 4, (M, n))
    elif name == "gain_mismatch":
        gains = np.ones(M)
        gains[1::2] = 1e-2
        x = S * gains[:, None] + np.where(gains[:, None] < 1, 0.4, 50.0) * rng.normal(0, 1, (M, n))
    elif name == "quiet_mic0":
        interf = rng.normal(0, 3000, n)
        x = S + rng.normal(0, 20, (M, n)) + np.stack([np.roll(interf, -2 * i) for i in m])
        x[0] = S[0] + rng.normal(0, 1, n)
    else:
        raise KeyError(name)
    return _i16(x), delays, src * loud


_scenes = {}


def cached_scene(name, n_mics):
    """scene(), built once and read-only"""
    key = (name, n_mics)
    if key not in _scenes:
        pcm, delays, src = scene(name, n_mics)
        pcm.setflags(write=False)
        src.setflags(write=False)
        _scenes[key] = (pcm, delays, src)
    return _scenes[key]


LATE = 26                                    # a loud block of 512 behind both pauses


def late_block_figures(pre, src, pcm, block):
    """(1 - correlation with the clean source, rms over microphone 0's) of the emission for the samples of block LATE"""
    lo, hi = LATE * 512, (LATE + 1) * 512
    got = np.asarray(pre, np.float64)[lo - block:hi - block]
    return 1 - np.corrcoef(got, src[lo:hi])[0, 1], np.sqrt((got ** 2).mean() / (pcm[0, lo:hi].astype(np.float64) ** 2).mean())


DISTORTIONLESS_LOADINGS = [1e-3, 1e-6]       # loading 1 leaves the estimate no shape: r falls to 0.98 in ref64


def delays_key(delays):
    return None if delays is None else tuple(np.asarray(delays, np.float64).tolist())


# ---- what a loading-0 case leaves out -------------------------------------------------------------------------------
def events_upto(flags):
    """estimation frames seen when block b is processed (its own included): quiet blocks behind a quiet block"""
    quiet = np.asarray(flags) == 0
    ev = np.zeros(quiet.size, np.int64)
    ev[1:] = quiet[1:] & quiet[:-1]
    return np.cumsum(ev)


def held_mask(flags, n_mics, loading, block):
    """bool per emitted sample: False where loading == 0 and fewer than n_mics estimation frames have been seen"""
    ev = events_upto(flags)[1:]
    held = np.ones(ev.size, bool) if loading != 0 else ev >= n_mics
    assert np.count_nonzero(~held) <= MAX_LEFT_OUT[n_mics], (np.count_nonzero(~held), n_mics)
    return np.repeat(held, block)


def flags_of(orc, pcm, n_fft):
    """the oracle's VAD decision of every block on microphone 0"""
    B = n_fft // 2
    return np.array([orc.mvdr_vad_block(pcm[0, b * B:(b + 1) * B])[0] for b in range(pcm.shape[1] // B)], np.uint8)


def share(pre, o_pre, held):
    """the share of the 1e-5 bar the worst held sample takes, and whether the finite masks agree on the held samples"""
    fin = np.isfinite(o_pre) & held
    same = np.array_equal(np.isfinite(pre)[held], np.isfinite(o_pre)[held])
    if not fin.any():
        return 0.0, same
    both = fin & np.isfinite(pre)
    return float(np.abs(pre[both] - o_pre[both]).max() / (TOL * max(np.abs(o_pre[fin]).max(), 1.0))), same


# ---- the restatements -----------------------------------------------------------------------------------------------
def _solve(A, b):
    """orc_mvdrn_stream2's solve_cplx on every bin at once: Gauss-Jordan with partial pivoting; A [bins, M, M], b [bins, M]"""
    A, b = A.copy(), b.copy()
    n_bins, M = b.shape
    idx = np.arange(n_bins)
    for p in range(M):
        best = p + np.argmax(np.abs(A[:, p:, p]), axis=1)
        rows, rhs = A[idx, best].copy(), b[idx, best].copy()
        A[idx, best], b[idx, best] = A[:, p], b[:, p]
        A[:, p], b[:, p] = rows, rhs
        piv = A[:, p, p].copy()
        A[:, p] /= piv[:, None]
        b[:, p] /= piv
        f = A[:, :, p].copy()
        f[:, p] = 0
        A -= f[:, :, None] * A[:, p, None, :]
        b -= f * b[:, p, None]
    return b


_tw32 = {}


def _fft32(z):
    """FFT along the last axis in complex64 arithmetic: radix 2, decimation in time, twiddles rounded from FP64"""
    z = np.asarray(z, np.complex64)
    n = z.shape[-1]
    if n not in _tw32:
        lg = n.bit_length() - 1
        rev = np.array([int(format(i, "0%db" % lg)[::-1], 2) for i in range(n)])
        _tw32[n] = rev, np.exp(-2j * np.pi * np.arange(n // 2) / n).astype(np.complex64)
    rev, tw = _tw32[n]
    a = z[..., rev]
    size = 2
    while size <= n:
        half = size // 2
        a = a.reshape(z.shape[:-1] + (n // size, size))
        t = a[..., half:] * tw[::n // size]
        a = np.concatenate([a[..., :half] + t, a[..., :half] - t], axis=-1)
        size *= 2
    return a.reshape(z.shape)


def _spectra(x, mode):
    """the N/2 + 1 bins of real rows x [M, N]: FP64; an FP32 transform per row; or two rows per complex FP32 transform"""
    M, N = x.shape
    if mode == "64":
        return np.fft.rfft(x.astype(np.float64), axis=-1)
    if mode == "32":
        return _fft32(x.astype(np.float32))[:, :N // 2 + 1]
    if M & 1:
        x = np.concatenate([x, np.zeros((1, N))])
    Z = _fft32(x[0::2].astype(np.float32) + 1j * x[1::2].astype(np.float32))
    Zr = np.conj(np.roll(Z[:, ::-1], 1, axis=-1))
    out = np.empty((x.shape[0], N), np.complex64)
    out[0::2] = (Z + Zr) * np.complex64(0.5)
    out[1::2] = (Z - Zr) * np.complex64(-0.5j)
    return out[:M, :N // 2 + 1]


def _hermitian32(Y, N):
    full = np.empty(N, np.complex64)
    full[:N // 2 + 1] = Y
    full[0] = full[0].real
    full[N // 2] = full[N // 2].real
    full[N // 2 + 1:] = np.conj(Y[1:N // 2][::-1])
    return full


def _run(pcm, delays, loading, n_fft, mode="64", mutant=None):
    """orc_mvdrn_stream2 restated: its VAD on microphone 0, its steering constant 3.141592, its KEEP_LEN framing, the
    update in front of the apply.  mode "64": FP64 throughout (ref64).  "32" / "paired": an FP32 transform, spectra
    rounded to FP32, the covariance and the solve in FP64 as the kernels have them, weights rounded to FP32, apply and
    inverse transform in FP32; "paired" puts two microphones through one complex forward transform and two blocks
    (2 i, 2 i + 1) through one inverse, a block whose spectrum is not finite going in as zero and out as NaN.
    mutant (FP64 only): "load00" loads with R[0][0] instead of tr / n_mics, "round_delays" rounds delays_s to whole
    samples, "stale_weights" processes an estimation block with the weights from before its own update."""
    pcm = np.asarray(pcm)
    M, n = pcm.shape
    N, B, K = n_fft, n_fft // 2, n_fft // 2 - 1
    NB, nb = N // 2 + 1, n // B
    d = np.zeros(M) if delays is None else np.asarray(delays, np.float64)
    if mutant == "round_delays":
        d = np.rint(d * FS) / FS
    c = np.exp(1j * (2 * 3.141592 * np.arange(NB)[:, None] * (FS / N) * d[None, :]))
    win = 0.54 - 0.46 * np.cos(2 * 3.141592 * np.arange(N) / (N - 1))
    R = np.zeros((NB, M, M), complex)
    eye = np.eye(M)
    run = events = 0
    w = None
    weights, traces, counts, spectra, flags = [], [], [], [], []
    with np.errstate(all="ignore"):
        for b in range(nb):
            s = np.zeros(N)
            s[K:K + B] = pcm[0, b * B:(b + 1) * B]
            voice = (np.trunc(s * win) ** 2).sum() / N > 700.0
            flags.append(voice)
            stale = w
            if not voice:
                run += 1
                if run > 1:
                    X = _spectra(pcm[:, (b - 1) * B:(b + 1) * B], mode).astype(complex).T
                    R += X[:, :, None] * X[:, None, :].conj() / N
                    events += 1
                    w = None
            else:
                run = 0
            if w is None:
                tr = np.einsum("kii->k", R).real
                load = loading * (R[:, 0, 0].real if mutant == "load00" else tr / M)
                x = _solve(R + load[:, None, None] * eye, c)
                w = x / (c.conj() * x).sum(1)[:, None]
                if mode != "64":
                    w = w.astype(np.complex64)
            use = stale if mutant == "stale_weights" and stale is not None else w
            x = np.zeros((M, N))
            if b > 0:
                x[:, :K] = pcm[:, (b - 1) * B:(b - 1) * B + K]
            x[:, K:K + B] = pcm[:, b * B:(b + 1) * B]
            X = _spectra(x, mode).T
            spectra.append((use.conj() * X).sum(1))
            weights.append(use)
            traces.append(np.einsum("kii->k", R).real.copy())
            counts.append(events)
        frames = []
        if mode == "64":
            frames = [np.fft.irfft(Y, N) for Y in spectra]
        elif mode == "32":
            frames = [np.conj(_fft32(np.conj(_hermitian32(Y, N)))).real * np.float32(1.0 / N) for Y in spectra]
        else:
            for b in range(0, nb, 2):
                pair = [spectra[b], spectra[b + 1] if b + 1 < nb else np.zeros(NB, np.complex64)]
                bad = [not np.isfinite(Y).all() for Y in pair]
                full = [_hermitian32(np.zeros(NB, np.complex64) if bad[t] else pair[t], N) for t in range(2)]
                z = np.conj(_fft32(np.conj(full[0] + np.complex64(1j) * full[1]))) * np.float32(1.0 / N)
                frames.append(np.full(N, np.nan) if bad[0] else z.real)
                frames.append(np.full(N, np.nan) if bad[1] else z.imag)
        pre = np.concatenate([np.asarray(f, np.float64)[K:K + B] for f in frames[1:nb]]) if nb > 1 else np.zeros(0)
    return {"pre": pre, "weights": weights, "tr": np.array(traces), "events": np.array(counts),
            "flags": np.array(flags, np.uint8), "R": R}


def ref64(pcm, delays, loading, n_fft=1024, mutant=None):
    """FP64 restatement of orc_mvdrn_stream2.  A dict: pre (the emitted samples before the cast), and per block the
    weights [bins, n_mics], tr (R_k's trace), events (estimation frames seen) and flags (the VAD's decision); R is the
    covariance the stream ends with."""
    return _run(pcm, delays, loading, n_fft, "64", mutant)


def ref32(pcm, delays, loading, n_fft=1024, paired=False):
    """The same chain in plain FP32 (see _run); paired=True is a plain-arithmetic model of the 512-point path."""
    return _run(pcm, delays, loading, n_fft, "paired" if paired else "32")


def covariance_after_first_pause(pcm, n_fft=1024):
    """R_k [bins, n_mics, n_mics] after the first quiet stretch (FP64)"""
    return _run(np.asarray(pcm)[:, :QUIET[0][1] * 512], None, 0.0, n_fft)["R"]
