"""CPU restatements of the reference's time-domain analysis programs (not a test module):

  PitchEstimation_method2.cpp:69-101   CalcPitch, AMDF              -> pitch_stream(pcm, 2)
  PitchEstimation_method3.cpp:69-101   CalcPitch, autocorrelation   -> pitch_stream(pcm, 3)
  LPCEstimation.cpp:87-137             LPCEstimation                -> lpc_stream(pcm, block_len, order)

The pitch sums are integers (numpy int64, exact); the reference holds them in a double, which is exact as well
(|sum| < 2^53), and divides once by (double)(1024 - k): the restatement gives the reference's bits.
The LPC chain is FP64 as in the reference; its solve is written as partial-pivot LU inverse times vector
(numpy.linalg.inv is LAPACK getrf + getri), which is what Eigen's inverse() * v does.  solve_ext() is an
extended-precision solve of the same Toeplitz system (mpmath), the yardstick for forward errors.
"""
import functools

import numpy as np

EPS = float(np.finfo(np.float64).eps)          # 2^-52


# ---- input families ------------------------------------------------------------------------------------------
def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def voiced(seed, n_blocks, block=512, f0=137.0, fs=16000.0, noise=200.0):
    rng = np.random.default_rng(seed)
    t = np.arange(n_blocks * block)
    f = f0 * (1 + 0.05 * np.sin(2 * np.pi * 0.7 * t / fs))
    ph = 2 * np.pi * np.cumsum(f) / fs
    return _i16(5000 * np.sin(ph) + 2500 * np.sin(2 * ph + 0.3) + 1200 * np.sin(3 * ph + 1.0) + rng.normal(0, noise, t.size))


def white(seed, n_blocks, block=512, sigma=3000.0):
    return _i16(np.random.default_rng(seed).normal(0, sigma, n_blocks * block))


def lowpassed(seed, n_blocks, block=512, sigma=6000.0):
    """white noise through a 9-tap moving average: a steep spectrum, the ill-conditioned end of the LPC families"""
    x = np.random.default_rng(seed).normal(0, sigma, n_blocks * block + 8)
    return _i16(np.convolve(x, np.ones(9) / 9.0, mode="valid"))


def full_scale(seed, n_blocks, block=512):
    return np.where(np.random.default_rng(seed).integers(0, 2, n_blocks * block) == 1, 32767, -32768).astype(np.int16)


def silence(n_blocks, block=512):
    return np.zeros(n_blocks * block, np.int16)


def constant(n_blocks, block=512, level=-12345):
    return np.full(n_blocks * block, level, np.int16)


def mixed(seed, n_blocks=40):
    """voiced tone plus noise, two silent blocks and one block of random +-full-scale samples"""
    x = voiced(seed, n_blocks, noise=400.0)
    x[17 * 512:19 * 512] = 0
    x[30 * 512:31 * 512] = full_scale(seed + 1, 1)
    return x


def pitch_families(n_blocks):
    """name -> int16 stream of n_blocks blocks of 512; every stream's first block follows a zero keep buffer"""
    fam = {
        "voiced": voiced(11, n_blocks),
        "white": white(12, n_blocks),
        "silence": silence(n_blocks),
        "constant": constant(n_blocks),
        "full_scale": full_scale(13, n_blocks),
    }
    if n_blocks >= 40:
        fam["mixed"] = mixed(14, n_blocks)
    return fam


def lpc_families(n_samples):
    """name -> int16 stream for the LPC checks (silence, whose frames have no solution, is checked apart)"""
    n = n_samples // 512
    return {
        "constant": constant(n)[:n_samples],
        "voiced": voiced(21, n)[:n_samples],
        "lowpassed": lowpassed(22, n)[:n_samples],
        "white": white(23, n)[:n_samples],
        "full_scale": full_scale(24, n)[:n_samples],
    }


# ---- pitch ---------------------------------------------------------------------------------------------------
def frames_of(pcm, block, prev_block=None):
    pcm = np.asarray(pcm, np.int16).reshape(-1, block)
    prev = np.zeros(block, np.int16) if prev_block is None else np.asarray(prev_block, np.int16).reshape(block)
    return np.concatenate([np.concatenate([prev[None], pcm[:-1]]), pcm], axis=1)       # [nb, 2 block]


def pitch_stream(pcm, method, prev_block=None):
    """-> (arg int32[nb], value float64[nb], curve float64[nb, 512]) of CalcPitch, method 2 (AMDF) or 3 (ACF)"""
    assert method in (2, 3)
    f = frames_of(pcm, 512, prev_block).astype(np.int64)
    nb = f.shape[0]
    sums = np.zeros((nb, 512), np.int64)
    for k in range(512):                                                               # :79-84
        a, c = f[:, :1024 - k], f[:, k:]
        sums[:, k] = np.abs(a - c).sum(axis=1) if method == 2 else (a * c).sum(axis=1)
    assert np.abs(sums).max(initial=0) < 2 ** 53
    curve = sums.astype(np.float64) / (1024 - np.arange(512)).astype(np.float64)
    # :87-95: from lag 511 down to 101 with <= (>=): the extreme value, and among equal values the smallest lag
    tail = curve[:, 101:]
    at = (tail.argmin(axis=1) if method == 2 else tail.argmax(axis=1)) + 101
    return at.astype(np.int32), curve[np.arange(nb), at], curve


# ---- LPC -----------------------------------------------------------------------------------------------------
def lpc_window(n):
    i = np.arange(n, dtype=np.float64)
    return 0.54 - 0.46 * np.cos((2 * 3.141592) * i / float(n - 1))                      # :105, PI 3.141592 (:34)


def lpc_windowed(pcm, block_len, prev_block=None):
    return frames_of(pcm, block_len, prev_block).astype(np.float64) * lpc_window(2 * block_len)


def lpc_autocorr(y, order):
    """[nb, N] windowed frames -> r [nb, order + 1] (:108-113) and the sums of |products| over (N - i)"""
    n = y.shape[1]
    r = np.stack([(y[:, :n - i] * y[:, i:]).sum(axis=1) / (n - i) for i in range(order + 1)], axis=1)
    mag = np.stack([np.abs(y[:, :n - i] * y[:, i:]).sum(axis=1) / (n - i) for i in range(order + 1)], axis=1)
    return r, mag


def toeplitz_system(r):
    p = len(r) - 1
    idx = np.abs(np.arange(p)[:, None] - np.arange(p)[None, :])
    return r[idx], -r[1:p + 1]                                                         # :115-123


def solve_lu_inverse(r):
    """the reference's solve in FP64: (partial-pivot LU inverse) times vector (:126); NaNs where T is singular"""
    T, v = toeplitz_system(np.asarray(r, np.float64))
    try:
        return np.linalg.inv(T) @ v
    except np.linalg.LinAlgError:
        return np.full(len(v), np.nan)


def solve_ext(r, digits=60):
    """the same system solved in `digits`-digit arithmetic (mpmath LU), rounded to float64 at the end"""
    import mpmath as mp
    T, v = toeplitz_system(np.asarray(r, np.float64))
    with mp.workdps(digits):
        x = mp.lu_solve(mp.matrix(T.tolist()), mp.matrix(v.tolist()))
        return np.array([float(t) for t in x])


def lpc_stream(pcm, block_len=256, order=12, prev_block=None):
    """-> (lpc [nb, order], autocorr [nb, order + 1]); all-zero frames give NaN rows"""
    r, _ = lpc_autocorr(lpc_windowed(pcm, block_len, prev_block), order)
    a = np.stack([solve_lu_inverse(row) if row[0] != 0 else np.full(order, np.nan) for row in r])
    return a, r


def cond2(r):
    T, _ = toeplitz_system(np.asarray(r, np.float64))
    return float(np.linalg.cond(T, 2))


def forward_error_units(a, a_ext, cond):
    """max |a - a_ext| in units of eps * cond_2(T) * max |a_ext|"""
    return float(np.abs(a - a_ext).max() / (EPS * cond * np.abs(a_ext).max()))


LPC_CASES = [(256, 12), (256, 1), (256, 16), (512, 12), (512, 1), (512, 16)]       # (block_len, order)
LPC_SAMPLES = 50 * 512                                                              # per family


@functools.lru_cache(maxsize=None)
def measure_k_ref(verbose=False):
    """K_ref: the worst forward error of the FP64 LU-inverse restatement against the extended-precision solve, in
    units of eps * cond_2(T) * |a|_inf, over lpc_families() x LPC_CASES (every frame).  Also the largest cond_2."""
    worst, worst_cond = 0.0, 0.0
    for block_len, order in LPC_CASES:
        for name, pcm in lpc_families(LPC_SAMPLES).items():
            a, r = lpc_stream(pcm, block_len, order)
            k_case = 0.0
            for row_a, row_r in zip(a, r):
                c = cond2(row_r)
                k_case = max(k_case, forward_error_units(row_a, solve_ext(row_r), c))
                worst_cond = max(worst_cond, c)
            if verbose:
                print("K_ref %-10s block %3d order %2d: %.3f" % (name, block_len, order, k_case))
            worst = max(worst, k_case)
    return worst, worst_cond
