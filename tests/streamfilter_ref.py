"""numpy / math restatements of the reference's two sample-serial filters and the seeded input families their tests
share (not a test module):
    7Band_GEQ.cpp   CalcCoefficient (:136-257) and ApplyIirGEQ (:259-332)
    NormalLMS.cpp   LMSFilter (:96-136)
Every product and every sum is one IEEE double operation, in the reference's order; Python floats and numpy float64
scalars never fuse.  tests/golden/streamfilter.npz holds what the compiled reference writes for these streams."""
import math

import numpy as np

GEQ_BLOCK, NLMS_BLOCK = 512, 1024
GAINS = (12.0, 12.0, 0.0, 0.0, 3.0, 0.0, -12.0)                      # 7Band_GEQ.cpp:51-57
FREQS = (44.0, 125.0, 250.0, 500.0, 2000.0, 6000.0, 11313.0)         # :47
PI, RATE, Q = 3.141592, 48000.0, 4.318
ROOT2 = 1.0 / Q


def cast_i16(v):
    """(short)double of the reference's build for values inside int32: truncate toward zero, keep the low 16 bits"""
    t = np.trunc(np.asarray(v, np.float64)).astype(np.int64)
    return ((t + 32768) % 65536 - 32768).astype(np.int16)


def _cast1(v):
    return ((int(v) + 32768) & 0xffff) - 32768


def geq_design(gain_db=None):
    """CalcCoefficient with the boost / cut branch taken from the sign of the gain; float64 [7, 2, 3].  math.tan, pow
    and sqrt are the C library's."""
    G = GAINS if gain_db is None else tuple(float(g) for g in gain_db)
    K = [math.tan(PI * f / RATE) for f in FREQS]
    V = [math.pow(10, g / 20.0) for g in G]
    V = [1.0 / v if v < 1 else v for v in V]
    sq, p2 = math.sqrt, lambda x: math.pow(x, 2.0)
    c = np.zeros((7, 2, 3), np.float64)
    if G[0] > 0:
        t = (1 + ROOT2 * K[0] + p2(K[0]))
        c[0, 0, 0] = (1 + sq(V[0]) * ROOT2 * K[0] + V[0] * p2(K[0])) / t
        c[0, 0, 1] = (2 * (V[0] * p2(K[0]) - 1)) / t
        c[0, 0, 2] = (1 - sq(V[0]) * ROOT2 * K[0] + V[0] * p2(K[0])) / t
        c[0, 1, 1] = (2 * (p2(K[0]) - 1)) / t
        c[0, 1, 2] = (1 - ROOT2 * K[0] + p2(K[0])) / t
    else:
        t = (1 + ROOT2 * sq(V[0]) * K[0] + V[0] * p2(K[0]))
        c[0, 0, 0] = (1 + ROOT2 * K[0] + p2(K[0])) / t
        c[0, 0, 1] = (2 * (p2(K[0]) - 1)) / t
        c[0, 0, 2] = (1 - ROOT2 * K[0] + p2(K[0])) / t
        c[0, 1, 1] = (2 * (K[0] * p2(K[0]) - 1)) / t                                  # :173, as written
        c[0, 1, 2] = (1 - ROOT2 * sq(K[0]) * K[0] + K[0] * p2(K[0])) / t              # :174, as written
    if G[6] > 0:
        t = (1 + ROOT2 * K[6] + p2(K[6]))
        c[6, 0, 0] = (V[6] + ROOT2 * sq(V[6]) * K[6] + p2(K[6])) / t
        c[6, 0, 1] = (2 * (p2(K[6]) - V[6])) / t
        c[6, 0, 2] = (V[6] - ROOT2 * sq(V[6]) * K[6] + p2(K[6])) / t
        c[6, 1, 1] = (2 * (p2(K[6]) - 1)) / t
        c[6, 1, 2] = (1 - ROOT2 * K[6] + p2(K[6])) / t
    else:
        t = (V[6] + ROOT2 * sq(V[6]) * K[6] + p2(K[6]))
        c[6, 0, 0] = (1 + ROOT2 * K[6] + p2(K[6])) / t
        c[6, 0, 1] = (2 * (p2(K[6]) - 1)) / t
        c[6, 0, 2] = (1 - ROOT2 * K[6] + p2(K[6])) / t
        t = (1 + ROOT2 / sq(V[6]) * K[6] + (p2(K[6])) / V[6])
        c[6, 1, 1] = (2 * ((p2(K[6])) / V[6] - 1)) / t
        c[6, 1, 2] = (1 - ROOT2 / sq(V[6]) * K[6] + (p2(K[6])) / V[6]) / t
    for k in range(1, 6):
        if G[k] > 0:
            t = (1 + ((1 / Q) * K[k]) + p2(K[k]))
            c[k, 0, 0] = (1 + ((V[k] / Q) * K[k]) + p2(K[k])) / t
            c[k, 0, 1] = (2 * (p2(K[k]) - 1)) / t
            c[k, 0, 2] = (1 - ((V[k] / Q) * K[k]) + p2(K[k])) / t
            c[k, 1, 1] = c[k, 0, 1]
            c[k, 1, 2] = (1 - ((1 / Q) * K[k - 1]) + p2(K[k])) / t                     # :231, K of the band below
        else:
            t = (1 + ((V[k] / Q) * K[k]) + p2(K[k]))
            c[k, 0, 0] = (1 + ((1.0 / Q) * K[k]) + p2(K[k])) / t
            c[k, 0, 1] = (2 * (p2(K[k]) - 1)) / t
            c[k, 0, 2] = (1 - ((1.0 / Q) * K[k]) + p2(K[k])) / t
            c[k, 1, 1] = c[k, 0, 1]
            c[k, 1, 2] = (1 - ((V[k] / Q) * K[k - 1]) + p2(K[k])) / t                  # :247
    return c


def geq_zero_state(n_sections):
    return np.zeros((n_sections + 1, 2), np.int16)


def geq(pcm, coeff, state=None):
    """One stream through the cascade, samples outside and sections inside.  state: int16 [n_sections + 1, 2],
    {older, newer}; row 0 the input's last two, row k + 1 section k's last two outputs.
    Returns (out int16 [n], precast float64 [n] of the last section, new state)."""
    coeff = np.asarray(coeff, np.float64)
    ns = coeff.shape[0]
    co = [[float(v) for v in coeff[k].reshape(6)] for k in range(ns)]
    st = geq_zero_state(ns) if state is None else np.asarray(state, np.int16)
    h = [[int(st[r, 0]), int(st[r, 1])] for r in range(ns + 1)]
    x = np.asarray(pcm, np.int16)
    out = np.zeros(len(x), np.int16)
    pre = np.zeros(len(x), np.float64)
    for t in range(len(x)):
        v = int(x[t])
        d = 0.0
        for k in range(ns):
            b0, b1, b2, _, a1, a2 = co[k]
            hi, ho = h[k], h[k + 1]
            d = 0.0
            d += b2 * hi[0]
            d -= a2 * ho[0]
            d += b1 * hi[1]
            d -= a1 * ho[1]
            d += b0 * v
            y = _cast1(d)
            hi[0], hi[1] = hi[1], v          # row k is complete once section k has read it
            v = y
        h[ns][0], h[ns][1] = h[ns][1], v
        out[t], pre[t] = v, d
    return out, pre, np.array(h, np.int16)


def nlms_zero_state(L=256):
    return np.zeros(L, np.float64), np.zeros(L - 1, np.int16)


def tree_sum(p, T):
    """The device's order: leaf l adds its T consecutive terms in ascending order, then a balanced pairwise tree over
    the 64 leaves, adjacent leaves first."""
    p = np.asarray(p, np.float64).reshape(64, T)
    s = p[:, 0].copy()
    for q in range(1, T):
        s = s + p[:, q]
    while len(s) > 1:
        s = s[0::2] + s[1::2]
    return float(s[0])


def nlms(x, ref, L=256, mu=1e-4, compensation=1e-4, state=None, order="reference"):
    """One stream.  state: (coefficients float64 [L], keep int16 [L - 1]).  order "reference": the dot product added
    in ascending j (np.add.accumulate is strictly left to right); "device": tree_sum.
    Returns (est int16 [n], err int16 [n], precast float64 [n], (coefficients, keep))."""
    assert order in ("reference", "device")
    cf, kp = nlms_zero_state(L) if state is None else state
    c = np.array(cf, np.float64)
    x = np.asarray(x, np.int16)
    ref = np.asarray(ref, np.int16)
    buf = np.concatenate([np.asarray(kp, np.int16), x]).astype(np.float64)
    sq = np.concatenate([[0.0], np.cumsum(buf * buf)])            # integers below 2^53: exact
    n = len(x)
    est, err, pre = np.zeros(n, np.int16), np.zeros(n, np.int16), np.zeros(n, np.float64)
    mu, compensation = np.float64(mu), np.float64(compensation)
    for i in range(n):
        w = buf[i:i + L]
        prod = c[::-1] * w                                        # :113 c[L-1-j] x[i+j]
        s = float(np.add.accumulate(prod)[-1]) if order == "reference" else tree_sum(prod, L // 64)
        e_hat = _cast1(s)
        e = int(ref[i]) - e_hat
        norm = (sq[i + L] - sq[i]) + compensation
        c += (((2.0 * w) * mu) * np.float64(e)) / norm            # :125, left to right
        est[i], err[i], pre[i] = e_hat, ((e + 32768) & 0xffff) - 32768, s
    keep = np.concatenate([np.asarray(kp, np.int16), x])[-(L - 1):]
    return est, err, pre, (c, keep.astype(np.int16))


# ---- seeded input families ------------------------------------------------------------------------------------------
def _i16(v):
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def white(seed, n, sigma=1500.0):
    return _i16(np.random.default_rng(seed).normal(0.0, sigma, n))


def silence(n):
    return np.zeros(n, np.int16)


def constant(n, value=12345):
    return np.full(n, value, np.int16)


def full_scale(seed, n):
    """+-full scale in runs of random length"""
    rng = np.random.default_rng(seed)
    sign = np.repeat(rng.integers(0, 2, n) * 2 - 1, rng.integers(1, 9, n))[:n]
    return np.where(sign > 0, 32767, -32768).astype(np.int16)


def impulse(n, value=16384):
    x = np.zeros(n, np.int16)
    x[0] = value
    return x


def echo_pair(seed, n, sigma=1500.0, taps=24, noise=20.0):
    """(input, reference): the reference is the input through a short decaying FIR plus noise"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, sigma, n)
    h = rng.normal(size=taps) * np.exp(-np.arange(taps) / 6.0) * 0.5
    d = np.convolve(x, h)[:n] + rng.normal(0.0, noise, n)
    return _i16(x), _i16(d)


def geq_families(n_blocks=16):
    n = n_blocks * GEQ_BLOCK
    return {"white": white(21, n), "loud": white(22, n, 9000.0), "silence": silence(n), "constant": constant(n),
            "full_scale": full_scale(23, n), "impulse": impulse(n)}


def nlms_families(n_blocks=8):
    n = n_blocks * NLMS_BLOCK
    z = silence(n)
    return {"echo": echo_pair(31, n), "loud": echo_pair(32, n, 9000.0, noise=100.0), "silence": (z, z),
            "constant": (constant(n), constant(n, -321)), "full_scale": (full_scale(33, n), full_scale(34, n)),
            "impulse": (impulse(n), white(35, n, 300.0))}


def stable_sections(n_sections, seed=5):
    """Caller-supplied coefficients for cascades other than the reference's seven: mild peaking sections (poles of
    radius below 0.9) whose gains keep the cascade near unity"""
    rng = np.random.default_rng(seed)
    c = np.zeros((n_sections, 2, 3), np.float64)
    for k in range(n_sections):
        r, th = rng.uniform(0.3, 0.85), rng.uniform(0.2, 2.8)
        rz = rng.uniform(0.3, 0.85)
        c[k, 1] = [0.0, -2 * r * math.cos(th), r * r]
        c[k, 0] = [1.0, -2 * rz * math.cos(th), rz * rz]
        c[k, 0] *= rng.uniform(0.7, 1.2)
    return c
