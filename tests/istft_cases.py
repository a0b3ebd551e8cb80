"""STFT synthesis (jdsp_istft) on the spectra white noise does not reach (not a test module): the cases, two
restatements and the bars that test_istft_hard_cpu.py (CPU) and test_istft_hard_gpu.py (device) share.

  restate (test_istft_gpu.py)     the header's steps in FP64: the truth every comparison is against, computed from the
                                  stored complex64 values
  restate32(...)                  the same steps in plain FP32: Hermitian part, the radix-2 ifft_r2 of denoise_fp32_ref.py
                                  on complex64, 1/n, synthesis window, overlap-add in ascending frame order, gain -- what
                                  FP32 alone makes of a case, NOT what the device is compared with
  bars_of(...), truth(ci)         per sample: the stream bar 1e-5 P g (P the largest windowed sample of any frame, as
                                  test_istft_gpu.py) and the frame bar 1e-5 g sum_f P_f |w_s[t - hop f]| over the frames
                                  whose support holds t, P_f = max_i |y_f[i]| before the synthesis window.  The frame bar
                                  is built from the frames that add into a sample and not from their sum: frames may
                                  cancel in the overlap, and the FP32 overlap-add the header specifies cannot do better
                                  than its terms.

1e-5 is the project's figure; plain radix-2 FP32 against each frame's own peak gives 0.020-0.025 of it on single bins, an
off-bin tone, a square, an impulse and white noise at n = 512 and 1024.

Admission of a case: restate32 stays at or under ADMIT = 0.25 of both bars on it (test_istft_hard_cpu.py asserts it for
every case).  The bars are never widened; a case that does not meet the rule is redesigned, and the reason stands beside
it.  Every case keeps |g s| <= LIMIT, so the int16 rules hold on every sample with no exclusions; fit() scales a stream
to that.  The power-of-two scaled runs and the non-finite runs are built from cases here (scaled(), poisoned()) and are
checked in float32.

Families (the `fam` of a case):
   1  basis sweep: one row per bin, and (FULL) rows with only X[k] or only X[n - k] set
   2  shaped single frames, R - 1 zero rows behind each: DC, Nyquist, both, flat, flat with linear phase, an off-bin
      tone, a square
   3  non-Hermitian FULL rows X = H + c A, c in {1, 1e3, 1e4}, and a purely anti-Hermitian row between two ordinary ones
   4  loud frames alternating with the same kind of frame 60, 80 and 120 dB lower (white; the off-bin tone)
   5  frames 8..15 loud, the rest 80 dB lower
   6  zero rows: an all-zero stream; at hop = n zero rows among loud ones
   7  one fixed row, isolated by R - 1 zero rows on each side, at several positions next to runs of loud frames
   9  the clean twin (run B) of a stream with one non-finite value: row f zero; poisoned() makes run A
  10  the white control: the rows and seeds of test_istft_gpu.py::test_against_restatement at F = 37
Family 8 (power-of-two scale) is the cases marked `scale`, run through scaled().
"""
import functools

import numpy as np

import denoise_fp32_ref as D
from test_istft_gpu import CONFIGS, WINDOWS, cast_i16, hermitian, restate, rows, window, wola_den  # noqa: F401

F32 = np.float32
C64 = np.complex64
TOL = 1e-5
ADMIT = 0.25
LIMIT = 32000.0
LOUD = 30000.0
LAYOUTS = ("full", "half")
SCALES = (-60, 60)
TINY = float(np.finfo(F32).tiny)


def bins_of(n, layout):
    return n if layout == "full" else n // 2 + 1


def pairs_of(n, hop):
    """The window pairs (synthesis = analysis) create accepts at (n, hop): Hann / Hann has no WOLA inverse at hop = n."""
    out = []
    for w in WINDOWS:
        den = wola_den(n, hop, w, w)
        if den.min() >= 1e-6 * den.max():
            out.append(w)
    return out


# ---- the FP32 restatement ----------------------------------------------------------------------------------------------
def hermitian32(spec, n, layout):
    x = np.asarray(spec, C64)
    if layout == "full":
        x = x[:, :n]
        m = np.conj(x[:, (-np.arange(n)) % n])
        return ((x + m).astype(C64) * F32(0.5)).astype(C64)
    x = x[:, :n // 2 + 1].copy()
    x[:, 0] = x[:, 0].real
    x[:, n // 2] = x[:, n // 2].real
    return np.concatenate([x, np.conj(x[:, n // 2 - 1:0:-1])], axis=1).astype(C64)


def restate32(spec, n, hop, layout="full", syn="none", ana="none", steps=None):
    """Emitted samples and tail as one float32 array, every operation in FP32.  steps: a list that receives every
    intermediate array (the Hermitian part, the transform, the scaled and the windowed frames, the sums, the output)."""
    h = hermitian32(spec, n, layout)
    z = D.ifft_r2(h)
    assert z.dtype == C64
    y = (z.real * F32(1.0 / n)).astype(F32)
    yw = (y * window(syn, n).astype(F32)).astype(F32)
    F = yw.shape[0]
    s = np.zeros(hop * F + n - hop, F32)
    for f in range(F):
        s[hop * f: hop * f + n] += yw[f]
    g = (1.0 / wola_den(n, hop, syn, ana)).astype(F32)
    out = (s * np.resize(g, s.size)).astype(F32)
    if steps is not None:
        steps.extend([h.real, h.imag, z.real, z.imag, y, yw, s, out])
    return out


# ---- the bars ----------------------------------------------------------------------------------------------------------
def bars_of(spec, n, hop, layout, syn, ana):
    """(want [hop F + n - hop], stream bar, frame bar) of a stream in FP64"""
    em, tail, peak, g = restate(spec, n, hop, layout, syn, ana)
    want = np.concatenate([em, tail])
    gg = np.resize(g, want.size)
    y = np.real(np.fft.ifft(hermitian(spec, n, layout), axis=1))
    pf = np.abs(y).max(axis=1) if y.shape[0] else np.zeros(0)
    ws = np.abs(window(syn, n))
    acc = np.zeros(want.size)
    for f in range(y.shape[0]):
        acc[hop * f: hop * f + n] += pf[f] * ws
    return want, TOL * peak * gg, TOL * gg * acc


def window_sum(n, hop, syn):
    """The largest sum_f |w_s[t - hop f]| a sample can see."""
    return np.abs(window(syn, n)).reshape(n // hop, hop).sum(axis=0).max()


def frame_peaks(spec, n, layout):
    """P_f, before the synthesis window (FP64)."""
    return np.abs(np.real(np.fft.ifft(hermitian(spec, n, layout), axis=1))).max(axis=1)


def ratios_of(got, bars):
    """Worst |got - want| over each bar: (of the stream bar, of the frame bar); an error under a zero bar is inf."""
    want, stream_bar, frame_bar = bars
    err = np.abs(np.asarray(got, np.float64) - want)
    out = []
    for bar in (stream_bar, frame_bar):
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / bar)
        out.append(float(q.max()) if q.size else 0.0)
    return tuple(out)


def cfg_of_case(c):
    return dict(n_fft=c["n"], hop=c["hop"], layout=c["layout"], synthesis_window=c["syn"], analysis_window=c["ana"])


def geo(c):
    return c["n"], c["hop"], c["layout"], c["syn"], c["ana"]


@functools.lru_cache(maxsize=None)
def truth(ci):
    """bars_of case ci, computed once and shared (read-only)."""
    c = cases()[ci]
    out = bars_of(c["spec"], *geo(c))
    for a in out:
        a.setflags(write=False)
    return out


def ratios(got, ci):
    return ratios_of(got, truth(ci))


# ---- building blocks ---------------------------------------------------------------------------------------------------
def _layout(H, n, layout):
    """A Hermitian [F, n] spectrum in the layout's bins"""
    return H if layout == "full" else H[:, :n // 2 + 1]


def _white(rng, F, n):
    """Hermitian spectra of F real white frames of unit variance"""
    return np.fft.fft(rng.normal(size=(F, n)), axis=1)


def _tone(rng, F, n):
    """Hermitian spectra of F frames of a tone off its bin (64.37 cycles per frame), each at its own phase"""
    ph = rng.uniform(0, 2 * np.pi, (F, 1))
    return np.fft.fft(np.sin(2 * np.pi * 64.37 * np.arange(n)[None, :] / n + ph), axis=1)


def fit(X, n, hop, layout, syn, ana, target=LOUD):
    """X (complex128) scaled so that the largest |g s| of its stream is `target`, as complex64"""
    em, tail, _, _ = restate(X, n, hop, layout, syn, ana)
    top = np.abs(np.concatenate([em, tail])).max()
    return (np.asarray(X, np.complex128) * (target / top if top > 0 else 1.0)).astype(C64)


def _case(out, fam, name, n, hop, layout, win, spec, **extra):
    spec = np.ascontiguousarray(spec, C64)
    assert spec.ndim == 2 and spec.shape[1] >= bins_of(n, layout)
    c = dict(name="%s-%d-%d-%s-%s" % (name, n, hop, layout, win), fam=fam, n=n, hop=hop, layout=layout, syn=win, ana=win,
             spec=spec, F=spec.shape[0], scale=False, poison=None, poison_mid=None, zero_rows=(), positions=(), fixed=False)
    c.update(extra)
    assert c["fixed"] or 24 <= c["F"] <= 40, (c["name"], c["F"])
    spec.setflags(write=False)
    out.append(c)
    return c


def _shapes(n):
    """Family 2: (name, Hermitian row [n] in FP64, relative level).  Every frame's peak before the window is its
    level; the impulses stand at half the level of the rest, so that no frame's peak before the window exceeds the
    stream's largest windowed sample (the frame bar then stays under the stream bar times the window sum)."""
    k = np.arange(n)
    out = []

    def bin_row(pairs):
        r = np.zeros(n, np.complex128)
        for b, v in pairs:
            r[b] = v
        return r

    out.append(("dc", bin_row([(0, n)]), 1.0))
    out.append(("nyquist", bin_row([(n // 2, n)]), 1.0))
    out.append(("dc+nyquist", bin_row([(0, n / 2), (n // 2, n / 2)]), 1.0))
    out.append(("flat", np.ones(n, np.complex128), 0.5))
    for p in (1, n // 2 - 1, n // 2, n // 2 + 1, n - 1):
        out.append(("flat@%d" % p, np.exp(-2j * np.pi * k * p / n), 0.5))
    out.append(("tone", np.fft.fft(np.sin(2 * np.pi * 64.37 * k / n + 0.3)), 1.0))
    out.append(("square", np.fft.fft(np.where((k // 32) % 2 == 0, 1.0, -1.0)), 1.0))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """Every case: dicts {name, fam, n, hop, layout, syn, ana, spec complex64 [F, pitch], F, scale, poison, poison_mid,
    zero_rows, positions, fixed}.  The same list, in the same order, whoever asks."""
    out = []
    combos = [(n, hop, layout) for n, hop in CONFIGS for layout in LAYOUTS]

    def win_of(fam, ci, n, hop):
        p = pairs_of(n, hop)
        return p[(fam + ci + ci // 2) % len(p)]

    # 1. the basis sweep.  1500 n e^{0.7j}: a cosine of amplitude 3000 (1500 at DC and Nyquist, which take the real
    # value).  No window at hop = n (each row its own block; Hamming / Hamming there has a gain of up to 156 at the
    # frame's ends and would pass LIMIT), Hamming at n/2, Hann at n/4.
    for n, hop, layout in combos:
        win = {1: "none", 2: "hamming", 4: "hann"}[n // hop]
        amp = 1500.0 * n * np.exp(0.7j)
        parts = []
        pair = np.zeros((n // 2 + 1, n), np.complex128)
        for k in range(n // 2 + 1):
            if k in (0, n // 2):
                pair[k, k] = amp.real
            else:
                pair[k, k], pair[k, n - k] = amp, np.conj(amp)
        parts.append(_layout(pair, n, layout))
        if layout == "full":                                   # one-sided rows: the truth is half the amplitude
            lower = np.zeros((n // 2 + 1, n), np.complex128)
            lower[np.arange(n // 2 + 1), np.arange(n // 2 + 1)] = amp
            upper = np.zeros((n // 2 - 1, n), np.complex128)
            upper[np.arange(n // 2 - 1), n - np.arange(1, n // 2)] = amp
            parts += [lower, upper]
        _case(out, 1, "basis", n, hop, layout, win, np.concatenate(parts).astype(C64), fixed=True)

    # 2. shaped single frames, R - 1 zero rows behind each; at R = 4 in two streams (eleven shapes do not fit 40 frames).
    # A stream cycles through its shapes until it has 24 frames, later passes at -1/2 and 1/4 of the level.
    for ci, (n, hop, layout) in enumerate(combos):
        R = n // hop
        shapes = _shapes(n)
        for part, chunk in enumerate([shapes] if R < 4 else [shapes[:6], shapes[6:]]):
            m = max(len(chunk), -(-24 // R))
            X = np.zeros((m * R, n), np.complex128)
            for i in range(m):
                _, row, level = chunk[i % len(chunk)]
                X[i * R] = row * level * (1.0, -0.5, 0.25)[i // len(chunk)]
            win = win_of(2, ci, n, hop)
            _case(out, 2, "shapes%s" % ("ab"[part] if R == 4 else ""), n, hop, layout, win,
                  fit(_layout(X, n, layout), n, hop, layout, win, win))

    # 3. non-Hermitian rows, FULL only: X = H + c A, A anti-Hermitian white of H's RMS, c cycling through 1, 1e3, 1e4.
    # Row 11 is purely anti-Hermitian (exactly: the upper half is the negated conjugate of the lower, bit for bit)
    # between the ordinary rows 10 and 12.
    for ci, (n, hop) in enumerate(CONFIGS):
        rng = np.random.default_rng([2811, 3, ci])
        F = 30
        H, A = _white(rng, F, n), 1j * _white(rng, F, n)
        c = np.array([(1.0, 1e3, 1e4)[f % 3] for f in range(F)])[:, None]
        c[10], c[12] = 0.0, 0.0
        win = win_of(3, 2 * ci, n, hop)
        Hs = fit(H, n, hop, "full", win, win).astype(np.complex128)
        k = float(np.abs(Hs).max() / np.abs(H).max())
        X = (Hs + c * k * A).astype(C64)
        a = (1e4 * k * A[11]).astype(C64)
        a[n // 2 + 1:] = -np.conj(a[n // 2 - 1:0:-1])
        a[0], a[n // 2] = 1j * a[0].imag, 1j * a[n // 2].imag
        X[11] = a
        _case(out, 3, "nonherm", n, hop, "full", win, X, zero_rows=(11,))

    # 4. loud beside quiet: even frames loud, odd frames the same kind 60, 80 and 120 dB lower in turn
    for ci, (n, hop, layout) in enumerate(combos):
        for ki, (kind, make) in enumerate((("white", _white), ("tone", _tone))):
            rng = np.random.default_rng([2811, 4, ci, ki])
            F = 30
            X = make(rng, F, n)
            X /= frame_peaks(X, n, "full")[:, None]
            level = np.array([1.0 if f % 2 == 0 else 10.0 ** (-(60, 80, 120)[(f // 2) % 3] / 20.0) for f in range(F)])
            win = win_of(4 + ki, ci, n, hop)
            _case(out, 4, "loudquiet_" + kind, n, hop, layout, win,
                  fit(_layout(X * level[:, None], n, layout), n, hop, layout, win, win), scale=True)

    # 5. a loud stretch: frames 8..15 loud, the rest 80 dB lower
    for ci, (n, hop, layout) in enumerate(combos):
        rng = np.random.default_rng([2811, 5, ci])
        F = 26
        X = _white(rng, F, n)
        X /= frame_peaks(X, n, "full")[:, None]
        level = np.where((np.arange(F) >= 8) & (np.arange(F) < 16), 1.0, 1e-4)
        win = win_of(5, ci, n, hop)
        _case(out, 5, "stretch", n, hop, layout, win, fit(_layout(X * level[:, None], n, layout), n, hop, layout, win, win))

    # 6. zero rows: an all-zero stream everywhere; at hop = n zero rows among loud ones
    for ci, (n, hop, layout) in enumerate(combos):
        win = win_of(6, ci, n, hop)
        _case(out, 6, "zeros", n, hop, layout, win, np.zeros((24, bins_of(n, layout)), C64), zero_rows=tuple(range(24)))
        if hop == n:
            rng = np.random.default_rng([2811, 6, ci])
            zero = (0, 3, 4, 9, 17, 23)
            X = _white(rng, 24, n)
            X[list(zero)] = 0
            _case(out, 6, "zeros_among_loud", n, hop, layout, win, fit(_layout(X, n, layout), n, hop, layout, win, win),
                  zero_rows=zero)

    # 7. position and neighbours: the row r (a white frame at 0.3 of the loud level) with R - 1 zero rows on each side,
    # after loud runs of 3, 5, 2, 4, 1, ... frames until the stream has 24 frames
    for ci, (n, hop, layout) in enumerate(combos):
        R = n // hop
        rng = np.random.default_rng([2811, 7, ci])
        r = _white(rng, 1, n)
        r *= 0.3 / frame_peaks(r, n, "full")[0]
        blocks, pos, at = [], [], 0
        for run in (3, 5, 2, 4, 1, 3, 5, 2):
            loud = _white(rng, run, n)
            loud /= frame_peaks(loud, n, "full")[:, None]
            blocks += [loud, np.zeros((R - 1, n)), r, np.zeros((R - 1, n))]
            pos.append(at + run + R - 1)
            at += run + 2 * R - 1
            if at >= 24:
                break
        win = win_of(7, ci, n, hop)
        _case(out, 7, "position", n, hop, layout, win,
              fit(_layout(np.concatenate(blocks), n, layout), n, hop, layout, win, win), positions=tuple(pos))

    # 9. the clean twin of a stream with one non-finite value: white rows, row f zero, f in the middle of the stream,
    # near its start and its last row.  poison = (f, bin, part, value), in turn a NaN and a +Inf.  "No sample of the
    # frame stays finite" is a statement about the inverse transform only where the poisoned component has a weight
    # other than zero in every sample: the real part of X[k] enters sample i with cos(2 pi k i / n), the imaginary part
    # with -sin(2 pi k i / n), and an inverse may add a term of weight exactly zero as 0 * NaN or leave it out (a
    # butterfly turns by +-j with a swap, not a product).  The sine vanishes at i = 0 for every k; the cosine vanishes
    # nowhere only for k = 0 and k = n/2.  So `poison` stands in the real part of bin 0 or n/2 and is held to the
    # statement as it stands, and `poison_mid` puts the value into a bin in between, real or imaginary part, and is
    # held to it wherever the weight is not zero (zero_weight()); where it is zero the sample is non-finite or equals
    # the clean twin's bit for bit.
    for ci, (n, hop, layout) in enumerate(combos):
        rng = np.random.default_rng([2811, 9, ci])
        F = 24
        f = (11, 1, F - 1)[ci % 3]
        X = _white(rng, F, n)
        X[f] = 0
        win = win_of(9, ci, n, hop)
        poison = (f, (0, n // 2)[(ci + ci // 4) % 2], "real", (np.nan, np.inf)[(ci // 2) % 2])
        mid = (f, (37, n // 2 - 1, 1, 64)[ci % 4], ("real", "imag")[(ci // 2) % 2], (np.nan, np.inf)[(ci + ci // 2) % 2])
        _case(out, 9, "twin", n, hop, layout, win, fit(_layout(X, n, layout), n, hop, layout, win, win, 20000.0),
              poison=poison, poison_mid=mid, zero_rows=(f,))

    # 10. the white control: test_istft_gpu.py::test_against_restatement draws one stream per (synthesis, analysis)
    # pair from one generator; the pairs with equal windows that create accepts are kept.  Hamming / Hamming at hop = n
    # is left out: its gain reaches 156 at a frame's ends and these rows then pass LIMIT (that test excludes samples
    # and compares modulo the wrap; these do neither).
    for ci, (n, hop, layout) in enumerate(combos):
        rng = np.random.default_rng(n + hop)
        pitch = n if layout == "full" else n // 2 + 1 + 3
        for syn in WINDOWS:
            for ana in WINDOWS:
                spec = rows(rng, 37, n, pitch)
                if syn != ana or syn not in pairs_of(n, hop) or (hop == n and syn == "hamming"):
                    continue
                _case(out, 10, "white", n, hop, layout, syn, spec, scale=syn == win_of(10, ci, n, hop) or hop == n)
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def index_of(name):
    return [c["name"] for c in cases()].index(name)


def scaled(spec, k):
    """Every value times 2^k, exactly"""
    return np.ldexp(np.ascontiguousarray(spec, C64).view(F32), k).astype(F32).view(C64)


# Family 8.  A case marked `scale` runs with every spectrum value times 2^-60 and times 2^+60; the float32 output must
# be the unscaled one times the same power of two, bit for bit.  The condition for a run is that restate32 has that
# property on it and that none of its intermediate values is subnormal or infinite (scale_admitted(); asserted for every
# run by test_istft_hard_cpu.py).  Every marked case meets it at 2^+60 and the white control at 2^-60 too.  Of the
# loud-beside-quiet streams only these meet it at 2^-60: in the others a product inside the radix-2 transform of a frame
# 120 dB down (values near 2e-19 after the scaling, their rounding residues far lower) underflows, so the scaling is no
# longer exact in plain FP32 and the case says nothing about the kernel.  The CPU test asserts that the others do fail
# the condition, so the list cannot go stale.
DOWN_OK = ("loudquiet_white-1024-512-full-hamming", "loudquiet_white-1024-512-half-hann",
           "loudquiet_white-1024-256-full-hamming", "loudquiet_white-1024-256-half-hann",
           "loudquiet_white-512-512-half-none", "loudquiet_white-512-256-full-hamming",
           "loudquiet_white-512-128-full-hamming")


def scale_runs(admitted=True):
    """(case index, exponent) of family 8's runs; admitted=False: the 2^-60 runs left out"""
    out = []
    for i, c in enumerate(cases()):
        if c["scale"]:
            for k in SCALES:
                if (k > 0 or c["fam"] != 4 or c["name"] in DOWN_OK) == admitted:
                    out.append((i, k))
    return out


def scale_admitted(c, k):
    """The condition of a family-8 run on restate32: exact scaling, no intermediate value subnormal or infinite"""
    base = restate32(c["spec"], *geo(c))
    steps = []
    try:
        with np.errstate(under="raise", over="raise"):
            got = restate32(scaled(c["spec"], k), *geo(c), steps=steps)
    except FloatingPointError:
        return False
    for a in steps:
        a = np.abs(a[a != 0])
        if a.size and not (a.min() >= TINY and np.isfinite(a.max())):
            return False
    return np.array_equal(got.view(np.int32), np.ldexp(base, k).astype(F32).view(np.int32))


def poisoned(c, which="poison"):
    """Run A of a family-9 case: its spectrum with the one non-finite value in row f"""
    f, b, part, v = c[which]
    spec = np.array(c["spec"])
    if part == "real":
        spec[f, b] = complex(v, 0.0)
    else:
        spec[f, b] = complex(0.0, v)
    return spec


def zero_weight(n, b, part):
    """bool [n]: the samples of a frame into which the real (imaginary) part of X[b] enters with weight exactly zero,
    cos(2 pi b i / n) (sin(2 pi b i / n)), in integer arithmetic"""
    q = 4 * b * np.arange(n)                                   # the angle in quarter turns is q / n
    whole = q % n == 0
    turns = q // n
    return whole & (turns % 2 == 1) if part == "real" else whole & (turns % 2 == 0)


def subset():
    """Case indices for the bit-identity checks: for every (n, hop, layout) two cases, so that every family is in"""
    by = {}
    for i, c in enumerate(cases()):
        by.setdefault((c["n"], c["hop"], c["layout"]), {}).setdefault(c["fam"], i)
    fams = [4, 2, 5, 3, 7, 9, 6, 10, 1]
    out, k = [], 0
    for key in sorted(by):
        have = [f for f in fams if f in by[key] and (f != 1 or key[1] == key[0])]
        for j in range(2):
            out.append(by[key][have[(k + j * 4) % len(have)]])
        k += 1
    got = {cases()[i]["fam"] for i in out}
    for f in fams:                                             # a family the rotation missed
        if f not in got:
            out.append(next(i for i, c in enumerate(cases()) if c["fam"] == f and (f != 1 or c["hop"] == c["n"])))
    return sorted(set(out))
