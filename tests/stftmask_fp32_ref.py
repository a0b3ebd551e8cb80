"""Fused STFT masking on the inputs where transform rounding shows (not a test module): a mask that removes something
loud and keeps something faint.  The streams, their masks, two restatements and the bars that
test_stftmask_fp32_ref_cpu.py (CPU) and test_stftmask_suppress_gpu.py (device) share.

  restate (test_stftmask_gpu.py)      header steps 1-5 in FP64: the truth every comparison is against
  restate32(...)                      the same steps in plain FP32: window, the radix-2 fft_r2 / ifft_r2 of
                                      denoise_fp32_ref.py on complex64, mask multiply, 1/n, synthesis window and
                                      overlap-add (frames in ascending order), gain -- what FP32 alone makes of a stream
  bars_of(...), truth(ci)             per sample: the stream bar 1e-5 P g and the local bar 1e-5 g max|s| over the
                                      hop-blocks b - (R-1) .. b + (R-1) (the blocks the frames that touch b cover)
  criterion(case)                     the kernels' per-frame figure rho (stftmask_kernels.hip, stftmask_unsafe)

Why FP32 is not enough.  The forward transform rounds every bin by about 2^-23 sqrt(E), E = sum (w_a x)^2 the frame's
energy, wherever the energy sits.  A mask that passes the bins of a faint part and zeroes a loud one passes that
rounding too: in the output it is 2^-23 sqrt(E mean|M|^2 / n) per sample, against an output of sqrt(sum y^2 / n).  So

    rho = 2^-23 sqrt(E mean|M|^2 / sum y^2),    mean|M|^2 over all n bins, y the frame before the synthesis window

predicts a frame's error relative to its own output, up to the constant of the transform and the crest factors.  White
input under a mask of order one has rho near 2^-23 = 1.2e-7; a part 60 dB under a suppressed one 1.2e-4.  The kernels
compute a frame with rho > RHO again in FP64.
"""
import functools

import numpy as np

import denoise_fp32_ref as D
from test_stftmask_gpu import BINS, LIMIT, N, cast_i16, gain, mask_of, pcm_of, restate, stream_combo, window  # noqa: F401

F32 = np.float32
C64 = np.complex64
TOL = 1e-5
# The kernels' threshold on rho (JDSP_STFTMASK_RHO in stftmask_kernels.hip).  rho predicts a frame's error relative to
# its own output; half the bar is what a frame may use where two frames meet in a block.  Over every frame of cases()
# the smallest rho of a frame whose plain-FP32 error exceeds half its local bar is 8.4e-6 (40 dB under a notched tone),
# but a frame without an analysis window under the 1 / w_s gain of hop 1024 is at 0.29 of the bar with rho = 1.0e-6
# already (the tone off its bin leaks past the notch, and the leak sits at the frame's edges, where w_s is small).
# RHO leaves a factor RHO_MARGIN to the first and keeps the second's extrapolation to half the bar (1.7e-6) above it
# by the same factor; the largest rho of a white-control frame is 1.26e-7, six times under it
# (test_stftmask_fp32_ref_cpu.py asserts all three).
RHO = 8.0e-7
RHO_MARGIN = 2.0
LOUD = 30000.0


# ---- the FP32 restatement ----------------------------------------------------------------------------------------------
def _rows(mask, F, ctype):
    M = np.asarray(mask).astype(ctype)
    M = np.broadcast_to(M[None, :BINS], (F, BINS)) if M.ndim == 1 else M[:F, :BINS]
    M = M.copy()
    M[:, 0] = M[:, 0].real                                     # Im of M[0], M[n/2] ignored
    M[:, N // 2] = M[:, N // 2].real
    return M


def frames32(pcm, mask, F, hop, ana):
    """Per frame in plain FP32: (y [F, N] before the synthesis window, E [F] = sum (w_a x)^2)."""
    wa = window(ana).astype(F32)
    x = (np.stack([pcm[hop * f: hop * f + N] for f in range(F)]).astype(F32) * wa).astype(F32)
    X = D.fft_r2(x.astype(C64))[:, :BINS]
    Y = (_rows(mask, F, C64) * X).astype(C64)
    Y[:, 0] = Y[:, 0].real
    Y[:, N // 2] = Y[:, N // 2].real
    H = np.concatenate([Y, np.conj(Y[:, N // 2 - 1:0:-1])], axis=1).astype(C64)
    y = (D.ifft_r2(H).real.astype(F32) * F32(1.0 / N)).astype(F32)
    return y, (x.astype(np.float64) ** 2).sum(axis=1)


def overlap_add32(y, F, hop, ana, syn, normalise):
    y = (y.astype(F32) * window(syn).astype(F32)).astype(F32)
    s = np.zeros(hop * F + N - hop, F32)
    for f in range(F):
        s[hop * f: hop * f + N] += y[f]
    return (s * np.resize(gain(hop, ana, syn, normalise).astype(F32), s.size)).astype(np.float64)


def restate32(pcm, mask, F, hop, ana, syn, normalise):
    """Emitted samples and tail as one float64 array, every operation in FP32."""
    y, _ = frames32(pcm, mask, F, hop, ana)
    return overlap_add32(y, F, hop, ana, syn, normalise)


def mask_mean_sq(mask, F):
    """mean |M|^2 over all n bins of the Hermitian-extended row (bins 0 and n/2 by their real parts)."""
    p = np.abs(_rows(mask, F, np.complex128)) ** 2
    return (p[:, 0] + p[:, N // 2] + 2.0 * p[:, 1:N // 2].sum(axis=1)) / N


def criterion(c):
    """rho per frame from the plain-FP32 restatement's own sums; 0 where the mask row is zero (the output is exact)."""
    y, e = frames32(c["pcm"], c["mask"], c["F"], c["hop"], c["combo"][0])
    num = e * mask_mean_sq(c["mask"], c["F"])
    den = (y.astype(np.float64) ** 2).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 2.0 ** -23 * np.sqrt(num / den)
    return np.where(num == 0, 0.0, np.where(np.isnan(r), np.inf, r))


# ---- the bars ----------------------------------------------------------------------------------------------------------
def bars_of(pcm, mask, F, hop, combo):
    """(want [hop F + N - hop], stream bar, local bar) of a stream in FP64"""
    R = N // hop
    em, tail, P, g = restate(pcm, mask, F, hop, *combo)
    want = np.concatenate([em, tail])
    gg = np.resize(g, want.size)
    pk = np.abs(want / gg).reshape(-1, hop).max(axis=1)            # F + R - 1 hop-blocks, un-normalised
    loc = np.array([pk[max(0, b - (R - 1)): b + R].max() for b in range(pk.size)])
    return want, TOL * P * gg, TOL * np.repeat(loc, hop) * gg


@functools.lru_cache(maxsize=None)
def truth(ci):
    """bars_of case ci, computed once and shared (read-only)."""
    c = cases()[ci]
    out = bars_of(c["pcm"], c["mask"], c["F"], c["hop"], c["combo"])
    for a in out:
        a.setflags(write=False)
    return out


def ratios_of(got, bars):
    """Worst |got - want| over each bar: (of the stream bar, of the local bar); an error under a zero bar is inf."""
    want, stream_bar, local_bar = bars
    err = np.abs(np.asarray(got, np.float64) - want)
    out = []
    for bar in (stream_bar, local_bar):
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / bar)
        out.append(float(q.max()))
    return tuple(out)


def ratios(got, ci):
    return ratios_of(got, truth(ci))


def frame_ratios(y_got, y_want, ci):
    """Per frame: the frame's own error (after the synthesis window and the gain) over the smallest local bar of the
    samples it adds into, sample by sample -- the share of a block's bar one frame uses."""
    c = cases()[ci]
    hop, F = c["hop"], c["F"]
    _, _, local_bar = truth(ci)
    ws = window(c["combo"][1])
    gg = np.resize(gain(hop, *c["combo"]), local_bar.size)
    out = np.zeros(F)
    for f in range(F):
        sl = slice(hop * f, hop * f + N)
        err = np.abs(y_got[f] - y_want[f]) * ws * gg[sl]
        with np.errstate(divide="ignore", invalid="ignore"):
            out[f] = np.where(err == 0, 0.0, err / local_bar[sl]).max()
    return out


def frames64(c):
    """The FP64 frames before the synthesis window (restate's steps 1-3 per frame)."""
    hop, F = c["hop"], c["F"]
    x = np.stack([c["pcm"][hop * f: hop * f + N] for f in range(F)]).astype(np.float64) * window(c["combo"][0])
    Y = _rows(c["mask"], F, np.complex128) * np.fft.fft(x, axis=1)[:, :BINS]
    Y[:, 0] = Y[:, 0].real
    Y[:, N // 2] = Y[:, N // 2].real
    return np.fft.irfft(Y, n=N, axis=1)


# ---- streams -----------------------------------------------------------------------------------------------------------
def _n(F, hop):
    return hop * (F - 1) + N


def _mix(loud, target):
    """int16 of loud + target; nothing clips, so the loud part stays what its name says"""
    s = np.asarray(loud, np.float64) + target
    assert np.abs(s).max() <= 32767.0, np.abs(s).max()
    return np.rint(s).astype(np.int16)


def _pass(kind):
    """The pass value of a mask: 1, or for a complex mask a delay of three samples (|M| = 1 at every bin)"""
    if kind == "real":
        return np.ones(BINS, F32)
    return np.exp(-2j * np.pi * 3 * np.arange(BINS) / N).astype(C64)


def _notch(kind, zero_bins):
    m = _pass(kind)
    m[np.asarray(sorted(set(b for b in zero_bins if 0 <= b < BINS)), np.int64)] = 0
    return m


def _band_noise(rng, n, top_bin, peak):
    """White noise with nothing at or above top_bin (of N), by a brick wall over the whole stream"""
    Z = np.fft.rfft(rng.normal(size=n))
    Z[int(np.ceil(top_bin * n / N)):] = 0
    x = np.fft.irfft(Z, n=n)
    return peak * x / np.abs(x).max()


def _case(name, hop, kind, pcm, mask, F, pitch=None, white=False, level=None, span=None):
    combo = stream_combo(hop)
    mask = np.ascontiguousarray(mask)
    assert mask.dtype == (F32 if kind == "real" else C64) and pcm.dtype == np.int16 and pcm.size == _n(F, hop)
    assert 24 <= F <= 40 and (mask.ndim == 1) == (pitch == 0)
    c = dict(name="%s-%d-%s" % (name, hop, kind), hop=hop, kind=kind, combo=combo, pcm=pcm, mask=mask, F=F,
             mask_pitch=mask.shape[1] if mask.ndim == 2 else 0, white=white, level=level, span=span)
    pcm.setflags(write=False)
    mask.setflags(write=False)
    return c


def _spectra(x, F, hop, ana):
    fr = np.stack([x[hop * f: hop * f + N] for f in range(F)]).astype(np.float64) * window(ana)
    return np.fft.fft(fr, axis=1)[:, :BINS]


@functools.lru_cache(maxsize=None)
def cases():
    """Every stream of the suppressing-mask tests: dicts {name, hop, kind, combo, pcm, mask, mask_pitch, F, white, level
    (dB the kept part lies under the removed one, or None), span}.  The same list, in the same order, whoever asks."""
    out = []
    k = 0
    harmonics = [16 * h + d for h in range(1, 64, 2) for d in (-2, -1, 0, 1, 2)]
    spread = {"notch_on": ((512, "real"), (256, "complex"), (1024, "real")),
              "notch_off": ((256, "real"), (1024, "complex"), (512, "real")),
              "comb_square": ((1024, "complex"), (512, "complex"), (256, "real")),
              "band_split": ((256, "complex"), (512, "real"), (512, "complex"))}
    for fam in ("notch_on", "notch_off", "comb_square", "band_split"):
        for li, (level, sigma) in enumerate(((40, 300.0), (60, 30.0), (80, 3.0))):
            hop, kind = spread[fam][li]
            k += 1
            F = 24 + (5 * k) % 17
            n = _n(F, hop)
            rng = np.random.default_rng([2207, k])
            if fam == "notch_on":
                loud, zero = LOUD * np.sin(2 * np.pi * 64 * np.arange(n) / N), range(61, 68)
            elif fam == "notch_off":
                loud, zero = LOUD * np.sin(2 * np.pi * 64.37 * np.arange(n) / N + 0.3), range(52, 77)
            elif fam == "comb_square":
                loud, zero = np.where((np.arange(n) // 32) % 2 == 0, LOUD, -LOUD), harmonics
            else:
                loud, zero = _band_noise(rng, n, 128, LOUD), range(0, 136)
            pcm = _mix(loud, rng.normal(0.0, sigma, n))
            out.append(_case("%s_%ddB" % (fam, level), hop, kind, pcm, np.tile(_notch(kind, zero), (F, 1)), F, level=level))
    # ratio masks over a vowel, the target 60 dB under it
    for name, hop, kind in (("ratio", 512, "real"), ("cratio", 256, "complex")):
        F = 30
        n = _n(F, hop)
        rng = np.random.default_rng([2207, 100 + hop])
        I = D.vowel(rng, n, 12000.0).astype(np.float64)
        T = rng.normal(0.0, I.std() / 1000.0, n)
        st, si = _spectra(T, F, hop, stream_combo(hop)[0]), _spectra(I, F, hop, stream_combo(hop)[0])
        if kind == "real":
            m = (np.abs(st) ** 2 / (np.abs(st) ** 2 + np.abs(si) ** 2)).astype(F32)
        else:
            m = st / (st + si)
            m = (m * np.minimum(1.0, 8.0 / np.maximum(np.abs(m), 1e-300)) * 0.99999).astype(C64)
            assert np.abs(m).max() <= 8.0
        out.append(_case(name + "_60dB", hop, kind, _mix(I, T), m, F, level=60))
    # a fixed equaliser: one row for every frame (the kernels keep it in registers)
    for hop, kind in ((512, "complex"), (256, "real")):
        F = 33
        n = _n(F, hop)
        rng = np.random.default_rng([2207, 200 + hop])
        pcm = _mix(LOUD * np.sin(2 * np.pi * 64 * np.arange(n) / N), rng.normal(0.0, 30.0, n))
        out.append(_case("fixed_eq_60dB", hop, kind, pcm, _notch(kind, range(61, 68)), F, pitch=0, level=60))
    # a boost of 1000 on bins that hold only the faint target, 1 elsewhere
    for hop, kind in ((256, "real"), (512, "complex")):
        F = 28
        n = _n(F, hop)
        rng = np.random.default_rng([2207, 300 + hop])
        m = _pass(kind)
        m[200:400] *= 1000
        pcm = _mix(_band_noise(rng, n, 128, 6000.0), rng.normal(0.0, 1.0, n))
        out.append(_case("boost", hop, kind, pcm, np.tile(m, (F, 1)), F, level=None))
    # an interferer in frames 8..15 only, suppressed only there; frame 16 (all ones) follows the loud stretch
    # directly.  The tone stops where frame 15 stops: frame 16 holds R - 1 hops of it and nothing removes them.
    for hop, kind in ((256, "real"), (512, "complex"), (1024, "real")):
        F = 26
        n = _n(F, hop)
        rng = np.random.default_rng([2207, 400 + hop])
        loud = 24000.0 * np.sin(2 * np.pi * 64 * np.arange(n) / N)    # passes unsuppressed at the edges: under LIMIT
        loud[:8 * hop] = 0
        loud[15 * hop + N:] = 0
        m = np.tile(_pass(kind), (F, 1))
        m[8:16] = _notch(kind, range(61, 68))
        out.append(_case("local", hop, kind, _mix(loud, rng.normal(0.0, 30.0, n)), m, F, level=60, span=(8, 16)))
    # all-zero mask over loud PCM: every output sample is exactly zero
    for hop, kind in ((512, "real"), (256, "complex")):
        F = 25
        rng = np.random.default_rng([2207, 500 + hop])
        out.append(_case("zero_mask", hop, kind, pcm_of(rng, F, hop, 8000.0), np.zeros((F, BINS), F32 if kind == "real" else C64), F))
    # the white control: the PCM and mask of test_stftmask_gpu.py::test_against_restatement at F = 37, same seeds
    for hop in (1024, 512, 256):
        for kind in ("real", "complex"):
            F = 37
            rng = np.random.default_rng(1000 * hop + 10 * F + len(kind))
            pcm, m = pcm_of(rng, F, hop), mask_of(rng, kind, F)
            out.append(_case("white", hop, kind, pcm, m, F, white=True))
    for c in out:
        try:
            restate(c["pcm"], c["mask"], c["F"], c["hop"], *c["combo"])   # asserts the output under LIMIT
        except AssertionError as e:
            raise AssertionError(c["name"], *e.args)
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def index_of(name):
    return [c["name"] for c in cases()].index(name)


# Cases whose plain-FP32 restatement misses a bar (test_stftmask_fp32_ref_cpu.py asserts exactly these, from the CPU
# run); on each of them the device must recompute at least one frame.
MISSING = ("notch_on_60dB-256-complex", "notch_on_80dB-1024-real", "notch_off_80dB-512-real", "comb_square_60dB-512-complex",
           "comb_square_80dB-256-real", "band_split_60dB-512-real", "band_split_80dB-512-complex", "ratio_60dB-512-real",
           "cratio_60dB-256-complex", "fixed_eq_60dB-512-complex", "fixed_eq_60dB-256-real", "boost-256-real",
           "boost-512-complex", "local-512-complex", "local-1024-real")
# Not missing although 60 dB under: notch_off_60dB-1024-complex (no analysis window at hop 1024: the tone off its bin
# leaks past any notch, so the output is loud: P = 26,287) and local-256-real (at R = 4 every block the eight
# suppressed frames cover has an unsuppressed, loud block within R - 1 of it, so both bars are loud).
