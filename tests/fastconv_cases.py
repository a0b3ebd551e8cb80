"""The overlap-save convolver on the streams white noise does not reach (not a test module): input families, filters,
the two bars and the int16 rules that test_fastconv_fp32_ref_cpu.py (CPU) and test_fastconv_streams_gpu.py (device)
share.

  family(name, shape)       seeded int16 streams of shape.n_blocks blocks: white, full-scale square, constant, full-scale
                            sines on and between the transform's bins, one impulse, silence, a loud stretch inside a
                            quiet stream, a loud tone over faint noise, a silent head followed by content
  FILTERS                   name -> (n_fft, taps [F, n_taps]); every row keeps 32768 sum|h| under 2^31 (past int32 the
                            cast is not specified)
  restate32(x, h, n_fft)    the same overlap-save in plain FP32: numpy's rfft on float32 segments, complex64 spectra,
                            never upcast -- what FP32 alone makes of a stream
  truth(filter, family)     the oracle's int16 and pre-cast streams and the two bars, computed once, read-only
  ratios_of(got, t)         the worst |got - w| as a fraction of each bar
  cast_i16, wrap_diff       the cast (truncate to int32, keep the low 16 bits: oracle/jdsp_oracle.c cast_i16, DESIGN §4,
                            frame_io.h cast_i16_bits) and the difference of two int16 values across a wrap

The bars, for the pre-cast output of one filter h, with B the block length, N = n_fft and w the oracle's pre-cast:

  global   |got - w| <= 1e-5 max(max|w|, 0.05 max|x| sum|h|)                    (test_fastconv_gpu.py's check())
  local    for output block e:  |got - w| <= 1e-5 max(max|w| over output blocks e-1 .. e+1,
                                                      0.05 max|x over the N input samples that end with block e's
                                                      last sample| sum|h|)
           samples before the stream's start count as zero; where that scale is 0, got must be exactly 0 (either sign)

0.05 |x|max sum|h| is the scale FP32 round-off of a segment lives on when the kept samples themselves are (nearly)
zero: sum|h| |x|max bounds every sample of the segment's circular convolution.  The local bar judges a quiet stretch
on its own scale, not on that of the stream's loudest stretch.
"""
import collections
import functools
import os

import numpy as np

TOL = 1e-5
FLOOR = 0.05
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

Shape = collections.namedtuple("Shape", "n_fft n_taps block hist_blocks n_blocks")


def shape_of(n_fft, n_taps, n_blocks=None):
    """The convolver's geometry and the stream length the family tests use: 24 blocks on the 1024-point transform
    (history + 177 where a block is shorter than 64 samples: 1024 taps give blocks of ONE sample and a history of 1023
    of them), history + 8 on the 8192-point one."""
    block = n_fft - n_taps + 1
    hist = -(-(n_taps - 1) // block)
    if n_blocks is None:
        n_blocks = hist + 8 if n_fft == 8192 else (24 if block >= 64 else hist + 177)
    return Shape(n_fft, n_taps, block, hist, n_blocks)


# ---- the cast ----------------------------------------------------------------------------------------------------------
def cast_i16(v):
    """oracle/jdsp_oracle.c cast_i16: truncate toward zero, keep the low 16 bits"""
    return (np.trunc(np.asarray(v, np.float64)).astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)


def wrap_diff(a, b):
    """a - b of two int16 arrays modulo 65536, in [-32768, 32767]"""
    return ((np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64) + 32768) % 65536) - 32768


# ---- families ----------------------------------------------------------------------------------------------------------
def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


FAMILIES = ("white", "full_square", "constant", "sine_fs_on", "sine_fs_off", "impulse", "silence", "loud_then_quiet",
            "tone_plus_faint", "silence_then_white")


def loud_span(s):
    """[lo, hi) of loud_then_quiet's loud sixth.  It starts a quarter into the stream where that leaves quiet output
    both before it and more than a transform length after it (the 1024-point shapes), so that the local bar judges
    quiet blocks that FOLLOW a loud history; on the 8192-point shapes, whose history + 8 blocks hold no such stretch,
    it is the stream's last sixth and the quiet outputs precede it."""
    n = s.n_blocks * s.block
    sixth = n // 6
    lo = n // 4
    if lo >= (s.hist_blocks + 2) * s.block and n - (lo + sixth) >= s.n_fft + 3 * s.block:
        return lo, lo + sixth
    return n - sixth, n


def family(name, s, sigma=2000.0):
    """int16 [n_blocks * block]; seeded by the family's name and the shape alone"""
    n = s.n_blocks * s.block
    rng = np.random.default_rng([1905, FAMILIES.index(name), s.n_fft, s.n_taps, s.n_blocks])
    t = np.arange(n, dtype=np.float64)
    if name == "white":
        x = _i16(rng.normal(0.0, sigma, n))
    elif name == "full_square":
        x = np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    elif name == "constant":
        x = np.full(n, -12345, np.int16)
    elif name == "sine_fs_on":                                    # bin n_fft / 8 + 3 of the transform, exactly
        x = _i16(32000.0 * np.sin(2 * np.pi * (s.n_fft // 8 + 3) * t / s.n_fft))
    elif name == "sine_fs_off":                                   # between two bins
        x = _i16(32000.0 * np.sin(2 * np.pi * (s.n_fft // 8 + 3.47) * t / s.n_fft + 0.3))
    elif name == "impulse":
        x = np.zeros(n, np.int16)
        x[(s.hist_blocks + (s.n_blocks - s.hist_blocks) // 2) * s.block + s.block // 3] = 30000
    elif name == "silence":
        x = np.zeros(n, np.int16)
    elif name == "loud_then_quiet":
        v = rng.normal(0.0, 30.0, n)
        lo, hi = loud_span(s)
        v[lo:hi] = rng.normal(0.0, 9000.0, hi - lo)
        x = _i16(v)
    elif name == "tone_plus_faint":
        x = _i16(20000.0 * np.sin(2 * np.pi * 0.0913 * t + 1.1) + rng.normal(0.0, 20.0, n))
    elif name == "silence_then_white":
        x = _i16(rng.normal(0.0, sigma, n))
        x[:min(n, (s.hist_blocks + 2) * s.block)] = 0
    else:
        raise KeyError(name)
    x.setflags(write=False)
    return x


# ---- filters -----------------------------------------------------------------------------------------------------------
def _hrir(n_filters):
    rng = np.random.default_rng(1906)
    h = np.stack([rng.normal(size=256) * np.exp(-np.arange(256) / (40.0 + 15.0 * f)) for f in range(n_filters)])
    return h / np.sqrt((h * h).sum(axis=1, keepdims=True))


def _highpass():
    """256 taps, windowed-sinc high-pass at a quarter of the sample rate, the taps' mean removed: sum h = 0 to round-off"""
    k = np.arange(256) - 127.5
    h = -np.sinc(0.5 * k) * 0.5 * np.hanning(256)
    h[127] += 0.5
    h[128] += 0.5
    return (h - h.mean())[None]


def _rir():
    g = np.load(os.path.join(GOLDEN, "rir_taps.npz"), allow_pickle=False)
    taps = np.zeros(int(g["n_taps"]))
    taps[g["index"]] = g["value"]
    return taps[None]


def _dense(n_taps, n_filters, seed, tau):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n_filters, n_taps)) * np.exp(-np.arange(n_taps) / tau) * 0.05


@functools.lru_cache(maxsize=None)
def filters():
    """name -> (n_fft, taps float64 [F, n_taps]), read-only"""
    f = {
        "hrir1": (1024, _hrir(1)),                      # pairs kernel, one filter
        "hrir2": (1024, _hrir(2)),                      # pairs kernel, the HRIR pair, unit energy
        "hrir2_x8": (1024, 8.0 * _hrir(2)),             # the wrap: pre-cast values far past int16
        "highpass": (1024, _highpass()),                # sum h ~ 0: constant input gives output ~ 0
        "one_tap": (1024, np.array([[0.75]])),          # block 1024, no history
        "taps1024": (1024, _dense(1024, 1, 1907, 300.0) * 4.0),   # block 1, history 1023 blocks
        "taps200x3": (1024, _dense(200, 3, 1908, 60.0) * 6.0),    # block 825: the generic 1024-point kernel
        "rir": (8192, _rir()),                          # FilterCoefficient.h's room response
        "dense7169": (8192, _dense(7169, 1, 1909, 1500.0)),
        "dense7169_wrap": (8192, _dense(7169, 1, 1909, 1500.0) * 6.0),
        "taps7000": (8192, _dense(7000, 1, 1910, 900.0)),         # block 1193: always the 8192-point kernel
        "taps7681x2": (8192, _dense(7681, 2, 1911, 900.0)),       # block 512, 16 partitions
    }
    for name, (n_fft, h) in f.items():
        assert h.ndim == 2 and h.shape[1] <= n_fft
        assert 32768.0 * np.abs(h).sum(axis=1).max() < 2.0 ** 31, name     # past int32 the cast is not specified
        h.setflags(write=False)
    return f


WRAP_FILTERS = ("hrir2_x8", "dense7169_wrap")
# 8192-point filter -> a stream length at which loud_then_quiet's loud sixth comes FIRST (loud_span's quarter rule) and
# more than a transform length of quiet output follows it
LONG_8192 = {"dense7169": 40, "taps7000": 40, "taps7681x2": 80}


def shape_for(fname, n_blocks=None):
    n_fft, h = filters()[fname]
    return shape_of(n_fft, h.shape[1], n_blocks)


def stream(fname, fam, n_blocks=None, sigma=2000.0):
    return family(fam, shape_for(fname, n_blocks), sigma)


# ---- the FP32 restatement ----------------------------------------------------------------------------------------------
def segments(x, s):
    """[n_out, n_fft] int16: the segment of every output block, the reference's silent head (the first hist_blocks
    blocks of a stream never reach the transform) and the samples before the stream as zeros"""
    n_out = max(s.n_blocks - s.hist_blocks, 0)
    head = s.hist_blocks * s.block
    xz = np.concatenate([np.zeros(s.n_fft, np.int16), x])
    xz[:s.n_fft + head] = 0
    ends = (s.hist_blocks + 1 + np.arange(n_out)) * s.block + s.n_fft
    return np.stack([xz[e - s.n_fft:e] for e in ends]) if n_out else np.zeros((0, s.n_fft), np.int16)


def restate32(x, h, n_fft):
    """Pre-cast output [n_out * block] float32 of one filter, every operation in FP32.  The filter's spectrum is
    computed once in FP64 and rounded to complex64, as the library does when a handle is created."""
    h = np.asarray(h, np.float64).reshape(-1)
    s = shape_of(n_fft, h.size, x.size // (n_fft - h.size + 1))
    H = np.fft.rfft(np.concatenate([h, np.zeros(n_fft - h.size)])).astype(np.complex64)
    seg = segments(x, s).astype(np.float32)
    X = np.fft.rfft(seg, axis=1)
    assert X.dtype == np.complex64, "numpy's float32 transform is needed here (numpy >= 2)"
    y = np.fft.irfft((X * H).astype(np.complex64), n=n_fft, axis=1)
    assert y.dtype == np.float32
    return np.ascontiguousarray(y[:, h.size - 1:]).reshape(-1)


# ---- the bars ----------------------------------------------------------------------------------------------------------
Truth = collections.namedtuple("Truth", "out pre global_bar local_bar shape")


def bars_of(x, h, w, s):
    """(global bar: a number, local bar: one value per output sample) for the oracle pre-cast w of filter h on x"""
    sum_h = float(np.abs(h).sum())
    n_out = w.size // s.block
    if n_out == 0:
        return 0.0, np.zeros(0)
    g = TOL * max(float(np.abs(w).max()), FLOOR * float(np.abs(x.astype(np.int64)).max()) * sum_h)
    wpk = np.abs(w).reshape(n_out, s.block).max(axis=1)
    xa = np.concatenate([np.zeros(s.n_fft, np.int64), np.abs(x.astype(np.int64))])
    loc = np.zeros(n_out)
    for e in range(n_out):
        end = (s.hist_blocks + e + 1) * s.block + s.n_fft
        loc[e] = max(wpk[max(0, e - 1):e + 2].max(), FLOOR * float(xa[end - s.n_fft:end].max()) * sum_h)
    return g, TOL * np.repeat(loc, s.block)


def truth_of(oracle, x, h, n_fft):
    h = np.asarray(h, np.float64).reshape(-1)
    s = shape_of(n_fft, h.size, x.size // (n_fft - h.size + 1))
    out, pre = oracle.fastconv_stream(x, h, n_fft)
    g, loc = bars_of(x, h, pre, s)
    for a in (out, pre, loc):
        a.setflags(write=False)
    return Truth(out, pre, g, loc, s)


_TRUTH = {}


def truth(oracle, fname, fam, f=0, n_blocks=None, sigma=2000.0):
    """truth_of filter row f of `fname` on family `fam`: computed once and shared (read-only)"""
    key = (fname, fam, f, n_blocks, sigma)
    if key not in _TRUTH:
        n_fft, h = filters()[fname]
        _TRUTH[key] = truth_of(oracle, stream(fname, fam, n_blocks, sigma), h[f], n_fft)
    return _TRUTH[key]


def ratios_of(got, t):
    """Worst |got - w| over each bar: (of the global bar, of the local bar); an error under a zero bar is inf."""
    err = np.abs(np.asarray(got, np.float64).reshape(-1) - t.pre)
    assert err.shape == t.pre.shape
    if err.size == 0:
        return 0.0, 0.0
    out = []
    for bar in (np.full(err.size, t.global_bar), t.local_bar):
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / bar)
        out.append(float(q.max()))
    return tuple(out)


def int16_rules(out, pre, t):
    """(samples where out != cast_i16(pre), samples more than one step from cast_i16(w) modulo 65536)"""
    own = int(np.count_nonzero(np.asarray(out).reshape(-1) != cast_i16(np.asarray(pre, np.float32).reshape(-1))))
    far = int(np.count_nonzero(np.abs(wrap_diff(np.asarray(out).reshape(-1), cast_i16(t.pre))) > 1))
    return own, far
