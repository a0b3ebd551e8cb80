"""Batched reverberation (jdsp_reverb_batch): the banks, the batches, the two bars and the int16 rules that
test_reverb_fp32_ref_cpu.py (CPU) and test_reverb_batch_gpu.py (device) share (not a test module).

  banks()                   name -> taps [n_irs, n_taps] float64: 1 tap (row 0 the single tap 0.75), 512, 513 (one tap in
                            a second partition), 1025, 7169 (row 0: tests/golden/rir_taps.npz), 7680 dense decaying, a x6
                            "wrap" bank whose pre-cast values pass int16, and a zero-sum high-pass
  batch(name)               the bank's batch, computed once, read-only: utterances of B_u in {0, 1, 2, P - 1, P, P + 1,
                            G - 1, G, G + 1, 2 G + 1} blocks plus one of P + 2 blocks per input family
                            (fastconv_cases.family: white, full_square, constant, sine_fs_off, impulse, silence,
                            loud_then_quiet, silence_then_white), gains 1, 0.25, -3 and 0, several utterances on one
                            response and others on the bank's first and last; with the FP64 values (reverb_ref) and bars
  pack(utts, gaps, fill)    jdsp_denoise_batch_dev's layout with `gaps` samples in front of every span, filled with `fill`
  restate32(x, h, gain)     the partitioned sum in plain FP32: numpy's float32 rfft, complex64, never upcast, the bank
                            spectra rounded from FP64 -- what FP32 alone makes of an utterance
  ratios_of / int16_rules   the worst error as a fraction of each bar; the cast rules

The bars are the convolver's (tests/fastconv_cases.py: TOL = 1e-5, FLOOR = 0.05), per utterance, with w the FP64 value,
x the utterance, g its gain, h its response, P = ceil(n_taps / 512):

  global   |got - w| <= TOL max(max|w|, FLOOR max|x| |g| sum|h|)
  local    for output block e:  TOL max(max|w| over blocks e-1 .. e+1,
                                        FLOOR |g| sum|h| max|x| over the 512 (P + 1) input samples that end with block e)
           samples before the utterance count as zero; where a bar is 0 the output must be exact zeros (either sign)
"""
import collections
import functools

import numpy as np

import fastconv_cases as F
import reverb_ref

TOL, FLOOR = F.TOL, F.FLOOR
B = 512                # samples per block = taps per partition
G = 32                 # output blocks per workgroup of reverb_mac_kernel (csrc/reverb.h kReverbGroup)
GAINS = (1.0, 0.25, -3.0, 0.0)
FAMILIES = ("white", "full_square", "constant", "sine_fs_off", "impulse", "silence", "loud_then_quiet",
            "silence_then_white")
cast_i16, wrap_diff = F.cast_i16, F.wrap_diff


def n_part(n_taps):
    return -(-n_taps // B)


def _rows(n_taps, seed, tau, scale=1.0, n=3):
    return np.stack([F._dense(n_taps, 1, seed + r, tau)[0] * scale for r in range(n)])


@functools.lru_cache(maxsize=None)
def banks():
    rir = _rows(7169, 2010, 1500.0)
    rir[0] = F._rir()[0]
    hp = np.concatenate([F._highpass(), -0.5 * F._highpass(), F._highpass()[:, ::-1]])
    f = {
        "tap1": np.array([[0.75], [-0.5], [1.0]]),
        "taps512": _rows(512, 2001, 150.0, 4.0),
        "taps513": _rows(513, 2004, 150.0, 4.0),              # tap 512 alone in the second partition
        "taps1025": _rows(1025, 2007, 300.0, 2.0),
        "rir7169": rir,
        "dense7680": _rows(7680, 2013, 1500.0),
        "wrap1025": _rows(1025, 2016, 300.0, 6.0),            # x6: full-scale input drives the float far past int16
        "highpass": hp,                                       # sum h = 0: constant input gives output ~ 0
    }
    for name, h in f.items():
        assert h.ndim == 2 and 1 <= h.shape[1] <= 7680
        assert 32768.0 * 3.0 * np.abs(h).sum(axis=1).max() < 2.0 ** 31, name      # past int32 the cast is not specified
        h.setflags(write=False)
    return f


WRAP_BANKS = ("wrap1025",)


def utterance(fam, n_blocks, salt):
    """int16 [512 n_blocks] of the family; `salt` tells two utterances of one family and length apart"""
    if n_blocks == 0:
        return np.zeros(0, np.int16)
    return F.family(fam, F.Shape(1024, 513 + salt, B, 0, n_blocks))


def lengths_of(P):
    return sorted({0, 1, 2, max(P - 1, 0), P, P + 1, G - 1, G, G + 1, 2 * G + 1})


def plan_of(P, n_irs):
    """[(family, n_blocks, ir, gain)]: the lengths first, families and gains dealt round, then one utterance of P + 2
    blocks per family; responses: the bank's first, its last, then the middle one shared by the rest"""
    out = []
    for i, nb in enumerate(lengths_of(P) + [P + 2] * len(FAMILIES)):
        fam = FAMILIES[i % len(FAMILIES)]
        gain = GAINS[(i + i // 4) % len(GAINS)]
        ir = (0, n_irs - 1)[i % 3] if i % 3 < 2 else n_irs // 2
        out.append((fam, nb, ir, gain))
    return out


def bars_of(x, h, gain, w):
    """(global bar: a number, local bar: one value per sample) of the FP64 value w of utterance x"""
    nb = x.size // B
    if nb == 0:
        return 0.0, np.zeros(0)
    P = n_part(np.asarray(h).size)
    scale = abs(float(gain)) * float(np.abs(h).sum())
    xa = np.abs(x.astype(np.int64))
    g = TOL * max(float(np.abs(w).max()), FLOOR * float(xa.max()) * scale)
    wpk = np.abs(w).reshape(nb, B).max(axis=1)
    loc = np.zeros(nb)
    for e in range(nb):
        seg = xa[max(0, (e + 1) * B - B * (P + 1)):(e + 1) * B]
        loc[e] = max(wpk[max(0, e - 1):e + 2].max(), FLOOR * scale * float(seg.max()))
    return g, TOL * np.repeat(loc, B)


Utt = collections.namedtuple("Utt", "x ir gain family w global_bar local_bar")
Batch = collections.namedtuple("Batch", "name taps utts")


@functools.lru_cache(maxsize=None)
def batch(name):
    taps = banks()[name]
    utts = []
    for i, (fam, nb, ir, gain) in enumerate(plan_of(n_part(taps.shape[1]), taps.shape[0])):
        x = utterance(fam, nb, i)
        w = reverb_ref.reverb(x, taps[ir], gain)
        g, loc = bars_of(x, taps[ir], gain, w)
        for a in (w, loc):
            a.setflags(write=False)
        utts.append(Utt(x, ir, gain, fam, w, g, loc))
    return Batch(name, taps, tuple(utts))


def pack(utts, gaps=None, fill=0, tail=0):
    """(pcm int16, sample_first int64 [n], block_first int64 [n + 1]); gaps: even sample counts in front of each span"""
    gaps = [0] * len(utts) if gaps is None else list(gaps)
    assert len(gaps) == len(utts) and all(g % 2 == 0 and g >= 0 for g in gaps)
    first, at = [], 0
    for x, g in zip(utts, gaps):
        at += g
        first.append(at)
        at += x.size
    pcm = np.full(at + tail, fill, np.int16)
    for x, a in zip(utts, first):
        pcm[a:a + x.size] = x
    counts = [x.size // B for x in utts]
    return pcm, np.asarray(first, np.int64), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def gaps_of(n):
    """a gap pattern: none, a pair of samples, a block and a half, ... so that spans start at every alignment"""
    return [(0, 2, 768, 6, 0, 130)[i % 6] for i in range(n)]


# ---- the FP32 restatement ----------------------------------------------------------------------------------------------
def restate32(x, h, gain):
    """float32 [len(x)]: the library's arithmetic in plain FP32.  One float32 transform of [previous block | block] per
    block, the P partition spectra computed in FP64 and rounded to complex64, the sum over p ascending in complex64, the
    inverse in float32, its second half times the float32 gain."""
    h = np.asarray(h, np.float64).reshape(-1)
    nb, P = x.size // B, n_part(h.size)
    if nb == 0:
        return np.zeros(0, np.float32)
    hp = np.zeros((P, 2 * B))
    hp.reshape(-1)[np.arange(h.size) // B * 2 * B + np.arange(h.size) % B] = h
    H = np.fft.rfft(hp, axis=1).astype(np.complex64)
    xz = np.concatenate([np.zeros(B, np.int16), x]).astype(np.float32)
    seg = np.stack([xz[c * B:c * B + 2 * B] for c in range(nb)])
    X = np.fft.rfft(seg, axis=1)
    assert X.dtype == np.complex64, "numpy's float32 transform is needed here (numpy >= 2)"
    Y = np.zeros_like(X)
    for p in range(min(P, nb)):
        Y[p:] = (Y[p:] + (X[:nb - p] * H[p]).astype(np.complex64)).astype(np.complex64)
    y = np.fft.irfft(Y, n=2 * B, axis=1)
    assert y.dtype == np.float32
    return (np.ascontiguousarray(y[:, B:]).reshape(-1) * np.float32(gain)).astype(np.float32)


# ---- judging -----------------------------------------------------------------------------------------------------------
def ratios_of(got, u):
    """Worst |got - w| over each bar of utterance u: (of the global bar, of the local bar); an error under a zero bar
    is inf."""
    err = np.abs(np.asarray(got, np.float64).reshape(-1) - u.w)
    assert err.shape == u.w.shape
    if err.size == 0:
        return 0.0, 0.0
    out = []
    for bar in (np.full(err.size, u.global_bar), u.local_bar):
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / bar)
        out.append(float(q.max()))
    return tuple(out)


def int16_rules(out, pre, u):
    """(samples where out != cast_i16(pre), samples more than one step from cast_i16(w) modulo 65536)"""
    own = int(np.count_nonzero(np.asarray(out).reshape(-1) != cast_i16(np.asarray(pre, np.float32).reshape(-1))))
    far = int(np.count_nonzero(np.abs(wrap_diff(np.asarray(out).reshape(-1), cast_i16(u.w))) > 1))
    return own, far


def must_be_zero(u):
    """the utterance's output is exact zeros by the bars: silence in, or gain 0"""
    return u.x.size > 0 and u.global_bar == 0.0
