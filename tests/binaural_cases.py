"""Live binaural rendering on the streams white noise does not reach (not a test module): input families, banks, the
floored bar, the plain-FP32 restatement and the int16 rules that test_binaural_fp32_ref_cpu.py (CPU) and
test_binaural_streams_gpu.py (device) share.  The vocabulary is fastconv_cases.py's.

  family(name, n_blocks)    seeded int16 streams of n_blocks blocks of 512: fastconv_cases.family's recipes at n_fft = 1024
                            (loud_then_quiet with the loud stretch in block 2, so that quiet blocks follow it), and
                            dc_plus_faint, nyquist, full_white
  banks()                   name -> [n_dirs, 2, n_taps] float64
  RefFloored                binaural_ref.RefBinaural whose render3() also returns the floored bar
  Restate32                 the same deliveries in plain FP32: numpy's rfft on float32 segments, complex64 spectra, never
                            upcast; the gain on the spectrum before the bank product, the sum in list order, the ramp in
                            float32 on a second, "old", accumulation
  ratios, check_outputs     the worst error per bar, and the rules one delivery's outputs are held to

The two bars of one output block, with P_c the largest magnitude of chunk c's contribution to either ear over the block:

  unfloored   |got - want| <= 1e-5 sum_c P_c                     (binaural_ref.RefBinaural.render's bar)
  floored     |got - want| <= 1e-5 F,   F = sum_c max(P_c, 0.05 S_c),
              S_c = max|x over the chunk's 1024-sample segment| max(|g1| max_e sum|h[d1][e]|, |g0| max_e sum|h[d0][e]|),
              the (d0, g0) term only while the chunk fades, samples before a fresh stream zero;
              where F = 0, got must be exactly zero (of either sign)

S_c bounds every sample of the segment's circular convolution: 0.05 S_c is the scale FP32 round-off of the segment
lives on when the kept samples themselves are (nearly) zero (fastconv_cases.py's floor, per chunk).
"""
import functools

import numpy as np

import binaural_ref as R
import fastconv_cases as K
from fastconv_cases import FLOOR, TOL, cast_i16, wrap_diff  # noqa: F401  (the project's figures and cast, not new ones)

BLOCK = 512
N_FFT = 1024
N_BLOCKS = 10

FAMILIES = K.FAMILIES + ("dc_plus_faint", "nyquist", "full_white")
LOUD_BLOCK = 2


# ---- families ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family(name, n_blocks=N_BLOCKS):
    """int16 [512 n_blocks], read-only; seeded by the family's name and the length alone"""
    n = BLOCK * n_blocks
    rng = np.random.default_rng([1912, FAMILIES.index(name), n_blocks])
    if name == "loud_then_quiet":
        v = rng.normal(0.0, 30.0, n)
        v[BLOCK * LOUD_BLOCK:BLOCK * (LOUD_BLOCK + 1)] = rng.normal(0.0, 9000.0, BLOCK)
        x = K._i16(v)
    elif name == "dc_plus_faint":
        x = K._i16(20000.0 + rng.normal(0.0, 20.0, n))
    elif name == "nyquist":
        x = np.where(np.arange(n) % 2 == 0, 32000, -32000).astype(np.int16)
    elif name == "full_white":
        x = K._i16(rng.normal(0.0, 9000.0, n))
    else:
        return K.family(name, K.Shape(N_FFT, N_FFT - BLOCK + 1, BLOCK, 1, n_blocks))
    x.setflags(write=False)
    return x


# ---- banks -------------------------------------------------------------------------------------------------------------
def _lowpass_contra():
    """ear 0 a decaying-noise filter of 200 taps; ear 1 the same through a 33-tap low-pass (a fifth of the sample rate,
    unit gain at DC), 40 dB down overall"""
    k = np.arange(33) - 16.0
    lp = 0.4 * np.sinc(0.4 * k) * np.hanning(35)[1:-1]
    lp /= lp.sum()
    near = R.make_bank(1916, 2, 200)[:, 0]
    h = np.zeros((2, 2, 232))
    for d in range(2):
        h[d, 0, :200] = near[d]
        h[d, 1] = 0.01 * np.convolve(near[d], lp)
    return h


def _one_ear():
    """directions 0 and 1 are deaf on ear 1; direction 2 hears with both"""
    h = R.make_bank(1917, 3, 200).copy()
    h[:2, 1] = 0.0
    return h


@functools.lru_cache(maxsize=None)
def banks():
    """name -> [n_dirs, 2, n_taps] float64, read-only"""
    hp = K._highpass()[0]
    b = {
        "noise1": R.make_bank(1913, 3, 1),
        "noise2": R.make_bank(1913, 3, 2),
        "noise200": R.make_bank(1913, 3, 200),
        "noise513": R.make_bank(1913, 3, 513),
        "highpass": np.stack([np.stack([hp, 0.5 * hp]), np.stack([0.5 * hp, hp])]),   # sum h = 0: DC gives ~ 0
        "lowpass_contra": _lowpass_contra(),
        "one_ear": _one_ear(),
        "delta": np.array([[[0.75], [0.75]], [[0.5], [-0.75]]]),
        "loud": 8.0 * R.make_bank(1913, 3, 200),                   # the wrap: pre-cast values far past int16
    }
    for h in b.values():
        assert h.ndim == 3 and h.shape[1] == 2 and h.shape[2] <= 513
        h.setflags(write=False)
    return b


FAMILY_BANKS = ("noise1", "noise2", "noise200", "noise513", "highpass", "lowpass_contra", "one_ear", "delta")
# the pairs on which plain FP32 was found to break the header's unfloored bar: a quiet block behind a loud one under a
# one-tap filter, DC into a filter that removes it, the silence behind a click
BREAK_UNFLOORED = [("loud_then_quiet", "noise1"), ("constant", "highpass")] + [("impulse", b) for b in FAMILY_BANKS]
MAX_SUM = 2.0 ** 31 / 32768.0                                      # past int32 the cast is not specified


# ---- the reference with the floored bar -----------------------------------------------------------------------------
class RefFloored(R.RefBinaural):
    """RefBinaural, and per output block F = sum_c max(P_c, 0.05 S_c).  render() is the parent's."""

    def render3(self, pcm, stream_ids, sample_first, dirs, gains, chunk_first, block_first):
        """-> (out float64 [2, 512 n_total], bar [n_total], floored bar F [n_total]); out and bar are render()'s"""
        pcm = np.asarray(pcm, np.int16)
        gains = np.asarray(gains, np.float32)
        sum_h = np.abs(self.h).sum(axis=2).max(axis=1)             # per direction: max over the ears of sum|h|
        n_total = int(block_first[-1])
        floor = np.zeros(n_total)
        for m in range(len(chunk_first) - 1):
            b0, nb = int(block_first[m]), int(block_first[m + 1] - block_first[m])
            total = 0.0
            for c in range(int(chunk_first[m]), int(chunk_first[m + 1])):
                s, d1, g1, at = int(stream_ids[c]), int(dirs[c]), gains[c], int(sample_first[c])
                scale = np.full(nb, abs(float(g1)) * sum_h[d1])
                if nb and self.started[s] and (self.dir[s] != d1 or R.bits(self.gain[s]) != R.bits(g1)):
                    scale[0] = max(scale[0], abs(float(self.gain[s])) * sum_h[self.dir[s]])
                total += scale.max() if nb else 0.0
                x = np.abs(np.concatenate([self.hist[s], pcm[at:at + BLOCK * nb]]).astype(np.int64))
                seg = np.array([x[BLOCK * b:BLOCK * b + N_FFT].max() for b in range(nb)], np.float64)
                # the bar of this chunk as a mix of its own is its P_c per block; the stream's state is put back
                keep = (self.hist[s].copy(), self.dir[s], self.gain[s], self.started[s])
                _, p = self.render(pcm, [s], [at], [d1], [g1], [0, 1], [0, nb])
                self.hist[s], self.dir[s], self.gain[s], self.started[s] = keep
                floor[b0:b0 + nb] += np.maximum(p, FLOOR * seg * scale)
            assert total < MAX_SUM, ("32768 sum_c |g_c| sum|h| must stay under 2^31", m, total)
        out, bar = self.render(pcm, stream_ids, sample_first, dirs, gains, chunk_first, block_first)
        assert np.all(floor >= bar * (1 - 1e-12))
        return out, bar, floor


# ---- the FP32 restatement ----------------------------------------------------------------------------------------------
class Restate32:
    """What FP32 alone makes of the deliveries: every operation in float32 / complex64.  The bank's spectra are computed
    once in FP64 and rounded to complex64, as the library does when a handle is created."""

    def __init__(self, hrirs, n_streams):
        self.h = np.asarray(hrirs, np.float64)
        self.spectra = {}
        self.hist = np.zeros((n_streams, BLOCK), np.int16)
        self.dir = np.zeros(n_streams, np.int32)
        self.gain = np.zeros(n_streams, np.float32)
        self.started = np.zeros(n_streams, np.int32)

    def H(self, d):
        """complex64 [2, 513] of direction d, computed when first heard from"""
        if d not in self.spectra:
            self.spectra[d] = np.fft.rfft(self.h[d], N_FFT, axis=1).astype(np.complex64)
        return self.spectra[d]

    def render(self, pcm, stream_ids, sample_first, dirs, gains, chunk_first, block_first):
        """-> float32 [2, 512 n_total]"""
        pcm = np.asarray(pcm, np.int16)
        gains = np.asarray(gains, np.float32)
        out = np.zeros((2, BLOCK * int(block_first[-1])), np.float32)
        ramp = (np.arange(BLOCK, dtype=np.float32) / np.float32(BLOCK)).astype(np.float32)
        for m in range(len(chunk_first) - 1):
            b0, nb = int(block_first[m]), int(block_first[m + 1] - block_first[m])
            if nb == 0:
                continue
            new = np.zeros((2, nb, N_FFT // 2 + 1), np.complex64)
            old = np.zeros((2, N_FFT // 2 + 1), np.complex64)
            faded = False
            for c in range(int(chunk_first[m]), int(chunk_first[m + 1])):
                s, d1, g1, at = int(stream_ids[c]), int(dirs[c]), gains[c], int(sample_first[c])
                x = np.concatenate([self.hist[s], pcm[at:at + BLOCK * nb]]).astype(np.float32)
                X = np.fft.rfft(np.stack([x[BLOCK * b:BLOCK * b + N_FFT] for b in range(nb)]), axis=1)
                assert X.dtype == np.complex64, "numpy's float32 transform is needed here (numpy >= 2)"
                d0, g0 = d1, g1
                if self.started[s] and (self.dir[s] != d1 or R.bits(self.gain[s]) != R.bits(g1)):
                    d0, g0, faded = int(self.dir[s]), self.gain[s], True
                gX = (np.float32(g1) * X).astype(np.complex64)
                oX = (np.float32(g0) * X[0]).astype(np.complex64)
                for e in range(2):
                    new[e] += gX * self.H(d1)[e]
                    old[e] += oX * self.H(d0)[e]
                self.hist[s], self.dir[s], self.gain[s], self.started[s] = pcm[at:at + BLOCK * nb][-BLOCK:], d1, g1, 1
            y = np.fft.irfft(new, n=N_FFT, axis=2)[:, :, BLOCK:]
            assert y.dtype == np.float32
            if faded:
                o = np.fft.irfft(old, n=N_FFT, axis=1)[:, BLOCK:]
                y[:, 0] = ramp * y[:, 0] + (np.float32(1.0) - ramp) * o
            out[:, BLOCK * b0:BLOCK * (b0 + nb)] = y.reshape(2, BLOCK * nb)
        return out


# ---- the rules -----------------------------------------------------------------------------------------------------
def block_errors(got, want):
    got = np.asarray(got, np.float64)
    n = want.shape[1] // BLOCK
    return np.abs(got[:, :BLOCK * n] - want).reshape(2, n, BLOCK).max(axis=(0, 2))


def ratios(got, want, bar):
    """per block the worst |got - want| / (1e-5 bar): 0 where the error is 0, inf where only the bar is"""
    err = block_errors(got, want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / (TOL * bar))


def worst(q):
    return float(q.max()) if q.size else 0.0


def int16_rules(o16, o32, want):
    """(samples where o16 is not the cast of o32, samples more than one step from the cast of want modulo 65536)"""
    n = want.shape[1]
    o16, o32 = np.asarray(o16)[:, :n], np.asarray(o32, np.float32)[:, :n]
    return int(np.count_nonzero(o16 != cast_i16(o32))), int(np.count_nonzero(np.abs(wrap_diff(o16, cast_i16(want))) > 1))


def check_outputs(o16, o32, want, bar, floor, what="", unfloored=False):
    """One delivery against the floored bar (and the header's unfloored one where asked), the exact-zero rule and the
    int16 rules across the wrap.  -> (worst error / floored bar, worst error / unfloored bar)"""
    qf, qu = ratios(o32, want, floor), ratios(o32, want, bar)
    n = want.shape[1]
    got = np.asarray(o32)[:, :n].reshape(2, -1, BLOCK)
    assert not got[:, floor == 0].any(), (what, "a block whose bar is zero is not exact zeros")
    assert np.all(qf <= 1.0), (what, "worst error / floored bar", worst(qf), "block", int(qf.argmax()))
    if unfloored:
        assert np.all(qu <= 1.0), (what, "worst error / unfloored bar", worst(qu), "block", int(qu.argmax()))
    own, far = int16_rules(o16, o32, want)
    assert own == 0, (what, "int16 samples that are not the cast of the float", own)
    assert far == 0, (what, "int16 samples more than one step from the cast of the FP64 value", far)
    return worst(qf), worst(qu)


# ---- the family scenes: every family one single-source mix, one bank ----------------------------------------------
def family_delivery(bname, first, nb):
    """blocks first .. first + nb of every family, one mix each at gain 1, family i heard from direction i mod n_dirs"""
    n_dirs = banks()[bname].shape[0]
    k = len(FAMILIES)
    pcm = np.concatenate([family(f)[BLOCK * first:BLOCK * (first + nb)] for f in FAMILIES])
    ids = np.arange(k)[::-1].copy()                               # family i is stream k - 1 - i
    return pcm, (ids, BLOCK * nb * np.arange(k), np.arange(k) % n_dirs, np.ones(k, np.float32), np.arange(k + 1),
                 nb * np.arange(k + 1))


@functools.lru_cache(maxsize=None)
def family_truth(bname):
    """(want [2, 512 * 10 * 13], bar, floor) of family_delivery(bname, 0, 10): computed once, read-only"""
    pcm, args = family_delivery(bname, 0, N_BLOCKS)
    t = RefFloored(banks()[bname], len(FAMILIES)).render3(pcm, *args)
    for a in t:
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def family_fp32(bname):
    """family -> (plain FP32's worst error / floored bar, / unfloored bar) through bank bname"""
    pcm, args = family_delivery(bname, 0, N_BLOCKS)
    want, bar, floor = family_truth(bname)
    y = Restate32(banks()[bname], len(FAMILIES)).render(pcm, *args)
    qf, qu = ratios(y, want, floor).reshape(-1, N_BLOCKS), ratios(y, want, bar).reshape(-1, N_BLOCKS)
    return {f: (worst(qf[i]), worst(qu[i])) for i, f in enumerate(FAMILIES)}


def holds_unfloored(bname, fam):
    """plain FP32 held the header's unfloored bar with a factor of 2 to spare: the device is held to it too"""
    return family_fp32(bname)[fam][1] <= 0.5


# ---- the scenes: multi-source mixes, fades and many-chunk mixes, as lists of deliveries -----------------------------
class Scene:
    """bank [n_dirs, 2, n_taps], n_streams, and deliveries: a list of (pcm int16, the six arrays of one render call)"""

    def __init__(self, bank, n_streams):
        self.bank = banks()[bank] if isinstance(bank, str) else bank
        self.n_streams = n_streams
        self.deliveries = []

    def add(self, spans, ids, span_of, dirs, gains, chunks, blocks):
        """spans: the PCM spans, laid back to back; chunk c reads spans[span_of[c]] (spans may be shared); mix m has
        chunks[m] chunks and blocks[m] blocks"""
        first = np.concatenate([[0], np.cumsum([s.size for s in spans])])
        mix = np.repeat(np.arange(len(chunks)), chunks)
        for c, i in enumerate(span_of):
            assert spans[i].size == BLOCK * blocks[mix[c]]
        z = np.zeros(1, np.int64)
        self.deliveries.append((np.concatenate(spans).astype(np.int16),
                                (np.asarray(ids, np.int64), first[np.asarray(span_of)].astype(np.int64),
                                 np.asarray(dirs, np.int32), np.asarray(gains, np.float32),
                                 np.concatenate([z, np.cumsum(chunks)]).astype(np.int64),
                                 np.concatenate([z, np.cumsum(blocks)]).astype(np.int64))))
        return self


def _cut(x, first, nb):
    return x[BLOCK * first:BLOCK * (first + nb)]


def _noise(seed, n_blocks, sigma):
    return K._i16(np.random.default_rng([1914, seed]).normal(0.0, sigma, BLOCK * n_blocks))


def scene_wrap17():
    """17 full-scale sources at gains up to +-2 through `loud`: pre-cast peaks far past +-32,768"""
    s = Scene("loud", 17)
    src = [_noise(100 + k, 3, 9000.0) if k % 2 == 0 else np.roll(family("full_square"), 5 * k)[:BLOCK * 3] for k in range(17)]
    gains = np.float32([(-1) ** k * (0.25 + 1.75 * k / 16.0) for k in range(17)])
    return s.add(src, np.arange(17), np.arange(17), np.arange(17) % 3, gains, [17], [3])


def scene_wrap_gain8():
    s = Scene("noise200", 1)
    return s.add([_cut(family("full_square"), 0, 3)], [0], [0], [1], [8.0], [1], [3])


def scene_loud_plus_quiet():
    """a loud source and one 60 dB quieter"""
    s = Scene("noise200", 2)
    return s.add([_cut(family("full_white"), 0, 3), _cut(family("white"), 0, 3)], [0, 1], [0, 1], [0, 2], [1.0, 1e-3], [2], [3])


def scene_cancel():
    """two chunks on one PCM span and direction at gains g and -g: the exact sum is 0, the bar 2 P"""
    s = Scene("noise200", 2)
    x = family("full_white")
    s.add([_cut(x, 0, 2)], [1, 0], [0, 0], [2, 2], [1.5, -1.5], [2], [2])
    return s.add([_cut(x, 2, 2)], [1, 0], [0, 0], [2, 2], [1.5, -1.5], [2], [2])


def scene_two_dirs():
    """one span heard from two directions in one mix"""
    s = Scene("noise513", 2)
    return s.add([_cut(family("tone_plus_faint"), 0, 3)], [0, 1], [0, 0], [0, 2], [1.0, 0.7], [2], [3])


def scene_gains():
    """gains -1.0, 1e-3 and 1e3 in one mix (denormal-range gains are out of scope)"""
    s = Scene("noise200", 3)
    src = [_cut(family("white"), 0, 3), _cut(family("full_white"), 3, 3), _cut(family("white"), 6, 3)]
    return s.add(src, [2, 0, 1], [0, 1, 2], [0, 1, 2], [-1.0, 1e-3, 1e3], [3], [3])


def scene_fade_gain():
    """gain 1000 -> 0.001 -> 1000"""
    s = Scene("noise200", 1)
    x = family("white")
    for k, g in enumerate((1000.0, 0.001, 1000.0)):
        s.add([_cut(x, 2 * k, 2)], [0], [0], [1], [g], [1], [2])
    return s


def scene_signed_zero():
    """gain 1 -> +0.0f (a fade to silence) -> -0.0f (a change by the bit-pattern rule: a faded block of zeros) -> -0.0f"""
    s = Scene("noise200", 1)
    x = family("full_white")
    for k, g in enumerate((1.0, 0.0, -0.0, -0.0)):
        s.add([_cut(x, k, 1)], [0], [0], [1], [g], [1], [1])
    return s


def scene_one_ear():
    """mix 0: two sources that stay on the directions deaf on ear 1 while they swap directions and change gain: ear 1
    is exact zeros, plain and faded.  mix 1: one source that moves from a one-eared direction to a two-eared one and back"""
    s = Scene("one_ear", 3)
    a, b, c = family("white"), family("tone_plus_faint"), family("full_white")
    plan = [([0, 1, 0], [1.0, 0.5, 1.0]), ([1, 0, 2], [1.0, 0.5, 1.0]), ([1, 0, 0], [0.3, 0.5, 1.0]), ([1, 0, 0], [0.3, 0.5, 1.0])]
    for k, (dirs, gains) in enumerate(plan):
        s.add([_cut(a, 2 * k, 2), _cut(b, 2 * k, 2), _cut(c, 2 * k, 2)], [0, 1, 2], [0, 1, 2], dirs, gains, [2, 1], [2, 2])
    return s


def scene_seam_fade(bank):
    """a direction change on the block whose segment is [loud block | quiet block] of loud_then_quiet"""
    s = Scene(bank, 1)
    x = family("loud_then_quiet")
    s.add([_cut(x, 0, LOUD_BLOCK + 1)], [0], [0], [0], [1.0], [1], [LOUD_BLOCK + 1])
    return s.add([_cut(x, LOUD_BLOCK + 1, 3)], [0], [0], [2], [1.0], [1], [3])


MANY = [(64, 0), (64, 63), (65, 0), (65, 63), (65, 64), (130, 0), (130, 63), (130, 64), (130, 129)]


def scene_many(n, moved, never_changed=False):
    """one mix of n small sources, 2 blocks a delivery: all started; chunk `moved` alone changes direction; none
    changes.  never_changed: the same PCM with the moved chunk on its final direction from the start"""
    s = Scene("noise200", n + 3)
    rng = np.random.default_rng([1915, n])
    ids = rng.permutation(n + 3)[:n]
    dirs = rng.integers(0, 3, n)
    gains = rng.uniform(0.05, 0.3, n).astype(np.float32) * rng.choice([-1.0, 1.0], n).astype(np.float32)
    src = [_noise(1000 + c, 6, 1500.0) for c in range(n)]
    after = dirs.copy()
    after[moved] = (dirs[moved] + 1) % 3
    for k in range(3):
        d = after if (k >= 1 or never_changed) else dirs
        s.add([_cut(x, 2 * k, 2) for x in src], ids, np.arange(n), d, gains, [n], [2])
    return s


def _dir_taps(d, e):
    """three taps per ear, distinct for every direction: derived from its index"""
    u = (d * 7919 % 16384) / 16384.0
    return np.array([0.5 + 0.25 * u, -0.25 + 0.5 * (d / 16384.0), 0.125 * (1 - 2 * e) + 0.1 * u]) * (1.0 - 0.3 * e)


@functools.lru_cache(maxsize=None)
def big_bank():
    """n_dirs = 16384, the largest the header documents; 3 taps per ear"""
    d = np.arange(16384, dtype=np.float64)
    h = np.ascontiguousarray(np.stack([_dir_taps(d, e) for e in range(2)]).transpose(2, 0, 1))   # [n_dirs, 2, 3]
    assert np.unique(h.reshape(16384, -1), axis=0).shape[0] == 16384
    h.setflags(write=False)
    return h


BIG_DIRS = (0, 1, 8191, 16382, 16383)


def scene_directions():
    """sources from the first, the middle and the last directions of the largest bank, each its own mix, and all in one"""
    s = Scene(big_bank(), 10)
    x = [_cut(family("white"), k, 2) for k in range(5)]
    return s.add(x, np.arange(10), list(range(5)) * 2, BIG_DIRS * 2, [1.0] * 10, [1] * 5 + [5], [2] * 6)


def scenes():
    """name -> Scene builder: the mixes both test files run"""
    sc = {"wrap17": scene_wrap17, "wrap_gain8": scene_wrap_gain8, "loud_plus_quiet": scene_loud_plus_quiet,
          "cancel": scene_cancel, "two_dirs": scene_two_dirs, "gains": scene_gains, "fade_gain": scene_fade_gain,
          "signed_zero": scene_signed_zero, "one_ear": scene_one_ear,
          "seam_fade_noise1": functools.partial(scene_seam_fade, "noise1"),
          "seam_fade_noise200": functools.partial(scene_seam_fade, "noise200"), "directions": scene_directions}
    for n, moved in MANY:
        sc["many%d_moved%d" % (n, moved)] = functools.partial(scene_many, n, moved)
    return sc


@functools.lru_cache(maxsize=None)
def scene(name):
    return scenes()[name]()


@functools.lru_cache(maxsize=None)
def scene_truth(name):
    """per delivery (want, bar, floor, the reference's (hist, dir, gain, started) behind it): computed once, read-only"""
    s = scene(name)
    ref, out = RefFloored(s.bank, s.n_streams), []
    for pcm, args in s.deliveries:
        t = ref.render3(pcm, *args) + ((ref.hist.copy(), ref.dir.copy(), ref.gain.copy(), ref.started.copy()),)
        for a in t[:3]:
            a.setflags(write=False)
        out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def scene_fp32(name):
    """per delivery (plain FP32's worst error / floored bar, / unfloored bar, its output)"""
    s = scene(name)
    r32, out = Restate32(s.bank, s.n_streams), []
    for (pcm, args), (want, bar, floor, _) in zip(s.deliveries, scene_truth(name)):
        y = r32.render(pcm, *args)
        out.append((worst(ratios(y, want, floor)), worst(ratios(y, want, bar)), y))
    return out
