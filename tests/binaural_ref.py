"""FP64 reference of live binaural rendering (include/jdsp.h, "binaural rendering"), written from the header's
semantics and from nothing else: a direct np.convolve per chunk and ear, the one-block ramp, the sum over the chunks of
a mix.  It knows nothing of transforms or blocks of arithmetic; test_binaural_cpu.py holds it against an independently
written FFT form.  Also here: the inputs the GPU tests share (banks of decaying noise taps, noise and voiced PCM)."""
import numpy as np

BLOCK = 512


def cast_i16(v):
    """(short)double of the reference programs: truncate toward zero, keep the low 16 bits"""
    return (np.trunc(np.asarray(v, np.float64)).astype(np.int64) & 0xffff).astype(np.uint16).view(np.int16)


def bits(g):
    return np.asarray(g, np.float32).view(np.uint32)


class RefBinaural:
    """The streams of one handle and their deliveries, in exact (FP64) arithmetic."""

    def __init__(self, hrirs, n_streams):
        self.h = np.asarray(hrirs, np.float64)
        assert self.h.ndim == 3 and self.h.shape[1] == 2 and 1 <= self.h.shape[2] <= 513
        self.n_streams = n_streams
        self.reset()

    def reset(self, ids=None):
        if ids is None:
            self.hist = np.zeros((self.n_streams, BLOCK), np.int16)
            self.dir = np.zeros(self.n_streams, np.int32)
            self.gain = np.zeros(self.n_streams, np.float32)
            self.started = np.zeros(self.n_streams, np.int32)
            return
        for s in ids:
            self.hist[s], self.dir[s], self.gain[s], self.started[s] = 0, 0, 0.0, 0

    def _heard(self, x, d, g, n):
        """y_{d,g}[t] for the n new samples behind the 512 carried ones, both ears: [2, n]"""
        return np.stack([float(g) * np.convolve(x, self.h[d, e])[BLOCK:BLOCK + n] for e in range(2)])

    def render(self, pcm, stream_ids, sample_first, dirs, gains, chunk_first, block_first):
        """-> (out float64 [2, 512 n_total], bar float64 [n_total]): the mixes, and per output block the sum over the
        mix's chunks of the largest magnitude of the chunk's contribution to either ear over that block"""
        pcm = np.asarray(pcm, np.int16)
        gains = np.asarray(gains, np.float32)
        n_mixes, n_total = len(chunk_first) - 1, int(block_first[-1])
        out = np.zeros((2, BLOCK * n_total))
        bar = np.zeros(n_total)
        ramp = np.arange(BLOCK) / float(BLOCK)
        assert len(set(int(s) for s in stream_ids)) == len(stream_ids), "ids are distinct within a call"
        for m in range(n_mixes):
            b0, nb = int(block_first[m]), int(block_first[m + 1] - block_first[m])
            if nb == 0:
                continue                                    # its chunks' streams are untouched
            for c in range(int(chunk_first[m]), int(chunk_first[m + 1])):
                s, d1, g1, at = int(stream_ids[c]), int(dirs[c]), gains[c], int(sample_first[c])
                new = pcm[at:at + BLOCK * nb]
                assert new.size == BLOCK * nb
                x = np.concatenate([self.hist[s], new]).astype(np.float64)
                y = self._heard(x, d1, g1, BLOCK * nb)
                if self.started[s] and (self.dir[s] != d1 or bits(self.gain[s]) != bits(g1)):
                    old = self._heard(x, int(self.dir[s]), self.gain[s], BLOCK)
                    y[:, :BLOCK] = (1.0 - ramp) * old + ramp * y[:, :BLOCK]
                out[:, BLOCK * b0:BLOCK * (b0 + nb)] += y
                bar[b0:b0 + nb] += np.abs(y).reshape(2, nb, BLOCK).max(axis=(0, 2))
                self.hist[s], self.dir[s], self.gain[s], self.started[s] = new[-BLOCK:], d1, g1, 1
        return out, bar


# ---- inputs ----------------------------------------------------------------------------------------------------------
def make_bank(seed, n_dirs, n_taps, norm=0.25):
    """decaying noise taps, every filter of 2-norm `norm`"""
    rng = np.random.default_rng(seed)
    h = rng.normal(size=(n_dirs, 2, n_taps)) * np.exp(-np.arange(n_taps) / 48.0)
    return h * (norm / np.sqrt((h ** 2).sum(axis=2, keepdims=True)))


def make_pcm(seed, n, voiced=False):
    """sigma ~ 1,500 noise, or a voiced tone: a fundamental near 140 Hz (at 16 kHz) with falling harmonics, 2,400 peak"""
    rng = np.random.default_rng(seed)
    if not voiced:
        return np.clip(np.rint(rng.normal(0, 1500.0, n)), -32768, 32767).astype(np.int16)
    f0 = (130.0 + 25.0 * rng.random()) / 16000.0
    t = np.arange(n)
    v = sum(np.sin(2 * np.pi * f0 * k * t + rng.random() * 6.28) / k for k in range(1, 6))
    return np.rint(2400.0 * v / np.abs(v).max()).astype(np.int16)


def check_block_outputs(o16, o32, want, bar, what=""):
    """guarantee 1 for one delivery: o32 within 1e-5 bar of want per block, o16 the cast of o32 exactly and within +-1
    of the cast of want; the reference stays clear of the int16 wrap"""
    assert np.abs(want).max() < 30000.0, (what, np.abs(want).max())
    n_total = bar.size
    o32 = np.asarray(o32)[:, :BLOCK * n_total]
    o16 = np.asarray(o16)[:, :BLOCK * n_total]
    err = np.abs(o32.astype(np.float64) - want).reshape(2, n_total, BLOCK).max(axis=(0, 2))
    worst = (err / np.maximum(1e-5 * bar, 1e-300)).max() if n_total else 0.0
    assert np.all(err <= 1e-5 * bar), (what, "worst error / bar", worst)
    assert np.array_equal(o16, cast_i16(o32)), what
    lsb = np.abs(o16.astype(np.int32) - cast_i16(want).astype(np.int32)).max() if n_total else 0
    assert lsb <= 1, (what, lsb)
    return worst
