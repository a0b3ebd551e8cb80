"""The FP64 reference of binaural rendering (tests/binaural_ref.py) against an independently written FFT form of
itself, its own cut invariance, and sharding.binaural_layout.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import binaural_ref as R  # noqa: E402


def load_layout():
    """sharding.py without the package (whose import needs the built library)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("jdsp_sharding_only", os.path.join(ROOT, "jeicyboodsp_amd", "sharding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.binaural_layout


class FftForm:
    """The same semantics as overlap-save: per block one 1024-point segment [previous 512 | block], the product of
    its spectrum with the padded taps' spectrum, samples 512..1023 of the inverse; sums taken per block in the
    spectrum, the ramp on a separately accumulated "old" spectrum.  Shares no line with RefBinaural."""

    def __init__(self, hrirs, n_streams):
        self.H = np.fft.fft(np.asarray(hrirs, np.float64), 1024, axis=2)
        self.prev = np.zeros((n_streams, 512))
        self.last = [None] * n_streams

    def render(self, pcm, ids, sample_first, dirs, gains, chunk_first, block_first):
        out = np.zeros((2, 512 * int(block_first[-1])))
        for m in range(len(chunk_first) - 1):
            for b in range(int(block_first[m + 1] - block_first[m])):
                new, old, fade = np.zeros((2, 1024), complex), np.zeros((2, 1024), complex), False
                for c in range(int(chunk_first[m]), int(chunk_first[m + 1])):
                    s, at = int(ids[c]), int(sample_first[c]) + 512 * b
                    blk = np.asarray(pcm[at:at + 512], np.float64)
                    X = np.fft.fft(np.concatenate([self.prev[s], blk]))
                    now = (int(dirs[c]), np.float32(gains[c]).tobytes())
                    was = self.last[s] if (b == 0 and self.last[s] is not None) else now
                    fade |= was != now
                    new += float(np.float32(gains[c])) * X * self.H[now[0]]
                    old += float(np.frombuffer(was[1], np.float32)[0]) * X * self.H[was[0]]
                    self.prev[s], self.last[s] = blk, now
                y = np.fft.ifft(new, axis=1).real[:, 512:]
                if fade:
                    r = np.arange(512) / 512.0
                    y = (1 - r) * np.fft.ifft(old, axis=1).real[:, 512:] + r * y
                j = int(block_first[m]) + b
                out[:, 512 * j:512 * (j + 1)] = y
        return out


def delivery(layout, seed, blocks, chunks, n_dirs, ids):
    rng = np.random.default_rng(seed)
    sf, cf, bf, _, n = layout(blocks, chunks)
    pcm = R.make_pcm(seed, n)
    k = int(cf[-1])
    return pcm, ids[:k], sf, rng.integers(0, n_dirs, k), rng.uniform(0.1, 2.0, k).astype(np.float32), cf, bf


@pytest.mark.parametrize("n_taps", [1, 2, 200, 513])
def test_reference_equals_fft_form(n_taps):
    layout = load_layout()
    bank = R.make_bank(3, 6, n_taps)
    ref, alt = R.RefBinaural(bank, 12), FftForm(bank, 12)
    ids = np.random.default_rng(1).permutation(12)
    for k, (blocks, chunks) in enumerate([([2, 1, 3], [3, 0, 4]), ([1, 2, 1], [3, 0, 4]), ([3, 0, 1], [3, 2, 4])]):
        args = delivery(layout, 10 + k, blocks, chunks, 6, ids)
        want, bar = ref.render(*args)
        got = alt.render(*args)
        assert np.abs(got - want).max() <= 1e-9 * max(bar.max(), 1.0)
        assert bar.shape == (sum(blocks),) and np.all(bar[:blocks[0]] > 0)
        if chunks[1] == 0:
            assert np.all(bar[blocks[0]:blocks[0] + blocks[1]] == 0) and not want[:, 512 * blocks[0]:512 * (blocks[0] + blocks[1])].any()


def test_reference_cut_invariance():
    """six blocks in one delivery = the same six in any split that names the same (dir, gain): the ramp only follows a change"""
    bank = R.make_bank(4, 3, 300)
    pcm = R.make_pcm(5, 512 * 6 * 2)
    sf = np.array([0, 512 * 6])

    def run(cuts):
        ref, outs, at = R.RefBinaural(bank, 2), [], 0
        for n in cuts:
            o, _ = ref.render(pcm, [0, 1], sf + 512 * at, [2, 1], np.float32([0.7, 1.3]), [0, 2], [0, n])
            outs.append(o)
            at += n
        return np.concatenate(outs, axis=1), ref
    whole, ref = run([6])
    for cuts in ([3, 3], [2, 2, 2], [1] * 6, [1, 5]):
        got, r2 = run(cuts)
        assert np.abs(got - whole).max() <= 1e-9 * np.abs(whole).max()
        assert np.array_equal(r2.hist, ref.hist) and np.array_equal(r2.dir, ref.dir)


def test_reference_fades_only_on_change():
    bank = R.make_bank(6, 2, 64)
    pcm = R.make_pcm(7, 1024)
    ref = R.RefBinaural(bank, 1)
    one = lambda at, d, g: ref.render(pcm, [0], [at], [d], np.float32([g]), [0, 1], [0, 1])[0]
    one(0, 0, 1.0)
    got = one(512, 1, 1.0)
    x = pcm.astype(np.float64)
    new = np.stack([np.convolve(x, bank[1, e])[512:1024] for e in range(2)])
    old = np.stack([np.convolve(x, bank[0, e])[512:1024] for e in range(2)])
    r = np.arange(512) / 512.0
    assert np.allclose(got, (1 - r) * old + r * new, rtol=0, atol=1e-9)
    assert got[0, 0] == old[0, 0]                              # r[0] = 0: the block starts where the old source was
    assert R.cast_i16([1.9, -1.9, 32768.0, -32769.0]).tolist() == [1, -1, -32768, 32767]


def test_binaural_layout():
    layout = load_layout()
    sf, cf, bf, mix, n = layout([2, 0, 3], [2, 1, 0])
    assert sf.tolist() == [0, 1024, 2048] and cf.tolist() == [0, 2, 3, 3] and bf.tolist() == [0, 2, 2, 5]
    assert mix.tolist() == [0, 0, 1] and n == 2048
    assert all(a.dtype == np.int64 for a in (sf, cf, bf, mix))
    sf, cf, bf, mix, n = layout([], [])
    assert sf.size == 0 and cf.tolist() == [0] and bf.tolist() == [0] and n == 0
    for bad in (([1, 2], [1]), ([-1], [1]), ([1], [-2])):
        with pytest.raises(ValueError):
            layout(*bad)
