"""The four host entries over a batch of ragged utterances (jdsp_stft_half_batch, jdsp_istft_batch, jdsp_stftmask_batch,
jdsp_denoise_batch) share one layout check (csrc/ragged_layout.h; tests/test_ragged_layout_cpu.py runs it on the host).
Here each entry is called through the C ABI with the five layouts it must reject, and the WHOLE message is pinned --
`<entry>: <reason>` with the entry's own word for its unit array -- where the entries' own error tests only look for
the entry's name.  A good call succeeds before and after the bad ones and gives the same output both times.  The two
host entries over the chunks of live streams (jdsp_istft_streams, jdsp_stftmask_streams) make the same check of their
chunks and are held to the same messages."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N, HOP, PITCH, GAP = 1024, 512, 520, 2


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def vp(a):
    return a.ctypes.data


class Layout:
    """Utterances of `counts` units (frames: hop (f - 1) + n samples; blocks: n = hop) with GAP samples behind each
    span, the last included."""

    def __init__(self, counts, n):
        spans = [HOP * (c - 1) + n for c in counts]
        self.sample_first = np.concatenate([[0], np.cumsum([s + GAP for s in spans])])[:-1].astype(np.int64)
        self.first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.end = int(self.sample_first[-1]) + spans[-1]
        self.n_samples, self.n_utts, self.total = self.end + GAP, len(counts), int(self.first[-1])

    def bad(self, axis):
        """the five rejected layouts as (sample_first, first, n_samples, reason); each breaks one rule only, in an
        utterance behind a sound one, so the reason is the first check that fails"""
        s, f = self.sample_first, self.first

        def poke(a, i, d):
            a = a.copy()
            a[i] += d
            return a

        return [
            (s, f + 1, self.n_samples, axis + "[0] must be 0"),
            (s, poke(f, 2, int(f[1] - f[2]) - 1), self.n_samples, axis + " must not decrease"),
            (poke(s, 1, 1), f, self.n_samples, "sample_first entries must be even and >= 0"),
            (poke(s, 1, -GAP - 2), f, self.n_samples, "sample_first must ascend and the utterances' spans must not overlap"),
            (s, f, self.end - 2, "an utterance's span ends past n_samples"),
        ]


def run_entry(eng, entry, axis, lay, call, outputs):
    """call(sample_first, first, n_samples) -> rc; outputs() -> what a good call wrote"""
    from jeicyboodsp_amd._lib import lib as L
    assert call(lay.sample_first, lay.first, lay.n_samples) == 0, L.jdsp_last_error(eng._h)
    before = [o.copy() for o in outputs()]
    assert any(o.any() for o in before)                                     # the good call computed something
    for s, f, n_samples, reason in lay.bad(axis):
        s, f = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(f, np.int64)
        assert call(s, f, n_samples) == -1, reason
        assert L.jdsp_last_error(eng._h).decode() == "%s: %s" % (entry, reason)
    for o in outputs():
        o[...] = 0
    assert call(lay.sample_first, lay.first, lay.n_samples) == 0, L.jdsp_last_error(eng._h)
    for a, b in zip(before, outputs()):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))           # bit for bit, NaN or not


@pytest.fixture(scope="module")
def frames():
    lay = Layout([2, 3, 1], N)
    rng = np.random.default_rng(1500)
    lay.pcm = np.clip(np.rint(rng.normal(0, 3000.0, lay.n_samples)), -32768, 32767).astype(np.int16)
    return lay


def test_stft_half_batch_messages(eng, frames):
    from jeicyboodsp_amd._lib import lib as L
    spec = np.zeros((frames.total, PITCH), np.complex64)
    run_entry(eng, "jdsp_stft_half_batch", "frame_first", frames,
              lambda s, f, n: L.jdsp_stft_half_batch(eng._h, vp(frames.pcm), n, vp(s), vp(f), frames.n_utts, HOP, vp(spec),
                                                     PITCH),
              lambda: [spec])


def test_istft_batch_messages(eng, frames):
    from jeicyboodsp_amd._lib import lib as L
    spec = eng.stft_half_batch(frames.pcm, np.append(frames.sample_first, frames.n_samples), hop=HOP, pitch=PITCH)
    spec = np.ascontiguousarray(spec)
    h = eng.istft(n_fft=N, hop=HOP, layout="half")
    out, out_f32 = np.zeros(frames.n_samples, np.int16), np.zeros(frames.n_samples, np.float32)
    run_entry(eng, "jdsp_istft_batch", "frame_first", frames,
              lambda s, f, n: L.jdsp_istft_batch(h._h, vp(spec), PITCH, vp(s), vp(f), frames.n_utts, n, vp(out), vp(out_f32)),
              lambda: [out, out_f32])
    h.close()


def test_stftmask_batch_messages(eng, frames):
    from jeicyboodsp_amd._lib import lib as L
    mask = np.full((frames.total, PITCH), 0.5, np.float32)
    h = eng.stft_mask(n_fft=N, hop=HOP)
    out, out_f32 = np.zeros(frames.n_samples, np.int16), np.zeros(frames.n_samples, np.float32)
    run_entry(eng, "jdsp_stftmask_batch", "frame_first", frames,
              lambda s, f, n: L.jdsp_stftmask_batch(h._h, vp(frames.pcm), n, vp(mask), PITCH, vp(s), vp(f), frames.n_utts,
                                                    vp(out), vp(out_f32)),
              lambda: [out, out_f32])
    h.close()


IDS = np.array([2, 0, 1], np.int64)                                        # the live streams of the chunks [2, 3, 1]


def test_istft_streams_messages(eng):
    from jeicyboodsp_amd._lib import lib as L
    lay = Layout([2, 3, 1], HOP)                                           # a chunk's span is its hop F_c output samples
    rng = np.random.default_rng(1502)
    spec = ((rng.normal(size=(lay.total, PITCH)) + 1j * rng.normal(size=(lay.total, PITCH))) * 3000.0).astype(np.complex64)
    h = eng.istft(n_fft=N, hop=HOP, layout="half")
    h.open_streams(3)
    out, out_f32 = np.zeros(lay.n_samples, np.int16), np.zeros(lay.n_samples, np.float32)

    def call(s, f, n):
        assert L.jdsp_istft_streams_reset_dev(h._h, None, 0) == 0          # every call finds the streams fresh
        return L.jdsp_istft_streams(h._h, vp(spec), PITCH, vp(IDS), vp(s), vp(f), lay.n_utts, n, vp(out), vp(out_f32))

    run_entry(eng, "jdsp_istft_streams", "frame_first", lay, call, lambda: [out, out_f32])
    h.close()


def test_stftmask_streams_messages(eng, frames):
    from jeicyboodsp_amd._lib import lib as L
    mask = np.full((frames.total, PITCH), 0.5, np.float32)
    h = eng.stft_mask(n_fft=N, hop=HOP)
    h.open_streams(3)
    out, out_f32 = np.zeros(frames.n_samples, np.int16), np.zeros(frames.n_samples, np.float32)

    def call(s, f, n):
        assert L.jdsp_stftmask_streams_reset_dev(h._h, None, 0) == 0       # every call finds the streams fresh
        return L.jdsp_stftmask_streams(h._h, vp(frames.pcm), n, vp(mask), PITCH, vp(IDS), vp(s), vp(f), frames.n_utts,
                                       vp(out), vp(out_f32))

    run_entry(eng, "jdsp_stftmask_streams", "frame_first", frames, call, lambda: [out, out_f32])
    h.close()


def test_denoise_batch_messages(eng):
    from jeicyboodsp_amd._lib import lib as L
    lay = Layout([6, 14, 3], HOP)
    rng = np.random.default_rng(1501)
    pcm = np.clip(np.rint(rng.normal(0, 3000.0, lay.n_samples)), -32768, 32767).astype(np.int16)
    h = eng.denoiser(0)
    out, flags = np.zeros(lay.n_samples, np.int16), np.zeros(lay.total, np.uint8)
    run_entry(eng, "jdsp_denoise_batch", "block_first", lay,
              lambda s, f, n: L.jdsp_denoise_batch(h._h, vp(pcm), n, vp(s), vp(f), lay.n_utts, vp(out), None, vp(flags), None),
              lambda: [out, flags])
    h.close()
