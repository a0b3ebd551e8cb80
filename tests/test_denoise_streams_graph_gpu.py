"""hipGraph capture and replay of the live denoise streams (jdsp_denoise_streams_dev / _streams_reset_dev, class D of
include/jdsp.h's "Graph capture"): the scalars and the pointers are baked, the ids, the offsets and the buffers are read
at replay, and every replay advances the named streams from where they stand.  Captured with the helper of
tests/test_graph_replay_gpu.py; the yardstick is the batch entry on each stream's history as one utterance."""
import numpy as np
import pytest

import denoise_fp32_ref as R
import graph_replay_cases as G
from graph_replay_cases import dev_fill, dev_of, download, lib, ok, upload, vp
from test_denoise_gpu import speechlike
from test_denoise_streams_gpu import B, same_bits, yardstick

pytestmark = pytest.mark.gpu

N_STREAMS, N_CHUNKS, N_TOTAL = 5, 3, 9
ROOM = N_TOTAL * B + 4 + N_CHUNKS * 514          # the PCM and output buffers: every plan's spans fit


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def sync():
    import torch
    torch.cuda.synchronize()


def streams_pcm(mode):
    """five streams of 35 blocks and more; in spectral subtraction one is periodic (its frames go through the FP64 pass)"""
    xs = [speechlike(900 + s, 40, pattern=[11 + s, 3, 2, 12, 5]) for s in range(N_STREAMS)]
    if mode == 0:
        xs[3] = R.cases()[1]["pcm"][4 * B:]                  # ten quiet blocks (one latch), then the tones
    return xs


# (stream, blocks) per chunk: N_CHUNKS chunks and N_TOTAL blocks every time; other ids, cuts and (below) offsets
PLANS = [[(0, 4), (3, 4), (1, 1)], [(3, 1), (2, 0), (4, 8)], [(1, 3), (0, 3), (3, 3)], [(4, 2), (3, 7), (0, 0)],
         [(2, 5), (1, 2), (3, 2)], [(3, 3), (0, 5), (2, 1)]]
GAPS = [(0, 0), (4, 2), (0, 514), (2, 0), (4, 514), (0, 2)]              # (lead, gap) of plan k


class Delivery:
    """the buffers of one captured jdsp_denoise_streams_dev call"""

    def __init__(self, eng, h):
        self.eng, self.h = eng, h
        self.pcm = dev_of(np.zeros(ROOM, np.int16))
        self.ids = dev_of(np.zeros(N_CHUNKS, np.int64))
        self.first = dev_of(np.zeros(N_CHUNKS, np.int64))
        self.blocks = dev_of(np.zeros(N_CHUNKS + 1, np.int64))
        self.out, self.pre = dev_fill(ROOM * 2), dev_fill(ROOM * 4)
        self.flags, self.emitted = dev_fill(N_TOTAL), dev_fill(N_CHUNKS * 8)

    def load(self, k, xs, at):
        """plan k into the buffers; at[s]: the blocks stream s has been given (advanced here).  Returns the spans."""
        lead, gap = GAPS[k]
        pcm = np.full(ROOM, 32767, np.int16)
        starts, pos = [], lead
        for s, n in PLANS[k]:
            pcm[pos:pos + n * B] = xs[s][at[s] * B:(at[s] + n) * B]
            at[s] += n
            starts.append(pos)
            pos += n * B + gap
        assert pos <= ROOM
        upload(self.pcm, pcm)
        upload(self.ids, np.array([s for s, _ in PLANS[k]], np.int64))
        upload(self.first, np.array(starts, np.int64))
        upload(self.blocks, np.concatenate([[0], np.cumsum([n for _, n in PLANS[k]])]).astype(np.int64))
        for t in (self.out, self.pre, self.flags, self.emitted):
            t.fill_(G.FILL)
        return starts

    def deliver(self):
        ok(self.eng, lib().jdsp_denoise_streams_dev(self.h._h, vp(self.pcm), vp(self.ids), vp(self.first), vp(self.blocks),
                                                    N_CHUNKS, N_TOTAL, vp(self.out), vp(self.pre), vp(self.flags),
                                                    vp(self.emitted)), "jdsp_denoise_streams_dev")

    def take(self, k, starts, seen, got):
        """what plan k's replay wrote: the emitted blocks to got[s]; everything else is still the sentinel"""
        from jeicyboodsp_amd.sharding import denoise_stream_emitted
        out, pre = download(self.out, np.int16), download(self.pre, np.float32)
        flags, emitted = download(self.flags, np.uint8), download(self.emitted, np.int64)
        want = denoise_stream_emitted([seen[s] for s, _ in PLANS[k]], [n for _, n in PLANS[k]])
        assert np.array_equal(emitted, want), (k, emitted, want)
        covered, b = np.zeros(ROOM, bool), 0
        for (s, n), a, e in zip(PLANS[k], starts, want):
            covered[a:a + e * B] = True
            got[s][0].append(out[a:a + e * B])
            got[s][1].append(pre[a:a + e * B])
            got[s][2].append(flags[b:b + n])
            seen[s] += n
            b += n
        assert np.all(out[~covered] == G.sentinel(np.int16)) and np.all(pre[~covered].view(np.int32) == G.sentinel(np.int32)), k


def check(eng, mode, xs, first, last, got, streams, what):
    """stream s gave what the batch gives for its blocks first[s] .. last[s] as one utterance"""
    for s in streams:
        if last[s] == first[s]:
            assert not any(g.size for part in got[s] for g in part), (what, s)       # chunks of no blocks at the most
            continue
        y_i, y_f, y_flags, _, _ = yardstick(eng, mode, xs[s][first[s] * B:last[s] * B])
        assert np.array_equal(np.concatenate(got[s][0]), y_i), (what, s, "int16")
        assert same_bits(np.concatenate(got[s][1]), y_f), (what, s, "float32")
        assert np.array_equal(np.concatenate(got[s][2]), y_flags), (what, s, "flags")


def fresh_handle(eng, mode):
    h = eng.denoiser(mode)
    h.open_streams(N_STREAMS, N_TOTAL)
    return h


def warm(eng, h, dl, xs):
    """one eager delivery with the captured scalars, then every stream fresh again"""
    eng._use_torch_stream()
    dl.load(0, xs, [0] * N_STREAMS)
    dl.deliver()
    ok(eng, lib().jdsp_denoise_streams_reset_dev(h._h, None, 0), "jdsp_denoise_streams_reset_dev")
    sync()


@pytest.mark.parametrize("mode", [0, 1])
def test_one_captured_delivery_replayed_five_times(eng, mode):
    xs = streams_pcm(mode)
    h = fresh_handle(eng, mode)
    dl = Delivery(eng, h)
    warm(eng, h, dl, xs)
    g = G.capture(eng, dl.deliver)
    at, seen = [0] * N_STREAMS, [0] * N_STREAMS
    got = [([], [], []) for _ in range(N_STREAMS)]
    for k in range(5):
        starts = dl.load(k, xs, at)
        G.replay(eng, g)
        dl.take(k, starts, seen, got)
    assert seen == at and min(at) > 0
    check(eng, mode, xs, [0] * N_STREAMS, at, got, range(N_STREAMS), (mode, "five replays"))
    noise, n_seen = h.streams_state(range(N_STREAMS))
    assert n_seen.tolist() == at
    for s in range(N_STREAMS):
        assert same_bits(noise[s], yardstick(eng, mode, xs[s][:at[s] * B])[3]), s
    h.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_captured_pair_and_reset_replayed_twice(eng, mode):
    """two consecutive deliveries and the reset of one listed stream in ONE graph"""
    xs, r = streams_pcm(mode), 3
    h = fresh_handle(eng, mode)
    a, b = Delivery(eng, h), Delivery(eng, h)
    r_ids = dev_of(np.array([r], np.int64))
    warm(eng, h, a, xs)
    warm(eng, h, b, xs)

    def pair():
        a.deliver()
        b.deliver()
        ok(eng, lib().jdsp_denoise_streams_reset_dev(h._h, vp(r_ids), 1), "jdsp_denoise_streams_reset_dev")

    g = G.capture(eng, pair)
    at, seen, first = [0] * N_STREAMS, [0] * N_STREAMS, [0] * N_STREAMS
    got = [([], [], []) for _ in range(N_STREAMS)]
    for k in (0, 2):
        sa = a.load(k, xs, at)
        sb = b.load(k + 1, xs, at)
        G.replay(eng, g)
        a.take(k, sa, seen, got)
        b.take(k + 1, sb, seen, got)
        assert at[r] > first[r]
        check(eng, mode, xs, first, at, got, (r,), (mode, "the stream that is reset, replay", k))
        got[r], first[r], seen[r] = ([], [], []), at[r], 0                      # the reset: stream r starts again
    check(eng, mode, xs, [0] * N_STREAMS, at, got, [s for s in range(N_STREAMS) if s != r], (mode, "the others continue"))
    noise, n_seen = h.streams_state([r])
    assert n_seen[0] == 0 and not noise.any()
    h.close()
