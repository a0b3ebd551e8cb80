"""hipGraph capture and replay of the live n-microphone MVDR streams (jdsp_mvdrn_streams_dev / _streams_reset_dev, class D
of include/jdsp.h's "Graph capture"): the scalars and the pointers are baked, the ids, the offsets and the PCM are read
at replay, and every replay advances the named streams from where they stand.  Captured with the helper of
tests/test_graph_replay_gpu.py; the yardstick is a twin handle given the same deliveries by eager calls."""
import numpy as np
import pytest

import graph_replay_cases as G
import mvdrn_batch_cases as K
import mvdrn_streams_cases as S
from graph_replay_cases import dev_fill, dev_of, download, lib, ok, upload, vp
from mvdrn_batch_cases import B

pytestmark = pytest.mark.gpu

N_MICS, N_STREAMS, N_CHUNKS, N_TOTAL = 3, 6, 4, 11
STRIDE = N_TOTAL * B + 8 + N_CHUNKS * 6                       # every plan's spans fit in a plane (a multiple of 8)
# (stream, blocks) per chunk: N_CHUNKS chunks and N_TOTAL blocks every time; other ids, cuts and (below) offsets
PLANS = [[(0, 4), (3, 4), (1, 1), (5, 2)], [(3, 1), (2, 0), (4, 8), (0, 2)], [(1, 3), (2, 3), (3, 3), (5, 2)],
         [(4, 2), (3, 7), (0, 0), (1, 2)]]
GAPS = [(0, 0), (4, 2), (0, 6), (2, 0)]                       # (lead, gap) of plan k


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def sync():
    import torch
    torch.cuda.synchronize()


def streams_pcm():
    return [S.scene(800 + s, N_MICS, 24) for s in range(N_STREAMS)]


class Delivery:
    """the buffers of one jdsp_mvdrn_streams_dev call, captured or eager"""

    def __init__(self, eng, h):
        self.eng, self.h = eng, h
        self.pcm = dev_of(np.zeros((N_MICS, STRIDE), np.int16))
        self.ids = dev_of(np.zeros(N_CHUNKS, np.int64))
        self.first = dev_of(np.zeros(N_CHUNKS, np.int64))
        self.blocks = dev_of(np.zeros(N_CHUNKS + 1, np.int64))
        self.out, self.pre, self.flags = dev_fill(STRIDE * 2), dev_fill(STRIDE * 4), dev_fill(N_TOTAL)

    def load(self, k, xs, at):
        """plan k into the buffers; at[s]: the blocks stream s has been given (advanced here)"""
        lead, gap = GAPS[k]
        pcm = np.full((N_MICS, STRIDE), 32767, np.int16)
        starts, pos = [], lead
        for s, n in PLANS[k]:
            pcm[:, pos:pos + n * B] = xs[s][:, at[s] * B:(at[s] + n) * B]
            at[s] += n
            starts.append(pos)
            pos += n * B + gap
        assert pos <= STRIDE
        upload(self.pcm, pcm)
        upload(self.ids, np.array([s for s, _ in PLANS[k]], np.int64))
        upload(self.first, np.array(starts, np.int64))
        upload(self.blocks, np.concatenate([[0], np.cumsum([n for _, n in PLANS[k]])]).astype(np.int64))
        for t in (self.out, self.pre, self.flags):
            t.fill_(G.FILL)

    def deliver(self):
        ok(self.eng, lib().jdsp_mvdrn_streams_dev(self.h._h, vp(self.pcm), STRIDE, vp(self.ids), vp(self.first),
                                                  vp(self.blocks), N_CHUNKS, N_TOTAL, vp(self.out), vp(self.pre),
                                                  vp(self.flags)), "jdsp_mvdrn_streams_dev")

    def results(self):
        """every byte of the three outputs, the sentinel where nothing was written"""
        return tuple(download(t, np.uint8).tobytes() for t in (self.out, self.pre, self.flags))


def state(h):
    seen, cov = h.streams_state(range(N_STREAMS), want_cov=True)
    return seen.tolist(), cov.tobytes()


def fresh_pair(eng, xs):
    """the captured handle and its eager twin, both warm (one eager delivery with the captured scalars) and fresh again"""
    pair = []
    for _ in range(2):
        h = eng.mvdr_multi(N_MICS, K.delays_of(N_MICS), K.LOADING)
        h.open_streams(N_STREAMS, N_TOTAL)
        dl = Delivery(eng, h)
        eng._use_torch_stream()
        dl.load(0, xs, [0] * N_STREAMS)
        dl.deliver()
        ok(eng, lib().jdsp_mvdrn_streams_reset_dev(h._h, None, 0), "jdsp_mvdrn_streams_reset_dev")
        sync()
        pair.append((h, dl))
    return pair


def test_one_captured_delivery_replayed_for_three_further_deliveries(eng):
    xs = streams_pcm()
    (h, dl), (twin, tdl) = fresh_pair(eng, xs)
    at, tat = [0] * N_STREAMS, [0] * N_STREAMS
    dl.load(0, xs, at)
    g = G.capture(eng, dl.deliver)                              # capturing runs nothing: the streams are still fresh
    assert state(h)[0] == [0] * N_STREAMS
    for k in range(4):
        if k:
            dl.load(k, xs, at)                                  # ids, offsets and PCM rewritten in place
        G.replay(eng, g)
        eng._use_torch_stream()
        tdl.load(k, xs, tat)
        tdl.deliver()
        sync()
        assert dl.results() == tdl.results(), k
        assert state(h) == state(twin), k
    assert state(h)[0] == at and min(at) > 0
    out = download(dl.out, np.int16)
    assert np.any(out != G.sentinel(np.int16)) and np.any(out == G.sentinel(np.int16))
    h.close()
    twin.close()


def test_a_captured_reset_replayed(eng):
    """a delivery and the reset of two listed streams in ONE graph, replayed twice with other ids to reset"""
    xs = streams_pcm()
    (h, dl), (twin, tdl) = fresh_pair(eng, xs)
    r_ids, t_ids = dev_of(np.array([3, 0], np.int64)), dev_of(np.array([3, 0], np.int64))

    def both():
        dl.deliver()
        ok(eng, lib().jdsp_mvdrn_streams_reset_dev(h._h, vp(r_ids), 2), "jdsp_mvdrn_streams_reset_dev")

    at, tat = [0] * N_STREAMS, [0] * N_STREAMS
    dl.load(0, xs, at)
    g = G.capture(eng, both)
    for k, listed in ((0, [3, 0]), (2, [1, 4])):
        if k:
            dl.load(k, xs, at)
        upload(r_ids, np.array(listed, np.int64))
        G.replay(eng, g)
        eng._use_torch_stream()
        tdl.load(k, xs, tat)
        upload(t_ids, np.array(listed, np.int64))
        tdl.deliver()
        ok(eng, lib().jdsp_mvdrn_streams_reset_dev(twin._h, vp(t_ids), 2), "jdsp_mvdrn_streams_reset_dev")
        sync()
        assert dl.results() == tdl.results(), k
        seen, cov = state(h)
        assert (seen, cov) == state(twin), k
        assert all(seen[s] == 0 for s in listed) and any(seen)
        per = 513 * 64 * 16
        assert all(not any(cov[s * per:(s + 1) * per]) for s in listed)
    h.close()
    twin.close()
