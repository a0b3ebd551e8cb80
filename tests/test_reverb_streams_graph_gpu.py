"""hipGraph capture and replay of the live reverberation streams (jdsp_reverb_streams_dev / _streams_reset_dev, class D of
include/jdsp.h's "Graph capture"): the scalars and the pointers are baked, the ids, the offsets, ir, gain and the PCM are
read at replay, and every replay advances the named streams from where they stand.  Captured with the helper of
tests/test_graph_replay_gpu.py; the yardstick is a twin handle given the same deliveries by eager calls."""
import numpy as np
import pytest

import graph_replay_cases as G
import reverb_cases as K
from graph_replay_cases import dev_fill, dev_of, download, lib, ok, upload, vp

pytestmark = pytest.mark.gpu

B = K.B
BANK = "taps1025"                                             # P = 3: a ring of two rows
N_STREAMS, N_CHUNKS, N_TOTAL = 6, 4, 11
SIZE = N_TOTAL * B + 8 + N_CHUNKS * 6                         # every plan's spans fit
# (stream, blocks, ir, gain) per chunk: N_CHUNKS chunks and N_TOTAL blocks every time; other ids, cuts, responses, gains
PLANS = [[(0, 4, 0, 1.0), (3, 4, 1, 0.25), (1, 1, 2, -3.0), (5, 2, 0, 1.0)],
         [(3, 1, 1, 0.25), (2, 0, 0, 1.0), (4, 8, 2, 1.0), (0, 2, 0, 1.0)],
         [(1, 3, 2, -3.0), (2, 3, 1, 0.0), (3, 3, 0, 1.0), (5, 2, 2, 0.5)],
         [(4, 2, 2, 1.0), (3, 7, 0, 1.0), (0, 0, 1, 1.0), (1, 2, 2, -3.0)]]
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
    return [K.utterance("white", 24, 900 + s) for s in range(N_STREAMS)]


class Delivery:
    """the buffers of one jdsp_reverb_streams_dev call, captured or eager"""

    def __init__(self, eng, h):
        self.eng, self.h = eng, h
        self.pcm = dev_of(np.zeros(SIZE, np.int16))
        self.ids = dev_of(np.zeros(N_CHUNKS, np.int64))
        self.first = dev_of(np.zeros(N_CHUNKS, np.int64))
        self.blocks = dev_of(np.zeros(N_CHUNKS + 1, np.int64))
        self.ir = dev_of(np.zeros(N_CHUNKS, np.int32))
        self.gain = dev_of(np.zeros(N_CHUNKS, np.float32))
        self.o16, self.o32 = dev_fill(SIZE * 2), dev_fill(SIZE * 4)

    def load(self, k, xs, at):
        """plan k into the buffers; at[s]: the blocks stream s has been given (advanced here)"""
        lead, gap = GAPS[k]
        pcm = np.full(SIZE, 32767, np.int16)
        starts, pos = [], lead
        for s, n, _, _ in PLANS[k]:
            pcm[pos:pos + n * B] = xs[s][at[s] * B:(at[s] + n) * B]
            at[s] += n
            starts.append(pos)
            pos += n * B + gap
        assert pos <= SIZE
        upload(self.pcm, pcm)
        upload(self.ids, np.array([p[0] for p in PLANS[k]], np.int64))
        upload(self.first, np.array(starts, np.int64))
        upload(self.blocks, np.concatenate([[0], np.cumsum([p[1] for p in PLANS[k]])]).astype(np.int64))
        upload(self.ir, np.array([p[2] for p in PLANS[k]], np.int32))
        upload(self.gain, np.array([p[3] for p in PLANS[k]], np.float32))
        for t in (self.o16, self.o32):
            t.fill_(G.FILL)

    def deliver(self):
        ok(self.eng, lib().jdsp_reverb_streams_dev(self.h._h, vp(self.pcm), vp(self.ids), vp(self.first), vp(self.blocks),
                                                   vp(self.ir), vp(self.gain), N_CHUNKS, N_TOTAL, vp(self.o16), vp(self.o32)),
           "jdsp_reverb_streams_dev")

    def results(self):
        """every byte of the two outputs, the sentinel where nothing was written"""
        return tuple(download(t, np.uint8).tobytes() for t in (self.o16, self.o32))


def state(h):
    seen, last = h.streams_state(range(N_STREAMS))
    return seen.tolist(), last.tobytes()


def fresh_pair(eng, xs):
    """the captured handle and its eager twin, both warm (one eager delivery with the captured scalars) and fresh again"""
    pair = []
    for _ in range(2):
        h = eng.reverb(K.banks()[BANK])
        h.open_streams(N_STREAMS, N_TOTAL)
        dl = Delivery(eng, h)
        eng._use_torch_stream()
        dl.load(0, xs, [0] * N_STREAMS)
        dl.deliver()
        ok(eng, lib().jdsp_reverb_streams_reset_dev(h._h, None, 0), "jdsp_reverb_streams_reset_dev")
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
            dl.load(k, xs, at)                                  # ids, offsets, ir, gain and PCM rewritten in place
        G.replay(eng, g)
        eng._use_torch_stream()
        tdl.load(k, xs, tat)
        tdl.deliver()
        sync()
        assert dl.results() == tdl.results(), k
        assert state(h) == state(twin), k
    assert state(h)[0] == at and min(at) > 0
    out = download(dl.o16, np.int16)
    assert np.any(out != G.sentinel(np.int16)) and np.any(out == G.sentinel(np.int16))
    # the replays did carry the history: stream 3 was delivered with one response per chunk, and its last chunk (7
    # blocks, response 0, gain 1) is the FP64 value of all its 15 blocks with that response, within the global bar
    import reverb_ref
    w = reverb_ref.reverb(xs[3][:15 * B], K.banks()[BANK][0], 1.0)
    lead, gap = GAPS[3]
    a = lead + 2 * B + gap
    got = download(dl.o32, np.float32)[a:a + 7 * B]
    assert np.abs(got - w[8 * B:]).max() <= K.TOL * np.abs(w).max()
    h.close()
    twin.close()


def test_a_captured_reset_replayed(eng):
    """a delivery and the reset of two listed streams in ONE graph, replayed twice with other ids to reset"""
    xs = streams_pcm()
    (h, dl), (twin, tdl) = fresh_pair(eng, xs)
    r_ids, t_ids = dev_of(np.array([3, 0], np.int64)), dev_of(np.array([3, 0], np.int64))

    def both():
        dl.deliver()
        ok(eng, lib().jdsp_reverb_streams_reset_dev(h._h, vp(r_ids), 2), "jdsp_reverb_streams_reset_dev")

    at, tat = [0] * N_STREAMS, [0] * N_STREAMS
    dl.load(0, xs, at)
    g = G.capture(eng, both)
    for k, listed in ((0, [3, 0]), (2, [1, 5])):
        if k:
            dl.load(k, xs, at)
        upload(r_ids, np.array(listed, np.int64))
        G.replay(eng, g)
        eng._use_torch_stream()
        tdl.load(k, xs, tat)
        upload(t_ids, np.array(listed, np.int64))
        tdl.deliver()
        ok(eng, lib().jdsp_reverb_streams_reset_dev(twin._h, vp(t_ids), 2), "jdsp_reverb_streams_reset_dev")
        sync()
        assert dl.results() == tdl.results(), k
        seen, last = state(h)
        assert (seen, last) == state(twin), k
        assert all(seen[s] == 0 for s in listed) and any(seen)
        assert all(not any(last[s * 2 * B:(s + 1) * 2 * B]) for s in listed)
    h.close()
    twin.close()
