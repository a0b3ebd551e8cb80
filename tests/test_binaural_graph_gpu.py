"""hipGraph capture and replay of live binaural rendering (jdsp_binaural_render_dev / _streams_reset_dev, class D of
include/jdsp.h's "Graph capture"): the scalars and the pointers are baked; every array, dir and gain included, is read
at replay, and every replay advances the named streams from where they stand.  Captured with the helpers of
tests/graph_replay_cases.py; the yardstick is the same deliveries as direct calls on a second handle."""
import numpy as np
import pytest

import binaural_ref as R
import graph_replay_cases as G
from graph_replay_cases import dev_fill, dev_of, download, lib, ok, upload, vp

pytestmark = pytest.mark.gpu

BLOCK = 512
N_STREAMS, N_MIXES, N_CHUNKS, N_TOTAL = 8, 3, 5, 6
ROOM = BLOCK * N_TOTAL * N_CHUNKS            # every plan's packed spans fit
PLANE = BLOCK * N_TOTAL + 64

# per delivery: blocks per mix, chunks per mix, stream ids, directions, gains -- N_TOTAL blocks among N_MIXES mixes and
# N_CHUNKS chunks every time, dealt differently; streams come back with another direction or gain, or as they were
PLANS = [
    ([1, 2, 3], [2, 1, 2], [0, 5, 2, 7, 3], [0, 1, 2, 3, 0], [1.0, 0.5, 1.5, 0.8, 1.2]),
    ([3, 0, 3], [1, 2, 2], [5, 1, 4, 7, 0], [2, 1, 1, 3, 0], [0.5, 0.7, 0.9, 1.6, 1.0]),
    ([2, 2, 2], [0, 3, 2], [2, 3, 6, 0, 5], [2, 0, 3, 0, 1], [1.5, 1.2, 0.3, 1.0, 0.5]),
    ([1, 4, 1], [2, 2, 1], [7, 0, 5, 2, 1], [1, 0, 1, 2, 1], [0.8, 2.0, 0.5, 1.5, 0.7]),
]


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def plan_arrays(k, src, at):
    """delivery k as the arrays of the C entry; at[s]: the blocks stream s has been given (advanced here)"""
    from jeicyboodsp_amd.sharding import binaural_layout
    blocks, chunks, ids, dirs, gains = PLANS[k]
    sf, cf, bf, mix, n = binaural_layout(blocks, chunks)
    assert n <= ROOM and bf[-1] == N_TOTAL and cf[-1] == N_CHUNKS
    pcm = np.full(ROOM, 32767, np.int16)
    for c, s in enumerate(ids):
        nb = blocks[mix[c]]
        pcm[sf[c]:sf[c] + BLOCK * nb] = src[s][BLOCK * at[s]:BLOCK * (at[s] + nb)]
        at[s] += nb
    return dict(pcm=pcm, ids=np.array(ids, np.int64), sf=sf, dirs=np.array(dirs, np.int32), gains=np.float32(gains),
                cf=cf, bf=bf)


class Delivery:
    """the buffers of one jdsp_binaural_render_dev call"""

    def __init__(self, eng, h):
        self.eng, self.h = eng, h
        sizes = dict(pcm=ROOM * 2, ids=N_CHUNKS * 8, sf=N_CHUNKS * 8, dirs=N_CHUNKS * 4, gains=N_CHUNKS * 4,
                     cf=(N_MIXES + 1) * 8, bf=(N_MIXES + 1) * 8)
        self.b = {k: dev_of(np.zeros(n, np.uint8)) for k, n in sizes.items()}
        self.o16, self.o32 = dev_fill(2 * PLANE * 2), dev_fill(2 * PLANE * 4)

    def load(self, arrays):
        for k, a in arrays.items():
            upload(self.b[k], a)
        self.o16.fill_(G.FILL)
        self.o32.fill_(G.FILL)

    def deliver(self):
        b = self.b
        ok(self.eng, lib().jdsp_binaural_render_dev(self.h._h, vp(b["pcm"]), vp(b["ids"]), vp(b["sf"]), vp(b["dirs"]),
                                                    vp(b["gains"]), vp(b["cf"]), vp(b["bf"]), N_MIXES, N_CHUNKS, N_TOTAL,
                                                    vp(self.o16), vp(self.o32), PLANE), "jdsp_binaural_render_dev")

    def take(self):
        return download(self.o16, np.int16, (2, PLANE)), download(self.o32, np.float32, (2, PLANE))


def test_captured_delivery_and_reset_replayed(eng):
    import torch
    bank = R.make_bank(81, 4, 300)
    src = [R.make_pcm(90 + s, BLOCK * 16, voiced=(s == 3)) for s in range(N_STREAMS)]
    hg, hd = eng.binaural(bank), eng.binaural(bank)            # replayed / direct
    for h in (hg, hd):
        h.open_streams(N_STREAMS)
    dg, dd = Delivery(eng, hg), Delivery(eng, hd)
    r_ids_g, r_ids_d = dev_of(np.array([0, 0], np.int64)), dev_of(np.array([0, 0], np.int64))
    reset = lambda h, ids: ok(eng, lib().jdsp_binaural_streams_reset_dev(h._h, vp(ids), 2), "jdsp_binaural_streams_reset_dev")
    ref = R.RefBinaural(bank, N_STREAMS)

    # delivery 0 is the one captured: it runs when it is replayed the first time
    at_g, at_d = [0] * N_STREAMS, [0] * N_STREAMS
    eng._use_torch_stream()
    dg.load(plan_arrays(0, src, [0] * N_STREAMS))
    dg.deliver()                                                # warm: one eager call with the captured scalars ...
    ok(eng, lib().jdsp_binaural_streams_reset_dev(hg._h, None, 0), "jdsp_binaural_streams_reset_dev")   # ... undone
    torch.cuda.synchronize()
    g_render = G.capture(eng, dg.deliver)
    g_reset = G.capture(eng, lambda: reset(hg, r_ids_g))
    eng._use_torch_stream()

    for k in range(4):
        if k == 2:
            # a captured reset between two deliveries: streams 5 and 2, named in the buffer at replay
            for ids in (r_ids_g, r_ids_d):
                upload(ids, np.array([5, 2], np.int64))
            G.replay(eng, g_reset)
            eng._use_torch_stream()
            reset(hd, r_ids_d)
            ref.reset([5, 2])
        a = plan_arrays(k, src, at_g)
        dg.load(a)
        G.replay(eng, g_render)
        got = dg.take()
        eng._use_torch_stream()
        dd.load(plan_arrays(k, src, at_d))
        dd.deliver()
        torch.cuda.synchronize()
        want = dd.take()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32)), k
        # what no block wrote is still the sentinel, and what was written is the delivery
        assert np.all(got[0][:, BLOCK * N_TOTAL:] == G.sentinel(np.int16)), k
        assert np.all(got[1][:, BLOCK * N_TOTAL:].view(np.int32) == G.sentinel(np.int32)), k
        w, bar = ref.render(a["pcm"], a["ids"], a["sf"], a["dirs"], a["gains"], a["cf"], a["bf"])
        R.check_block_outputs(got[0], got[1], w, bar, what=("replay", k))
    every = np.arange(N_STREAMS)
    for x, y in zip(hg.streams_state(every), hd.streams_state(every)):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    assert np.array_equal(hg.streams_state(every)[0], ref.hist) and at_g == at_d
    hg.close()
    hd.close()
