"""hipGraph capture and replay of jdsp_mvdrn_batch_dev, class S of include/jdsp.h's "Graph capture": n_utts,
n_blocks_total, chan_stride and the pointers are baked, the PCM and the two offset arrays are read at replay.  One
captured call is replayed on changed PCM, on changed offsets with the same totals, and twice running; every replay
equals an eager call of a fresh handle on fresh buffers with the same contents, byte for byte, the sentinel outside the
emitted blocks included.  The capture and replay helpers are tests/test_graph_replay_gpu.py's."""
import numpy as np
import pytest

import mvdrn_batch_cases as K
import test_graph_replay_gpu as T
from graph_replay_cases import FILL, as_bytes, capture, dev_fill, dev_of, download, lib, ok, replay, upload, vp

pytestmark = pytest.mark.gpu
N_MICS, N_UTTS, TOTAL = 3, 3, 24


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def contents():
    """three batches of 24 blocks in 3 utterances on planes of one length: a batch, the same spans with other PCM, and
    the blocks dealt and the spans moved differently"""
    out = []
    for i, (lens, gaps) in enumerate([((7, 9, 8), (2, 6, 2)), ((7, 9, 8), (2, 6, 2)), ((9, 7, 8), (6, 2, 2))]):
        utts = [K.utterance(40 + 10 * i + u, N_MICS, n) for u, n in enumerate(lens)]
        pcm, counts, first = K.pack(utts, gaps=gaps)
        out.append({"pcm": pcm, "sample_first": first,
                    "block_first": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)})
    assert len({c["pcm"].shape for c in out}) == 1
    return out


def call(eng, h, Bf, n):
    return lib().jdsp_mvdrn_batch_dev(h._h, vp(Bf["pcm"]), n, vp(Bf["sample_first"]), vp(Bf["block_first"]), N_UTTS, TOTAL,
                                      vp(Bf["out"]), vp(Bf["precast"]), vp(Bf["flags"]))


def buffers(content, n):
    Bf = {k: dev_of(v) for k, v in content.items()}
    Bf.update({"out": dev_fill(2 * n), "precast": dev_fill(4 * n), "flags": dev_fill(TOTAL)})
    return Bf


def results(Bf):
    return {"out": download(Bf["out"], np.int16), "precast": download(Bf["precast"], np.float32),
            "flags": download(Bf["flags"], np.uint8)}


def test_one_captured_batch_call_replays_on_new_pcm_and_new_offsets(eng, oracle):
    cs = contents()
    n = cs[0]["pcm"].shape[1]
    want = []
    for c in cs:                                               # the yardstick: eager, fresh handle, fresh buffers
        h = eng.mvdr_multi(N_MICS, K.delays_of(N_MICS), K.LOADING)
        Bf = buffers(c, n)
        h.reserve_batch(TOTAL, N_UTTS)
        eng._use_torch_stream()
        ok(eng, call(eng, h, Bf, n), "jdsp_mvdrn_batch_dev")
        T.sync()
        want.append(results(Bf))
        # the eager result is the oracle's, and it left the sentinel wherever no block is emitted
        counts = np.diff(c["block_first"])
        utts = [c["pcm"][:, int(s):int(s) + int(nb) * K.B] for s, nb in zip(c["sample_first"], counts)]
        K.check_batch(oracle, utts, c["sample_first"], want[-1]["out"], want[-1]["precast"], want[-1]["flags"])
        keep = np.ones(n, bool)
        for s, nb in zip(c["sample_first"], counts):
            keep[int(s) + K.B:int(s) + int(nb) * K.B] = False
        assert np.all(as_bytes(want[-1]["out"]).reshape(n, 2)[keep] == FILL)
        assert np.all(as_bytes(want[-1]["precast"]).reshape(n, 4)[keep] == FILL)
        T.close(h)
    assert want[0]["out"].tobytes() != want[1]["out"].tobytes() != want[2]["out"].tobytes()
    # one capture, on a warm handle
    h = eng.mvdr_multi(N_MICS, K.delays_of(N_MICS), K.LOADING)
    Bf = buffers(cs[0], n)
    h.reserve_batch(TOTAL, N_UTTS)
    eng._use_torch_stream()
    ok(eng, call(eng, h, Bf, n), "jdsp_mvdrn_batch_dev (warm)")
    T.sync()
    g = capture(eng, lambda: ok(eng, call(eng, h, Bf, n), "jdsp_mvdrn_batch_dev (captured)"))
    for i in (0, 1, 2, 2):                                     # the last content twice running
        for k, v in cs[i].items():
            upload(Bf[k], v)
        for k in ("out", "precast", "flags"):
            Bf[k].fill_(FILL)
        replay(eng, g)
        got = results(Bf)
        for k in got:
            assert got[k].tobytes() == want[i][k].tobytes(), \
                ("replay on content", i, k, "%d bytes differ from the eager call" % int((as_bytes(got[k]) != as_bytes(want[i][k])).sum()))
    T.close(h)
