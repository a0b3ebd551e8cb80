"""hipGraph capture and replay of jdsp_reverb_batch_dev, class S of include/jdsp.h's "Graph capture": n_utts,
n_blocks_total and the pointers are baked; the PCM, the two offset arrays, ir and gain are read at replay.  One captured
call is replayed after all five arrays were rewritten in place -- other samples, the blocks dealt and the spans moved
differently, other responses and gains -- and twice running; every replay equals an eager call of a fresh handle on
fresh buffers with the same contents, byte for byte, the sentinel outside the spans included.  One capture stream, no
parallel branches.  The capture and replay helpers are tests/graph_replay_cases.py's."""
import numpy as np
import pytest

import reverb_cases as K
from graph_replay_cases import FILL, as_bytes, capture, dev_fill, dev_of, download, lib, ok, replay, upload, vp

pytestmark = pytest.mark.gpu
N_UTTS, TOTAL, BANK = 4, 40, "taps1025"


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def contents():
    """three batches of 40 blocks in 4 utterances in buffers of one length: a batch, the same spans with other PCM,
    responses and gains, and the blocks dealt and the spans moved differently (an empty utterance among them)"""
    out = []
    deals = [((7, 0, 1, 32), (2, 6, 0, 2)), ((7, 0, 1, 32), (2, 6, 0, 2)), ((33, 4, 3, 0), (6, 0, 2, 2))]
    for i, (lens, gaps) in enumerate(deals):
        utts = [K.utterance(("white", "sine_fs_off", "loud_then_quiet", "full_square")[(u + i) % 4], n, 60 + 10 * i + u)
                for u, n in enumerate(lens)]
        pcm, first, bf = K.pack(utts, gaps, fill=32767)
        out.append({"pcm": pcm, "sample_first": first, "block_first": bf,
                    "ir": np.array([(u + i) % 3 for u in range(N_UTTS)], np.int32),
                    "gain": np.array([(1.0, 0.25, -3.0, 0.5)[(u + 2 * i) % 4] for u in range(N_UTTS)], np.float32)})
        assert int(bf[-1]) == TOTAL
    assert len({c["pcm"].size for c in out}) == 1
    return out


def call(h, Bf):
    return lib().jdsp_reverb_batch_dev(h._h, vp(Bf["pcm"]), vp(Bf["sample_first"]), vp(Bf["block_first"]), vp(Bf["ir"]),
                                       vp(Bf["gain"]), N_UTTS, TOTAL, vp(Bf["out_i16"]), vp(Bf["out_f32"]))


def buffers(content, n):
    Bf = {k: dev_of(v) for k, v in content.items()}
    Bf.update({"out_i16": dev_fill(2 * n), "out_f32": dev_fill(4 * n)})
    return Bf


def results(Bf):
    return {"out_i16": download(Bf["out_i16"], np.int16), "out_f32": download(Bf["out_f32"], np.float32)}


def test_one_captured_batch_call_replays_on_rewritten_arrays(eng):
    import torch
    cs = contents()
    n = cs[0]["pcm"].size
    taps = K.banks()[BANK]
    want = []
    for c in cs:                                               # the yardstick: eager, fresh handle, fresh buffers
        h = eng.reverb(taps)
        Bf = buffers(c, n)
        h.reserve_batch(TOTAL, N_UTTS)
        eng._use_torch_stream()
        ok(eng, call(h, Bf), "jdsp_reverb_batch_dev")
        torch.cuda.synchronize()
        want.append(results(Bf))
        # the eager result left the sentinel wherever no span lies, and is not the sentinel inside
        keep = np.ones(n, bool)
        for s, nb in zip(c["sample_first"], np.diff(c["block_first"])):
            keep[int(s):int(s) + int(nb) * K.B] = False
        assert keep.any() and np.all(as_bytes(want[-1]["out_i16"]).reshape(n, 2)[keep] == FILL)
        assert np.all(as_bytes(want[-1]["out_f32"]).reshape(n, 4)[keep] == FILL)
        assert not np.any(np.all(as_bytes(want[-1]["out_f32"]).reshape(n, 4)[~keep] == FILL, axis=1))
        h.close()
    assert want[0]["out_f32"].tobytes() != want[1]["out_f32"].tobytes() != want[2]["out_f32"].tobytes()
    # one capture, on a warm handle
    h = eng.reverb(taps)
    Bf = buffers(cs[0], n)
    h.reserve_batch(TOTAL, N_UTTS)
    eng._use_torch_stream()
    ok(eng, call(h, Bf), "jdsp_reverb_batch_dev (warm)")
    torch.cuda.synchronize()
    g = capture(eng, lambda: ok(eng, call(h, Bf), "jdsp_reverb_batch_dev (captured)"))
    for i in (0, 1, 2, 2):                                     # the last content twice running
        for k, v in cs[i].items():
            upload(Bf[k], v)
        for k in ("out_i16", "out_f32"):
            Bf[k].fill_(FILL)
        replay(eng, g)
        got = results(Bf)
        for k in got:
            assert got[k].tobytes() == want[i][k].tobytes(), \
                ("replay on content", i, k, "%d bytes differ from the eager call" % int((as_bytes(got[k]) != as_bytes(want[i][k])).sum()))
    h.close()
