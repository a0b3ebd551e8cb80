"""Fused STFT masking under a mask that removes something loud and keeps something faint (stftmask_fp32_ref.py holds
the streams; test_stftmask_fp32_ref_cpu.py shows on the CPU what plain FP32 makes of them): notches on tones, a comb
on a square, a band split, ratio masks, a fixed equaliser row, a boost of 1000, an interferer in eight frames only, an
all-zero mask and the white control, at hop 1024 / 512 / 256 with real and complex masks.

Bars, each on every sample of the float32 output and tail: 1e-5 P g (the stream's peak, as test_stftmask_gpu.py) and
the local 1e-5 g max|s| over the hop-blocks within R - 1 of the sample's, which keeps a loud stretch elsewhere from
excusing a suppressed one; int16 = the cast of the device's own float, bit for bit, and within +-1 LSB of the cast of
the restatement.  The bit-identity the header promises (call cuts, frames_per_wave, shards, host = device,
batch = fresh handle) is asserted on these streams too, and frames_recomputed per stream.

Before the FP64 pass (stftmask_frame_f64) the library missed the bars on exactly the 15 streams stftmask_fp32_ref.MISSING
lists from the CPU run, by about what plain FP32 gives there: 60 dB under a notched tone 3.5 (stream bar) / 4.4
(local bar), a combed square 3.8 / 4.6, a band split 1.9 / 2.3, ratio masks 7.1 / 8.6 and 5.0 / 5.0, the fixed
equaliser row 4.2 / 5.1 and 3.7 / 3.7, the boost of 1000 3.6 / 4.0 and 3.9 / 4.7; 80 dB under: 20.2 / 25.8, 43.4 / 47.3,
28.4 / 33.0, 17.1 / 24.2; the interferer in eight frames 0.024 of the stream bar but 4.9 of the local one (hop 512) and
1.8 / 2.0 (hop 1024).  The white control sat at 0.02-0.03, the 40 dB streams at 0.2-0.6.  With the pass every stream
is within 0.033 of both, the white control included (profiles/r13_stftmask_suppress.txt has both tables).
"""
import numpy as np
import pytest

import stftmask_fp32_ref as S
from test_stftmask_gpu import bits, cfg_of

pytestmark = pytest.mark.gpu

CASES = S.cases()
IDS = [c["name"] for c in CASES]
N = S.N
# at least one case per hop and mask kind, every local-interferer one, one with a single mask row
SUBSET = [S.index_of(n) for n in ("notch_on_80dB-1024-real", "notch_off_60dB-1024-complex", "band_split_60dB-512-real",
                                  "local-512-complex", "comb_square_80dB-256-real", "cratio_60dB-256-complex",
                                  "local-256-real", "local-1024-real", "fixed_eq_60dB-256-real")]


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def count(sm):
    """frames_recomputed of the last call; -1 from a library without the entry"""
    return sm.frames_recomputed() if hasattr(sm, "frames_recomputed") else -1


def dev(c):
    import torch
    return torch.from_numpy(np.array(c["pcm"])).cuda(), torch.from_numpy(np.array(c["mask"])).cuda()


def open_case(eng, c):
    return eng.stft_mask(**cfg_of(c["hop"], c["kind"], c["combo"]))


def check(got_f, got_i, bars, what, hold=True):
    """Both bars and the two int16 rules; prints the figures before it asserts."""
    want = bars[0]
    rs, rl = S.ratios_of(got_f, bars)
    print("%s: %.4f of the stream bar, %.4f of the local bar, peak %.1f" % (what, rs, rl, np.abs(want).max()))
    if not hold:
        return rs, rl
    assert rs <= 1.0 and rl <= 1.0, (what, rs, rl)
    assert np.array_equal(got_i, S.cast_i16(got_f.astype(np.float32))), what      # the device's own float, bit for bit
    d = got_i.astype(np.int64) - S.cast_i16(want).astype(np.int64)
    assert np.all(np.abs(d) <= 1), (what, np.abs(d).max())                         # every sample, no exclusions
    return rs, rl


# ---- 1. every case, both bars --------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_case_holds_both_bars(eng, ci):
    import torch
    c = CASES[ci]
    pcm, mask = dev(c)
    sm = open_case(eng, c)
    o, f = sm.process(pcm, mask, c["F"], want_f32=True)
    n = count(sm)
    to, tf = sm.flush(want_f32=True)
    torch.cuda.synchronize()
    sm.close()
    got_f = torch.cat([f, tf]).cpu().numpy()
    got_i = torch.cat([o, to]).cpu().numpy()
    print("%s: %d of %d frames recomputed" % (c["name"], n, c["F"]))
    if c["name"].startswith("zero_mask"):
        assert not got_i.any() and not got_f.any()                                 # exactly zero, -0.0 included
        assert not got_f.view(np.int32).any()
    check(got_f.astype(np.float64), got_i, S.truth(ci), c["name"])


# ---- 2. the count of recomputed frames -----------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_frames_recomputed_count(eng, ci):
    c = CASES[ci]
    pcm, mask = dev(c)
    sm = open_case(eng, c)
    assert count(sm) == 0                                                          # before any call
    sm.process(pcm, mask, c["F"])
    n = count(sm)
    print("%s: %d of %d frames recomputed" % (c["name"], n, c["F"]))
    assert 0 <= n <= c["F"]
    if c["name"] in S.MISSING:
        assert n > 0
    if c["white"]:
        assert n == 0
    k = 5
    sm.process(pcm, mask if mask.ndim == 1 else mask[:k], k, write=False)          # the count is the last call's
    assert 0 <= count(sm) <= k
    sm.reset()
    assert count(sm) == 0
    sm.close()


# ---- 3. bit-identity on these streams ------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", SUBSET, ids=[IDS[i] for i in SUBSET])
def test_cuts_geometries_shards_and_host_bit_identical(eng, ci):
    import torch
    from jeicyboodsp_amd import sharding
    c = CASES[ci]
    hop, F = c["hop"], c["F"]
    R = N // hop
    pcm, mask = dev(c)
    rows = (lambda a, b: mask) if mask.ndim == 1 else (lambda a, b: mask[a:b])
    sm = open_case(eng, c)
    o1, f1 = sm.process(pcm, mask, F, want_f32=True)
    n1 = count(sm)
    t1, tf1 = sm.flush(want_f32=True)

    def same(parts, fparts, t2, tf2, what):
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts), o1), what
        assert torch.equal(bits(torch.cat(fparts)), bits(f1)), what
        assert torch.equal(t2, t1) and torch.equal(bits(tf2), bits(tf1)), what

    def in_calls(cuts, what):
        parts, fparts, j, n = [], [], 0, 0
        for k in cuts:
            o, f = sm.process(pcm[hop * j:], rows(j, j + k), k, want_f32=True)
            n += count(sm)
            parts.append(o.clone())
            fparts.append(f.clone())
            j += k
        assert j == F
        same(parts, fparts, *sm.flush(want_f32=True), what=what)
        assert n == n1, (what, n, n1)                          # a frame is recomputed in the call that emits it, once

    for k in range(1, F):                                      # one cut, at every frame
        in_calls([k, F - k], ("cut at", k))
    in_calls([1] * F, "one frame per call")
    in_calls([7, 1, 1, 6, 1, 1, F - 17], "the interferer's first and last frame +-1")
    for fpw in sorted({max(R - 1, 1), 3, 7, 0}):
        sm.set_option("frames_per_wave", fpw)
        o, f = sm.process(pcm, mask, F, want_f32=True)
        assert count(sm) == n1, fpw
        same([o], [f], *sm.flush(want_f32=True), what=("frames_per_wave", fpw))
    sm.set_option("frames_per_wave", 0)
    for world in (2, 3):                                       # the halo is primed with NULL outputs
        parts, fparts = [], []
        for rank in range(world):
            r = sharding.stftmask_sharded(sm, pcm, mask, F, world, rank, want_f32=True)
            parts.append(r[0].clone())
            fparts.append(r[1].clone())
        same(parts, fparts, *sm.flush(want_f32=True), what=("world", world))
    # the host entry
    oh, fh = sm.process(np.array(c["pcm"]), np.array(c["mask"]), F, want_f32=True)
    assert count(sm) == n1
    th, tfh = sm.flush(want_f32=True)
    assert np.array_equal(oh, o1.cpu().numpy()) and np.array_equal(th, t1.cpu().numpy())
    assert np.array_equal(fh.view(np.int32), f1.cpu().numpy().view(np.int32))
    assert np.array_equal(tfh.view(np.int32), tf1.cpu().numpy().view(np.int32))
    sm.close()


# ---- 4. the batch --------------------------------------------------------------------------------------------------
def batch_of(hop, kind):
    """Utterances (name, pcm, mask rows [F, BINS]) of one hop and kind: suppressed, white, suppressed (one frame),
    none (zero frames), white, suppressed"""
    mine = [c for c in CASES if (c["hop"], c["kind"]) == (hop, kind)]
    white = [c for c in mine if c["white"]][0]
    sup = [c for c in mine if c["level"] is not None]
    assert len(sup) >= 2

    def utt(c, F):
        m = np.array(c["mask"])
        m = np.tile(m[:S.BINS], (F, 1)) if m.ndim == 1 else m[:F, :S.BINS]
        return ("%s[:%d]" % (c["name"], F), np.array(c["pcm"][:hop * (F - 1) + N]), m, F)

    return [utt(sup[0], sup[0]["F"]), utt(white, white["F"]), utt(sup[1], 1),
            ("no frames", np.zeros(200, np.int16), np.zeros((0, S.BINS), mine[0]["mask"].dtype), 0),
            utt(white, 5), utt(sup[-1], sup[-1]["F"])]


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("hop", [1024, 512, 256])
def test_batch_equals_fresh_handles_and_holds_both_bars(eng, hop, kind):
    import torch
    from jeicyboodsp_amd import sharding
    utts = batch_of(hop, kind)
    combo = S.stream_combo(hop)
    offs = np.concatenate([[0], np.cumsum([u[1].size for u in utts])]).astype(np.int64)
    counts, frame_first = sharding.stftmask_batch_layout(offs, N, hop)
    assert counts.tolist() == [u[3] for u in utts]
    pcm = np.concatenate([u[1] for u in utts])
    mask = np.ascontiguousarray(np.concatenate([u[2] for u in utts]))
    sm = eng.stft_mask(**cfg_of(hop, kind, combo))
    bo, bf = sm.process_batch(torch.from_numpy(pcm).cuda(), torch.from_numpy(mask).cuda(), offs, want_f32=True)
    n_batch = count(sm)
    torch.cuda.synchronize()
    ho, hf = sm.process_batch(pcm, mask, offs, want_f32=True)
    assert count(sm) == n_batch
    bo, bf = bo.cpu().numpy(), bf.cpu().numpy()
    assert np.array_equal(ho, bo) and np.array_equal(hf.view(np.int32), bf.view(np.int32))      # host = device
    sm.close()
    n_fresh = 0
    for u, (name, p, m, F) in enumerate(utts):
        a, b = int(offs[u]), int(offs[u + 1])
        if F == 0:
            assert not bo[a:b].any() and not bf[a:b].any()
            continue
        one = eng.stft_mask(**cfg_of(hop, kind, combo))
        o, f = one.process(torch.from_numpy(p).cuda(), torch.from_numpy(m).cuda(), F, want_f32=True)
        n_fresh += count(one)
        to, tf = one.flush(want_f32=True)
        torch.cuda.synchronize()
        one.close()
        fo, ff = torch.cat([o, to]).cpu().numpy(), torch.cat([f, tf]).cpu().numpy()
        assert np.array_equal(bo[a:b], fo), name                                    # a fresh handle, bit for bit
        assert np.array_equal(bf[a:b].view(np.int32), ff.view(np.int32)), name
        check(bf[a:b].astype(np.float64), bo[a:b], S.bars_of(p, m, F, hop, combo), "batch %d %s %s" % (hop, kind, name))
    print("batch %d %s: %d of %d frames recomputed" % (hop, kind, n_batch, int(frame_first[-1])))
    assert n_batch == n_fresh and 0 < n_batch <= int(frame_first[-1])
