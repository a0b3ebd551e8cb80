"""GPU parity of spectral subtraction / Wiener on the inputs where transform rounding shows: exactly periodic stretches
(tones on a bin, squares), dithered and coloured ones, DC, impulses, vowels -- after a quiet lead-in that latches the
noise estimate, against the CPU oracle's block-by-block state machine (denoise_fp32_ref.py holds the streams;
test_denoise_fp32_ref_cpu.py shows on the CPU what plain FP32 makes of them).

Bars: test_denoise_gpu.check_stream (1e-5 of the stream's peak before the cast, +-1 LSB after it, finite-mask equal);
VAD flags bit-exact; final noise estimate within 1e-5; and per output block |pre - o_pre| <= 1e-5 x the largest
|o_pre| over the block and its two neighbours, so that a loud stretch elsewhere does not excuse a quiet block.

Before the FP64 pass (denoise_redo_f64_kernel) the mode-0 streams with periodic stretches missed them: up to 71.5 LSB
before the cast at 1024 points (7,604 per-block bars) and 101 at 512 (20,752 bars), dithered and square stretches
included; one 512-point stream with no estimate latched missed the per-block bar in both modes by 1.24 (a quiet frame
sharing its transform with a loud one); everything else passed (profiles/r11_denoise_periodic.txt).
"""
import numpy as np
import pytest

import denoise_fp32_ref as R
from test_denoise_gpu import check_stream, TOL

pytestmark = pytest.mark.gpu

CASES = R.cases()
IDS = [c["name"] for c in CASES]
PATHS = [i for i, c in enumerate(CASES) if c["name"] in ("tone_bin64_1024", "two_tones_1024", "square_1024", "tone_bin100_512",
                                                         "pair_tone20_white_512")]


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def check_blocks(pre, o_pre, block, what, hold=True):
    """The per-block bar; prints the figures before it asserts (hold=False: prints only)."""
    err = np.abs(np.asarray(pre, np.float64) - o_pre)
    per = err.reshape(-1, block).max(axis=1) / R.block_bars(o_pre, block)
    print("%s: %.3g before the cast, %.2e of the stream's peak, %.2f of the per-block bar (block %d)"
          % (what, err.max(), err.max() / np.abs(o_pre).max(), per.max(), 2 + int(per.argmax())))
    assert not hold or per.max() <= 1.0, what


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_stream_matches_oracle(eng, ci, mode):
    c = CASES[ci]
    o_out, o_pre, flags, noises, ver = R.trace(ci, mode)
    d = eng.denoiser(mode, c["n_fft"], c["block"])
    out, pre = d.process(c["pcm"], want_precast=True)
    n_redo = d.frames_recomputed() if hasattr(d, "frames_recomputed") else -1
    print("%s mode %d: %d frames recomputed" % (c["name"], mode, n_redo))
    check_blocks(pre, o_pre, c["block"], "%s mode %d" % (c["name"], mode))
    check_stream(out, pre, o_out, o_pre)
    assert np.array_equal(d.vad_trace(flags.size, flags_only=True).astype(np.int32), flags)
    assert np.abs(d.noise() - noises[-1]).max() <= TOL * max(noises[-1].max(), 1.0)
    d.close()


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_frames_recomputed_count(eng, ci):
    """Readable after a call: > 0 where the stream has exactly periodic stretches, 0 in mode 1 at 1024 points, and no
    more than the stream has frames."""
    c = CASES[ci]
    n_blocks = c["pcm"].size // c["block"]
    d = eng.denoiser(0, c["n_fft"], c["block"])
    assert d.frames_recomputed() == 0                       # before any call
    d.process(c["pcm"])
    n = d.frames_recomputed()
    assert 0 <= n < n_blocks
    if c["periodic"]:
        assert n >= 7
    d.reset()
    assert d.frames_recomputed() == 0
    d.close()
    w = eng.denoiser(1, c["n_fft"], c["block"])
    w.process(c["pcm"])
    if c["n_fft"] == 1024:                                  # Wiener lists frames only where two share a transform
        assert w.frames_recomputed() == 0
    w.close()


@pytest.mark.parametrize("w", R.WHITE_STREAMS, ids=R.white_id)
def test_white_streams_of_the_other_tests(eng, oracle, w):
    """Every speechlike / speechlike256 stream test_denoise_gpu.py names, mode 0: the FP64 pass takes no more frames
    than the CPU restatement finds over HALF the threshold (denoise_fp32_ref.WHITE_STREAMS; 0 on most: nothing is
    recomputed there), so a criterion that drifts on white input fails here instead of moving the white cost; and the
    stream meets the bars of test_denoise_gpu.py (the per-block figure is printed, not asserted: the issue sets that
    bar for the streams of cases())."""
    block, seed, n_blocks, pattern, counts, bound = w
    pcm = R.white_pcm(w)
    o_out, o_pre, *_ = oracle.denoise_trace(0, pcm, block=block)
    d = eng.denoiser(0, 2 * block, block)
    out, pre = d.process(pcm, want_precast=True)
    n = d.frames_recomputed()
    print("%s: %d frames recomputed (CPU: %s over the threshold, %d over half of it)" % (R.white_id(w), n, counts, bound))
    assert n <= bound
    check_stream(out, pre, o_out, o_pre)
    if o_pre.size:
        check_blocks(pre, o_pre, block, R.white_id(w), hold=False)
    d.close()


# ---- call paths: each against the same oracle output -------------------------------------------------------------------------
def _cuts(c):
    """Call boundaries at and around every family boundary, down to one block per call."""
    n_blocks = c["pcm"].size // c["block"]
    edges = sorted({0, n_blocks} | {b + o for _, b0, b1 in c["spans"] for b in (b0, b1) for o in (-1, 0, 1, 2)})
    return [e for e in edges if 0 <= e <= n_blocks]


@pytest.mark.parametrize("ci", PATHS, ids=lambda i: IDS[i])
def test_calls_cut_at_the_family_boundaries(eng, ci):
    c = CASES[ci]
    B = c["block"]
    o_out, o_pre, flags, noises, ver = R.trace(ci, 0)
    for cuts in (_cuts(c), list(range(c["pcm"].size // B + 1))):
        d = eng.denoiser(0, c["n_fft"], B)
        outs, pres, n_redo = [], [], 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            o, p = d.process(c["pcm"][a * B:b * B], want_precast=True)
            n_redo += d.frames_recomputed()
            outs.append(o)
            pres.append(p)
        out, pre = np.concatenate(outs), np.concatenate(pres)
        check_blocks(pre, o_pre, B, "%s in %d calls" % (c["name"], len(cuts) - 1))
        check_stream(out, pre, o_out, o_pre)
        assert n_redo >= 7
        assert np.abs(d.noise() - noises[-1]).max() <= TOL * max(noises[-1].max(), 1.0)
        d.close()


@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("ci", [i for i in PATHS if CASES[i]["n_fft"] == 1024], ids=lambda i: IDS[i])
def test_blocks_per_wave_variants(eng, ci, k):
    c = CASES[ci]
    o_out, o_pre, *_ = R.trace(ci, 0)
    d = eng.denoiser(0)
    d.set_option("blocks_per_wave", k)
    out, pre = d.process(c["pcm"], want_precast=True)
    assert d.frames_recomputed() >= 7
    check_blocks(pre, o_pre, 512, "%s, %d blocks per wave" % (c["name"], k))
    check_stream(out, pre, o_out, o_pre)
    d.close()


def _run_sharded(eng, c, world):
    import torch
    from jeicyboodsp_amd import sharding
    B = c["block"]
    n_total = c["pcm"].size // B
    t = torch.from_numpy(c["pcm"]).cuda()
    ranks = []
    for r in range(world):
        ext0, b0, b1 = sharding.denoise_shard_range(n_total, r, world)
        ranks.append(dict(d=eng.denoiser(0, c["n_fft"], B), ext0=ext0, b0=b0, b1=b1, pcm=t[ext0 * B:b1 * B].clone()))
    fl = [k["d"].shard_vad(k["pcm"], k["ext0"], k["b0"], k["b1"], n_total) for k in ranks]
    flags_all = torch.cat(fl).contiguous()
    summ = torch.stack([k["d"].shard_summary(flags_all) for k in ranks]).contiguous()
    last = torch.stack([k["d"].shard_rows(summ, world, r) for r, k in enumerate(ranks)]).contiguous()
    res = [k["d"].shard_finish(last, world, r, want_precast=True) for r, k in enumerate(ranks)]
    torch.cuda.synchronize()
    n_redo = sum(k["d"].frames_recomputed() for k in ranks)
    for k in ranks:
        k["d"].close()
    return torch.cat([o for o, _ in res]).cpu().numpy(), torch.cat([p for _, p in res]).cpu().numpy(), n_redo


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("ci", PATHS, ids=lambda i: IDS[i])
def test_sharded_finish(eng, ci, world):
    c = CASES[ci]
    o_out, o_pre, *_ = R.trace(ci, 0)
    out, pre, n_redo = _run_sharded(eng, c, world)
    assert n_redo >= 7
    check_blocks(pre, o_pre, c["block"], "%s on %d ranks" % (c["name"], world))
    check_stream(out, pre, o_out, o_pre)


@pytest.mark.parametrize("ci", PATHS, ids=lambda i: IDS[i])
def test_per_block_apply(eng, ci):
    """jdsp_denoise_apply, the reference's per-block signature: one block per call with the estimate the oracle used
    at that block."""
    c = CASES[ci]
    B = c["block"]
    o_out, o_pre, flags, noises, ver = R.trace(ci, 0)
    d = eng.denoiser(0, c["n_fft"], B)
    outs, pres, n_redo = [], [], 0
    for b in range(c["pcm"].size // B):
        o, p = d.apply(c["pcm"][b * B:(b + 1) * B], noises[ver[b]], want_precast=True)
        n_redo += d.frames_recomputed()
        outs.append(o)
        pres.append(p)
    out, pre = np.concatenate(outs), np.concatenate(pres)
    assert n_redo >= 7
    check_blocks(pre, o_pre, B, "%s through apply" % c["name"])
    check_stream(out, pre, o_out, o_pre)
    d.close()
