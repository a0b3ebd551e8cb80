"""What plain FP32 makes of fused STFT masking under a suppressing mask, on the CPU (stftmask_fp32_ref.py): the streams
of test_stftmask_suppress_gpu.py exercise the gap -- the white control and every frame's own content hold both bars,
the 60 / 80 dB streams do not -- and the kernels' criterion separates the two with no white frame flagged."""
import numpy as np
import pytest

import stftmask_fp32_ref as S

CASES = S.cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def fp32():
    """Per case, computed once: (plain-FP32 stream, its ratios to the two bars, per-frame ratio, rho)"""
    out = []
    for ci, c in enumerate(CASES):
        y, _ = S.frames32(c["pcm"], c["mask"], c["F"], c["hop"], c["combo"][0])
        got = S.overlap_add32(y, c["F"], c["hop"], *c["combo"])
        out.append((got, S.ratios(got, ci), S.frame_ratios(y.astype(np.float64), S.frames64(c), ci), S.criterion(c)))
    return out


def test_case_list():
    assert {(c["hop"], c["kind"]) for c in CASES} == {(h, k) for h in (1024, 512, 256) for k in ("real", "complex")}
    assert {(c["hop"], c["kind"]) for c in CASES if c["white"]} == {(c["hop"], c["kind"]) for c in CASES}
    assert any(c["mask_pitch"] == 0 for c in CASES) and set(S.MISSING) <= set(IDS)
    for c in CASES:
        assert 24 <= c["F"] <= 40 and c["combo"] == S.stream_combo(c["hop"])
        assert c["pcm"].size == c["hop"] * (c["F"] - 1) + S.N
    assert max(np.abs(c["mask"]).max() for c in CASES) >= 1000.0          # the boost; the other tests stay under 1.5


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_fp64_restatement_is_finite(ci):
    want, stream_bar, local_bar = S.truth(ci)
    assert np.isfinite(want).all() and np.abs(want).max() < S.LIMIT
    assert np.all(local_bar <= stream_bar * (1 + 1e-12))                 # the local bar never excuses more


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_fp32_holds_each_frames_own_content(ci):
    """Every frame alone under the full (all-pass) mask: FP32 is enough for what a frame holds, whatever it is."""
    c = CASES[ci]
    ones = np.ones(S.BINS, c["mask"].dtype)
    y32, _ = S.frames32(c["pcm"], ones, c["F"], c["hop"], c["combo"][0])
    y64 = S.frames64(dict(c, mask=ones))
    ws = S.window(c["combo"][1])
    # a stream of one frame: P = max |y w_s|, and its local bar is the same (every block is within R - 1 of every other)
    ratio = (np.abs(y32 - y64) * ws).max(axis=1) / (S.TOL * np.maximum(np.abs(y64 * ws).max(axis=1), 1e-300))
    print("%s: worst frame alone at full mask %.4f of the bar" % (c["name"], ratio.max()))
    assert ratio.max() <= 1.0


def test_fp32_misses_exactly_the_listed_cases(fp32):
    missing = []
    for c, (_, (rs, rl), _, rho) in zip(CASES, fp32):
        print("%-30s plain FP32: %8.3f of the stream bar, %8.3f of the local bar, rho %.2e .. %.2e" % (c["name"], rs, rl, rho.min(), rho.max()))
        if max(rs, rl) > 1.0:
            missing.append(c["name"])
        if c["white"]:
            assert max(rs, rl) <= 0.05, c["name"]                          # the white control: far inside both
    assert tuple(missing) == S.MISSING
    # every 80 dB stream with an analysis window, and every 60 dB one but the two stftmask_fp32_ref.py explains
    for c in CASES:
        if c["level"] in (60, 80) and c["name"] not in ("notch_off_60dB-1024-complex", "local-256-real"):
            assert c["name"] in S.MISSING, c["name"]


def test_criterion_separates(fp32):
    """No frame under the threshold (times the margin) misses half its local bar; no white frame is near it; every
    listed case has frames over it (the device must recompute there)."""
    low = [(r, q, c["name"]) for c, (_, _, fr, rho) in zip(CASES, fp32) for r, q in zip(rho, fr) if r <= S.RHO_MARGIN * S.RHO]
    worst = max(low, key=lambda t: t[1])
    print("frames with rho <= %.1e: %d, the worst at %.3f of its local bar (%s, rho %.2e)" % (S.RHO_MARGIN * S.RHO, len(low), worst[1], worst[2], worst[0]))
    assert worst[1] <= 0.5
    assert worst[1] * S.RHO_MARGIN * S.RHO / worst[0] <= 0.5             # ... nor would at the margin, error linear in rho
    first = min(r for c, (_, _, fr, rho) in zip(CASES, fp32) for r, q in zip(rho, fr) if q > 0.5)
    print("smallest rho of a frame over half its local bar: %.2e" % first)
    assert first >= 10 * S.RHO
    for c, (_, _, _, rho) in zip(CASES, fp32):
        if c["white"]:
            assert rho.max() * 6.0 <= S.RHO, c["name"]
        if c["name"] in S.MISSING:
            assert (rho > S.RHO).sum() > 0, c["name"]


def test_zero_mask_gives_zeros(fp32):
    n = 0
    for ci, (c, (got, _, _, rho)) in enumerate(zip(CASES, fp32)):
        if c["name"].startswith("zero_mask"):
            n += 1
            assert not S.truth(ci)[0].any() and not got.any() and not rho.any()
            assert not S.cast_i16(got).any()
    assert n == 2
