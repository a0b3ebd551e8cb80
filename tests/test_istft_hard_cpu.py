"""The cases of istft_cases.py on the CPU (no device, no library): what plain FP32 makes of each of them, and the
conditions under which test_istft_hard_gpu.py may hold the device to them.

  - admission: restate32 at or under 0.25 of the stream bar and of the frame bar on every case (the ratio is printed);
  - the amplitude limit |g s| <= 32000 on every case;
  - family 8: on every scaled run restate32 scales exactly and none of its intermediate values is subnormal or
    infinite; the 2^-60 runs that are left out do fail that;
  - the case list is the same, in the same order, on every call;
  - the frame bar against the stream bar.  1e-5 g sum_f P_f |w_s| <= 1e-5 g max_f P_f max sum_f |w_s| always; the
    stream bar holds P, the largest sample AFTER the synthesis window, so frame bar <= stream bar * max sum |w_s| is
    asserted as it stands wherever P = max_f P_f (no window), and with the factor max_f P_f / P under a tapering
    window -- there a frame's largest sample can sit where the window is small and the inequality without the factor
    is false (the white control at n = 1024, hop 512, Hamming: 1.29; printed per case).

Worst restate32 figures per family (stream bar / frame bar): basis 0.044 / 0.029, shapes 0.029 / 0.033, non-Hermitian
0.024 / 0.024, loud beside quiet 0.038 / 0.034, loud stretch 0.027 / 0.021, zero rows 0.018 / 0.021, position 0.020 /
0.022, the clean twins 0.025 / 0.022, the white control 0.029 / 0.023.
"""
import numpy as np
import pytest

import istft_cases as K

CASES = K.cases()
IDS = [c["name"] for c in CASES]


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_admission_and_amplitude(ci):
    c = CASES[ci]
    bars = K.truth(ci)
    rs, rf = K.ratios_of(K.restate32(c["spec"], *K.geo(c)), bars)
    top = np.abs(bars[0]).max()
    print("%s: restate32 at %.4f of the stream bar, %.4f of the frame bar, largest |g s| %.1f" % (c["name"], rs, rf, top))
    assert rs <= K.ADMIT and rf <= K.ADMIT, (c["name"], rs, rf)
    assert top <= K.LIMIT, (c["name"], top)
    assert c["spec"].dtype == np.complex64 and c["spec"].shape[1] >= K.bins_of(c["n"], c["layout"])
    if c["fam"] == 6 and len(c["zero_rows"]) == c["F"]:
        assert not np.asarray(bars[0]).any() and not np.asarray(bars[2]).any()


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_frame_bar_against_stream_bar(ci):
    c = CASES[ci]
    _, stream_bar, frame_bar = K.truth(ci)
    wsum = K.window_sum(c["n"], c["hop"], c["syn"])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(frame_bar == 0, 0.0, frame_bar / (stream_bar * wsum))
    worst = float(q.max())
    pf = K.frame_peaks(c["spec"], c["n"], c["layout"])
    ws = K.window(c["syn"], c["n"])
    y = np.real(np.fft.ifft(K.hermitian(c["spec"], c["n"], c["layout"]), axis=1))
    P = np.abs(y * ws).max()
    k = pf.max() / P if P > 0 else 1.0
    print("%s: frame bar at most %.4f of stream bar * %.3f; max P_f / P = %.4f" % (c["name"], worst, wsum, k))
    assert worst <= k * (1 + 1e-12), (c["name"], worst, k)
    if c["syn"] == "none":
        assert worst <= 1 + 1e-12, (c["name"], worst)


def test_every_configuration_occurs():
    combos = {(n, hop, layout) for n, hop in K.CONFIGS for layout in K.LAYOUTS}
    for fam in sorted({c["fam"] for c in CASES}):
        have = {(c["n"], c["hop"], c["layout"]) for c in CASES if c["fam"] == fam}
        want = {k for k in combos if k[2] == "full"} if fam == 3 else combos
        assert have == want, fam
    for n, hop in K.CONFIGS:
        assert {c["syn"] for c in CASES if (c["n"], c["hop"]) == (n, hop)} == set(K.pairs_of(n, hop)), (n, hop)
    assert {c["fam"] for c in CASES} == {1, 2, 3, 4, 5, 6, 7, 9, 10}
    sub = K.subset()
    assert {CASES[i]["fam"] for i in sub} == {c["fam"] for c in CASES}
    assert {(CASES[i]["n"], CASES[i]["hop"], CASES[i]["layout"]) for i in sub} == combos
    for fam in (4, 10):                                        # family 8 reaches every configuration
        assert {(CASES[i]["n"], CASES[i]["hop"], CASES[i]["layout"]) for i, _ in K.scale_runs() if CASES[i]["fam"] == fam} == combos


def test_case_list_is_the_same_on_every_call():
    again = K.cases.__wrapped__()
    assert [c["name"] for c in again] == IDS
    for a, b in zip(again, CASES):
        assert a["spec"].shape == b["spec"].shape and a["spec"].tobytes() == b["spec"].tobytes(), a["name"]
        assert all(str(a[k]) == str(b[k]) for k in ("poison", "poison_mid", "zero_rows", "positions", "scale")), a["name"]
    assert K.subset() == K.subset() and K.scale_runs() == K.scale_runs()


@pytest.mark.parametrize("ci,k", K.scale_runs(), ids=["%s@%+d" % (IDS[i], k) for i, k in K.scale_runs()])
def test_power_of_two_scale_is_exact_in_fp32(ci, k):
    assert K.scale_admitted(CASES[ci], k)


def test_left_out_scale_runs_do_miss_the_condition():
    left = K.scale_runs(admitted=False)
    assert left and all(k < 0 and CASES[i]["fam"] == 4 for i, k in left)
    for ci, k in left:
        assert not K.scale_admitted(CASES[ci], k), IDS[ci]


def test_special_rows_are_what_they_claim():
    for c in CASES:
        n = c["n"]
        if c["fam"] == 3:                                      # row 11: exactly anti-Hermitian, and not zero
            r = np.asarray(c["spec"][11], np.complex64)
            m = np.conj(r[(-np.arange(n)) % n])
            assert np.array_equal(r.real, -m.real) and np.array_equal(r.imag, -m.imag) and np.abs(r).max() > 1e3
        for f in c["zero_rows"]:
            if c["fam"] != 3:
                assert not c["spec"][f].any()
        if c["fam"] == 7:                                      # the same row, R - 1 zero rows on each side
            R = n // c["hop"]
            assert len(c["positions"]) >= 3
            for p in c["positions"]:
                assert np.array_equal(c["spec"][p], c["spec"][c["positions"][0]]) and c["spec"][p].any()
                for d in range(1, R):
                    assert not c["spec"][p - d].any() and not c["spec"][p + d].any()
        if c["fam"] == 9:
            for which in ("poison", "poison_mid"):
                f, b, part, v = c[which]
                a = K.poisoned(c, which)
                assert b < K.bins_of(n, c["layout"]) and not np.isfinite(a[f, b]) and np.isfinite(np.delete(a, f, axis=0)).all()
                # the weights that zero_weight() calls zero are, and no other: FP64 cosines of exact quarter turns
                w = (np.cos if part == "real" else np.sin)(2 * np.pi * ((b * np.arange(n)) % n) / n)
                assert np.array_equal(np.abs(w) < 1e-9, K.zero_weight(n, b, part))
            f, b, part, v = c["poison"]
            assert part == "real" and b in (0, n // 2) and not K.zero_weight(n, b, part).any()
            assert K.zero_weight(n, *c["poison_mid"][1:3]).any()
