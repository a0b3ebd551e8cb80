"""CPU side of tests/test_mvdrn_hard_gpu.py: what the oracle and two numpy restatements alone can show about the scenes
of tests/mvdrn_cases.py -- that the FP64 restatement is the oracle, that plain FP32 arithmetic keeps every held case
inside the bar with room to spare (so a kernel over the bar has lost something FP32 does not), and that the new scenes
see mistakes and matrices `white` cannot.  Run with -s for the figures (profiles/r23_mvdrn_hard.txt holds them)."""
import numpy as np
import pytest

import mvdrn_cases as H

_oracle_cache = {}


def oracle_case(orc, name, n_mics, loading, n_fft):
    """(o_pre, held) of one case, computed once"""
    key = (name, n_mics, loading, n_fft)
    if key not in _oracle_cache:
        pcm, delays, _ = H.cached_scene(name, n_mics)
        held = H.held_mask(H.flags_of(orc, pcm, n_fft), n_mics, loading, n_fft // 2)
        _oracle_cache[key] = (orc.mvdrn_stream(pcm, delays, loading, n_fft=n_fft)[1], held)
    return _oracle_cache[key]


@pytest.mark.parametrize("name", H.SCENES)
def test_every_scene_has_its_pauses_and_leaves_out_few_blocks(oracle, name):
    """The VAD calls exactly the blocks of QUIET quiet, at both block lengths, on microphone 0 of every scene: a
    loading-0 case then leaves out blocks 1 .. n_mics - 1 (held_mask asserts MAX_LEFT_OUT, the ceiling)."""
    for n_mics in (2, 3, 7, 8):
        pcm, _, _ = H.cached_scene(name, n_mics)
        for n_fft in (1024, 512):
            per = 512 // (n_fft // 2)
            want = np.ones(H.N_BLOCKS * per, np.uint8)
            for b0, nb in H.QUIET:
                want[b0 * per:(b0 + nb) * per] = 0
            flags = H.flags_of(oracle, pcm, n_fft)
            assert np.array_equal(flags, want), (n_mics, n_fft)
            held = H.held_mask(flags, n_mics, 0.0, n_fft // 2)
            assert np.count_nonzero(~held) == (n_mics - 1) * (n_fft // 2)


@pytest.mark.parametrize("name", H.SCENES)
def test_ref64_is_the_oracle(oracle, name):
    """ref64 within 1e-9 of the peak of orc_mvdrn_stream2, the same finite samples and the same VAD decisions."""
    worst = 0.0
    for n_mics in H.N_MICS:
        pcm, delays, _ = H.cached_scene(name, n_mics)
        for n_fft, loadings in ((1024, H.LOADINGS), (512, [1e-6])):
            for loading in loadings:
                o_pre, held = oracle_case(oracle, name, n_mics, loading, n_fft)
                r = H.ref64(pcm, delays, loading, n_fft)
                assert np.array_equal(r["flags"], H.flags_of(oracle, pcm, n_fft))
                s, same = H.share(r["pre"], o_pre, held)
                assert same and np.isfinite(o_pre[held]).all()
                worst = max(worst, s * H.TOL)
    print("ref64 vs oracle %-16s worst %.2e of the peak" % (name, worst))
    assert worst < 1e-9


CASES = [(name, m) for name in H.SCENES for m in H.N_MICS] + [("gain_mismatch", 2), ("gain_mismatch", 7)]


@pytest.mark.parametrize("name,n_mics", CASES)
def test_plain_fp32_stays_inside_the_bar(oracle, name, n_mics):
    """Every case the GPU test holds to the bar: ref32 under 0.5 of it, and for the 512-point cases the paired model
    under 0.7.  (2 and 7 microphones run on the 512-point path only, as on the GPU.)"""
    pcm, delays, _ = H.cached_scene(name, n_mics)
    for loading in H.LOADINGS:
        fig = []
        for n_fft, paired, ceiling in ((1024, False, 0.5), (512, False, 0.5), (512, True, 0.7)):
            if n_fft == 1024 and n_mics not in H.N_MICS:
                continue
            o_pre, held = oracle_case(oracle, name, n_mics, loading, n_fft)
            s, same = H.share(H.ref32(pcm, delays, loading, n_fft, paired)["pre"], o_pre, held)
            fig.append("%d%s %.3f" % (n_fft, " paired" if paired else "", s))
            assert same, (loading, n_fft, paired)
            assert s < ceiling, (loading, n_fft, paired, s)
        print("ref32 share of the bar %-16s mics %d loading %-6g %s" % (name, n_mics, loading, "  ".join(fig)))


MUTANTS = ["load00", "round_delays", "stale_weights"]


def test_each_mutant_is_caught_by_a_new_scene():
    """Three wrong beamformers against the right one, both in FP64, in bars (3 and 8 microphones, loading 1e-3 and 1):
    each is more than 10 bars away on a new scene.  Found on `white`: rounding the delays costs nothing there (they are
    whole samples), the stale weights show, and so does loading with R[0][0] -- 100 to 430 bars, not the "under one"
    that equal-power microphones suggest: tr(R_k) / n is an average over microphones and R_k[0][0] one draw of it, and
    over 8 to 12 frames the two differ by tens of per cent at most bins."""
    cost = {}
    for name in H.SCENES:
        for mu in MUTANTS:
            cost[name, mu] = 0.0
        for n_mics in H.N_MICS:
            pcm, delays, _ = H.cached_scene(name, n_mics)
            for loading in (1e-3, 1.0):
                base = H.ref64(pcm, delays, loading)
                held = np.ones(base["pre"].size, bool)
                for mu in MUTANTS:
                    # (stale weights leave the first emitted block NaN; the figure is over the samples finite in both)
                    s, _ = H.share(H.ref64(pcm, delays, loading, mutant=mu)["pre"], base["pre"], held)
                    cost[name, mu] = max(cost[name, mu], s)
        print("mutants, bars  %-16s %s" % (name, "  ".join("%s %.3g" % (mu, cost[name, mu]) for mu in MUTANTS)))
    for mu in MUTANTS:
        assert max(cost[name, mu] for name in H.NEW_SCENES) > 10, mu
    assert cost["white", "round_delays"] == 0.0
    assert max(cost[name, "round_delays"] for name in ("near", "steering_frac")) > 1000


def covariance_figures(name, n_mics):
    """tr(R_k) max / min over the bins and the diagonal's max / min over the microphones (the worst bin), both after the
    first pause; and the median over the bins of R_k's largest eigenvalue over its smallest, at the end of the stream"""
    pcm = H.cached_scene(name, n_mics)[0]
    R = H.covariance_after_first_pause(pcm)
    tr = np.einsum("kii->k", R).real
    dg = np.einsum("kii->ki", R).real
    ev = np.linalg.eigvalsh(H.ref64(pcm, None, 0.0)["R"])
    return np.array([tr.max() / tr.min(), (dg.max(1) / dg.min(1)).max(), np.median(ev[:, -1] / np.abs(ev[:, 0]))])


def test_new_scenes_have_the_dynamic_range_white_lacks():
    """For every new scene of signals, one figure of its covariance exceeds white's by x100 at 3 or at 8 microphones.
    The first two figures are on the diagonal.  `coherent` and `near` are flat there by construction -- white signals at
    equal gains -- and what they have is off it, R_k close to rank 1: the third figure, the eigenvalue spread, is for
    them.  Two families are left out with a reason each: the steering scenes are white's signals, and what they add is
    the round_delays mutant's business; loud_interferer's pauses are coherent's at a lower contrast, and what it adds is
    in the apply step -- its loud output is a small difference of large products, which the last assertion shows on
    ref64: the output of a late loud block is under a third of microphone 0's where white's is all of it."""
    white = {m: covariance_figures("white", m) for m in H.N_MICS}
    for name in H.SIGNAL_SCENES:
        figs = {m: covariance_figures(name, m) for m in H.N_MICS}
        for m in H.N_MICS:
            print("covariance %-16s mics %d  bins %.3g  microphones %.3g  eigenvalues %.3g" % ((name, m) + tuple(figs[m])))
        if name not in ("white", "loud_interferer"):
            assert max((figs[m] / white[m]).max() for m in H.N_MICS) > 100, name
    level = {}
    for name in ("white", "loud_interferer"):
        pcm, delays, _ = H.cached_scene(name, 8)
        pre = H.ref64(pcm, delays, 1e-3)["pre"]
        b = H.LATE
        level[name] = np.sqrt((pre[(b - 1) * 512:b * 512] ** 2).mean() / (pcm[0, b * 512:(b + 1) * 512].astype(float) ** 2).mean())
    print("output rms over microphone 0's, block %d: white %.3f  loud_interferer %.3f" % (H.LATE, level["white"], level["loud_interferer"]))
    assert level["white"] > 0.9 and level["loud_interferer"] < level["white"] / 3




def test_distortionless_response_of_ref64():
    """The GPU test asks a correlation above 0.99 with the clean source on a late loud block; ref64 has to give twice
    that margin first (1 - r < 0.005).  quiet_mic0 does, at the loadings that leave the estimate its shape (1e-3 and
    1e-6; with loading 1 the matrix is mostly the loading and r falls to 0.98).

    near and loud_interferer do NOT, at any loading, and are therefore not held to it on the GPU; the figures are
    printed.  The reason is the framing, not the arithmetic: a frame is [511 old | 512 new | 0] without a window, the
    emitted samples are its last 512, and y = IDFT(w^H X) is a circular filter.  Weights with a long or two-sided
    response -- a null a quarter sample off the look direction, or any null that needs an advance -- wrap into the
    emitted samples.  On `near` that costs r = 0.96 .. 0.99; on loud_interferer the wrapped share of an interferer
    66 times the source leaves r below 0.2 and the output at 10 .. 27 % of microphone 0's, not under 5 %, whatever
    the levels (tried: 7000 / 100 and 2000 / 50, interferer ahead of or behind the source)."""
    for name in ("near", "loud_interferer", "quiet_mic0"):
        for n_mics in H.N_MICS:
            pcm, delays, src = H.cached_scene(name, n_mics)
            for n_fft in (1024, 512):
                for loading in H.DISTORTIONLESS_LOADINGS:
                    d, level = H.late_block_figures(H.ref64(pcm, delays, loading, n_fft)["pre"], src, pcm, n_fft // 2)
                    print("ref64 late block %-16s mics %d n_fft %4d loading %-6g 1 - r %.2e  rms / microphone 0 %.4f" % (
                        name, n_mics, n_fft, loading, d, level))
                    if name == "quiet_mic0":
                        assert d < 0.005
