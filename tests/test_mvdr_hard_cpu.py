"""CPU side of tests/test_mvdr_hard_gpu.py: what the oracle and two numpy restatements alone can show about the scenes,
delays and matrices of tests/mvdr_cases.py -- that the FP64 restatement is the oracle, that plain FP32 arithmetic keeps
every case under a tenth of the bar (so a kernel held to a small multiple of it has lost nothing FP32 keeps), and that
the new scenes and delays see mistakes `white` at whole-sample delays cannot.  Run with -s for the figures
(profiles/r24_mvdr_hard.txt holds them)."""
import numpy as np
import pytest

import mvdr_cases as H

_oracle_cache = {}


def oracle_case(orc, name, d_time):
    """(o_out, o_pre, corr, trace) of one case, computed once"""
    key = (name, d_time)
    if key not in _oracle_cache:
        _oracle_cache[key] = orc.mvdr_stream(*H.cached_scene(name), d_time)
    return _oracle_cache[key]


def oracle_flags(orc, L):
    return np.array([orc.mvdr_vad_block(L[b * 512:(b + 1) * 512])[0] for b in range(L.size // 512)], np.uint8)


@pytest.mark.parametrize("name", H.SCENES)
def test_every_scene_has_its_pauses_and_its_finite_blocks(oracle, name):
    """The oracle's VAD calls the 14 blocks of QUIET quiet (all 30 where the left channel never speaks), the restatement
    decides alike, all 29 emitted blocks are finite -- none on dead_right_in_pauses, whose matrix is singular -- and
    full_scale under a delay leaves int16 before the cast."""
    L, R = H.cached_scene(name)
    flags = oracle_flags(oracle, L)
    want = np.zeros(H.N_BLOCKS, np.uint8) if name in H.NEVER_LOUD else (H._loud(H.N_BLOCKS)[::512] > 0).astype(np.uint8)
    assert np.array_equal(flags, want)
    assert np.count_nonzero(flags == 0) == (30 if name in H.NEVER_LOUD else 14)
    r = H.ref64(L, R, 0.0)
    assert np.array_equal(r["flags"], flags)
    assert r["events"] == (29 if name in H.NEVER_LOUD else 12)
    for d_time in H.DELAYS:
        o_out, o_pre, corr, trace = oracle_case(oracle, name, d_time)
        assert o_pre.size == 29 * 512
        if name == "dead_right_in_pauses":
            assert corr[3] == 0.0 and not np.isfinite(o_pre).any() and not o_out.any()
        else:
            assert np.isfinite(o_pre).all()
        if name == "full_scale":
            # the overwritten real part (:180-183) has gain above 1 once the weights are complex; the whole-sample delays
            # reach 37,661 to 39,361 here, the two fractional ones 28,070 and 28,223, no delay 32,768 at the most
            print("full_scale d_time %-10g oracle pre-cast peak %.0f" % (d_time, np.abs(o_pre).max()))
            if d_time in (2.5e-4, -2.5e-3, 1e-2):
                assert np.abs(o_pre).max() > 32767
            if d_time == 0.0:
                assert np.abs(o_pre).max() < 32768.5


@pytest.mark.parametrize("name", H.SCENES)
def test_ref64_is_the_oracle_and_plain_fp32_is_far_inside_the_bar(oracle, name):
    """ref64 within 1e-6 of the bar of orc_mvdr_stream, its matrix the oracle's (diagonal to 1e-12, the oracle's
    off-diagonal nothing but rounding); ref32 under 0.1 of the bar; the finite masks equal."""
    L, R = H.cached_scene(name)
    for d_time in H.DELAYS:
        _, o_pre, corr, trace = oracle_case(oracle, name, d_time)
        r = H.ref64(L, R, d_time)
        scale = max(corr[0], corr[3])
        assert np.abs(r["trace"][:, [0, 3]] - trace[:, [0, 3]]).max() <= 1e-12 * scale
        assert np.abs(trace[:, 1:3]).max() <= 1e-12 * scale
        s64, same64 = H.share(r["pre"], o_pre)
        s32, same32 = H.share(H.ref32(L, R, d_time)["pre"], o_pre)
        print("share of the bar %-20s d_time %-10g ref64 %.2e  ref32 %.4f" % (name, d_time, s64, s32))
        assert same64 and same32
        assert s64 < 1e-6
        assert s32 < 0.1


def test_each_mutant_is_caught_by_a_new_case_and_missed_by_todays():
    """Four wrong beamformers against the right one, both in FP64, in bars.  Each is more than 10 bars away on a new
    (scene, delay).  What today's cases cannot see: the mirror bins' steering taken as the conjugate costs under one bar
    on `white` without a delay and at 2.5e-4 (a whole number of samples: the angle at bin 1024 - m is 2 PI fs dTime minus
    the angle at m, a multiple of 2 pi up to 3.141592 against pi), and the overwritten real part is no quirk at all
    without a delay (the weights are real).  Stale weights on an estimation block cost under 2 bars where the pause's level ratio
    stands still (dc, hum) and over 50 where the matrix versions move (lowpassed)."""
    cost = {}
    for name in H.SCENES:
        L, R = H.cached_scene(name)
        for d_time in H.DELAYS:
            base = H.ref64(L, R, d_time)["pre"]
            for mu in H.MUTANTS:
                # (stale weights leave the first emitted block NaN; the figure is over the samples finite in both)
                cost[name, d_time, mu] = H.share(H.ref64(L, R, d_time, mutant=mu)["pre"], base)[0]
            print("mutants, bars  %-20s d_time %-10g %s" % (name, d_time, "  ".join(
                "%s %.3g" % (mu, cost[name, d_time, mu]) for mu in H.MUTANTS)))
    todays = [("white", 0.0), ("white", 2.5e-4)]
    for mu in H.MUTANTS:
        assert max(cost[n, d, mu] for n in H.SCENES for d in H.DELAYS if (n, d) not in todays) > 10, mu
    for n, d in todays:
        assert cost[n, d, "mirror_conj"] < 1
    assert max(cost["white", d, "mirror_conj"] for d in (1e-4, 1.37 * 6.25e-5)) > 1000
    for n in H.SCENES:
        assert cost[n, 0.0, "no_quirk"] == 0.0
    # The stale figure is one draw's: it is mostly block 2's, the weights of one estimation frame against those of two.
    # Over the seeds 1 .. 5 lowpassed gives 28 to 79 bars (30 to 48 at seed 1, the GPU tests' draw), dc and hum under 2 at
    # every seed and delay.
    stale = {}
    for n in ("dc", "hum", "lowpassed"):
        for seed in range(1, 6):
            L, R = H.scene(n, seed)
            for d in H.DELAYS:
                stale[n, seed, d] = H.share(H.ref64(L, R, d, mutant="stale")["pre"], H.ref64(L, R, d)["pre"])[0]
            print("stale, bars    %-20s seed %d  %s" % (n, seed, "  ".join("%.3g" % stale[n, seed, d] for d in H.DELAYS)))
    assert max(v for (n, _, _), v in stale.items() if n in ("dc", "hum")) < 2
    assert max(v for (n, _, _), v in stale.items() if n == "lowpassed") > 50
    assert min(v for (n, _, _), v in stale.items() if n == "lowpassed") > 10


@pytest.mark.parametrize("matrix", list(H.MATRICES))
def test_apply_matrices(oracle, matrix):
    """The same three checks for ProcessMVDR under one caller matrix, over the loud blocks 9..17 of `white`: the FP64
    restatement is oracle.mvdr_apply, plain FP32 stays under 0.1 of the bar, the masks are equal; and the denominator
    c^H R^-1 c keeps 5e-7 of its largest magnitude at every bin, so no case hangs on a quotient of rounding errors."""
    L, R = H.loud_blocks(*H.cached_scene("white"))
    corr = np.array(H.MATRICES[matrix])
    for d_time in H.APPLY_DELAYS:
        o_out, o_pre = oracle.mvdr_apply(L, R, corr, d_time)
        assert o_pre.size == 8 * 512 and np.isfinite(o_pre).all()
        r = H.apply_ref64(L, R, corr, d_time)
        s64, same64 = H.share(r["pre"], o_pre)
        s32, same32 = H.share(H.apply_ref32(L, R, corr, d_time)["pre"], o_pre)
        ratio = r["den"].min() / r["den"].max()
        print("apply, share of the bar %-14s d_time %-8g ref64 %.2e  ref32 %.4f  peak %.4g  min|den| / max|den| %.2e" % (
            matrix, d_time, s64, s32, np.abs(o_pre).max(), ratio))
        assert same64 and same32
        assert s64 < 1e-6
        assert s32 < 0.1
        assert ratio >= 5e-7


def test_vad_edge_blocks(oracle):
    """Energy sums of exactly 716,799, 716,800 and 716,801 = 700 x 1024 and its neighbours: quiet, quiet, voice (:233 is
    a strict comparison), and the stream built on them has the decisions it is meant to have."""
    blocks = H.vad_edge_blocks()
    assert blocks.dtype == np.int16 and blocks.shape == (3, 512)
    assert tuple(H.vad_sums(blocks)) == H.VAD_SUMS
    got = [oracle.mvdr_vad_block(b) for b in blocks]
    assert [g[0] for g in got] == [False, False, True]
    assert [g[1] * 1024 for g in got] == list(H.VAD_SUMS)
    assert np.count_nonzero(blocks[0] != blocks[1]) == 1 and np.count_nonzero(blocks[1] != blocks[2]) == 1
    L, R, flags = H.vad_edge_stream()
    assert np.array_equal(oracle_flags(oracle, L), flags)
    trace = oracle.mvdr_stream(L, R, 1e-4)[3]
    moved = np.flatnonzero(np.diff(trace[:, 0], prepend=0.0) != 0)
    assert list(moved) == list(range(1, 9)) + [19, 22]               # block 20 is voice: 21 starts a run, 22 is an event
