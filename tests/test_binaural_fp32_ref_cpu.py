"""What plain FP32 makes of the binaural renderer's hard streams (CPU): binaural_cases.Restate32 -- numpy's float32
rfft, complex64 spectra, never upcast -- on every (family, bank) pair and every scene of binaural_cases, against the FP64
reference and both bars.

These are conditions on the CHOICE OF INPUTS AND OF THE BAR, not measurements of the library: where plain FP32 stays
under half of the floored bar, a device miss is a kernel defect and not FP32's limit.  A pair that fails here is not to
be dropped: it would mean the floor is wrong.  Also asserted: on the pairs named in binaural_cases.BREAK_UNFLOORED plain
FP32 EXCEEDS the unfloored bar sum_c P_c (include/jdsp.h's earlier guarantee 1), so the floor is needed and not merely
convenient; the wrap scenes really wrap; the exact cancellation really is exact in the reference.

The table this prints (pytest -s) is recorded beside the device's figures in profiles/r22_binaural_streams.txt.
"""
import numpy as np
import pytest

import binaural_cases as B
import binaural_ref as R

HALF = 0.5


def pairs():
    return [(fam, bname) for bname in B.FAMILY_BANKS for fam in B.FAMILIES]


@pytest.fixture(scope="module")
def table():
    rows = {(fam, bname): B.family_fp32(bname)[fam] for fam, bname in pairs()}
    print("\nplain FP32 binaural overlap-save, worst error / bar (bank, family: floored, unfloored)")
    for (fam, bname), (qf, qu) in rows.items():
        print("  %-15s %-19s %8.4f %12.4f" % (bname, fam, qf, qu))
    return rows


def test_streams_and_banks_are_what_they_claim():
    for fam in B.FAMILIES:
        x = B.family(fam)
        assert x.dtype == np.int16 and x.shape == (B.BLOCK * B.N_BLOCKS,), fam
    lq = np.abs(B.family("loud_then_quiet").astype(np.int64)).reshape(B.N_BLOCKS, B.BLOCK).max(axis=1)
    assert lq[B.LOUD_BLOCK] > 20000 and np.delete(lq, B.LOUD_BLOCK).max() < 200       # quiet blocks follow the loud one
    on = np.abs(np.fft.rfft(B.family("sine_fs_on")[:1024].astype(np.float64)))
    assert on.argmax() == 131 and np.sort(on)[-2] < 1e-4 * on.max()                    # bin 131 exactly
    assert 8500 < B.family("full_white").astype(np.float64).std() < 9500 and B.family("nyquist")[:2].tolist() == [32000, -32000]
    hb = B.banks()
    assert abs(hb["highpass"][0, 0].sum()) < 1e-12 and not hb["one_ear"][:2, 1].any() and hb["one_ear"][2, 1].any()
    lc = np.abs(np.fft.rfft(hb["lowpass_contra"], 1024, axis=2))
    assert np.all(lc[:, 1, 0] < 0.011 * lc[:, 0, 0]) and np.all(lc[:, 1, 400:].max(axis=1) < 1e-4 * lc[:, 0].max(axis=1))
    assert np.allclose(np.sqrt((hb["noise200"] ** 2).sum(axis=2)), 0.25) and np.array_equal(hb["loud"], 8.0 * hb["noise200"])
    assert B.big_bank().shape == (16384, 2, 3)


def test_render3_keeps_the_parents_values_and_the_floor_is_the_stated_one():
    """out and bar are RefBinaural.render's bit for bit; F by hand on a single source: block by block
    max(P, 0.05 max|segment| |g| max_e sum|h|), the carried (d0, g0) counted on the faded block alone"""
    bank = B.banks()["noise200"]
    x = B.family("loud_then_quiet")
    a, b = B.RefFloored(bank, 2), R.RefBinaural(bank, 2)
    sum_h = np.abs(bank).sum(axis=2).max(axis=1)
    for k, (d, g) in enumerate(((0, 1.0), (2, 0.25))):
        args = ([1], [2560 * k], [d], np.float32([g]), [0, 1], [0, 5])
        prev = a.hist[1].copy()
        out, bar, floor = a.render3(x, *args)
        want, wbar = b.render(x, *args)
        assert np.array_equal(out, want) and np.array_equal(bar, wbar)
        xs = np.abs(np.concatenate([prev, x[2560 * k:2560 * (k + 1)]]).astype(np.float64))
        for blk in range(5):
            scale = g * sum_h[d] if not (k == 1 and blk == 0) else max(g * sum_h[d], 1.0 * sum_h[0])
            assert floor[blk] == max(bar[blk], 0.05 * xs[512 * blk:512 * blk + 1024].max() * scale)
    assert np.array_equal(a.hist, b.hist) and np.array_equal(a.gain, b.gain)
    with pytest.raises(AssertionError):                            # past int32 the cast is not specified
        B.RefFloored(bank, 1).render3(x, [0], [0], [0], np.float32([4e4]), [0, 1], [0, 1])


def test_restatement_in_fp64_is_the_reference():
    """the restatement's own structure is right: the same class on complex128 meets the reference to FP64 round-off"""
    s = B.scene("one_ear")
    got = []
    r = B.Restate32(s.bank, s.n_streams)
    for (pcm, args), (want, bar, floor, _) in zip(s.deliveries, B.scene_truth("one_ear")):
        y = r.render(pcm, *args)
        assert y.dtype == np.float32 and np.abs(y - want).max() < 1e-4 * bar.max()
        got.append(y)
    assert np.abs(got[1][:, :512] - got[3][:, :512]).max() > 10    # delivery 1 did fade


@pytest.mark.parametrize("fam,bname", pairs())
def test_plain_fp32_is_under_half_of_the_floored_bar(table, fam, bname):
    qf, qu = table[fam, bname]
    assert qf <= HALF, (fam, bname, qf)


@pytest.mark.parametrize("fam,bname", B.BREAK_UNFLOORED)
def test_plain_fp32_exceeds_the_unfloored_bar(table, fam, bname):
    qf, qu = table[fam, bname]
    assert qu > 1.0 and qf <= HALF, (fam, bname, qu, qf)
    assert not B.holds_unfloored(bname, fam)


def test_silence_is_exact():
    for bname in B.FAMILY_BANKS:
        want, bar, floor = B.family_truth(bname)
        i = B.FAMILIES.index("silence")
        assert not floor[B.N_BLOCKS * i:B.N_BLOCKS * (i + 1)].any() and B.family_fp32(bname)["silence"] == (0.0, 0.0)


@pytest.mark.parametrize("name", list(B.scenes()))
def test_plain_fp32_is_under_half_of_the_floored_bar_on_the_scenes(name):
    truth = B.scene_truth(name)
    for k, (qf, qu, y) in enumerate(B.scene_fp32(name)):
        want = truth[k][0]
        own, far = B.int16_rules(B.cast_i16(y), y, want)
        print("  %-22s delivery %d: plain FP32 %8.4f of the floored bar, %10.4f of the unfloored; int16 > 1 step off: %d"
              % (name, k, qf, qu, far))
        assert qf <= HALF and far == 0, (name, k, qf, far)


def test_the_scenes_are_what_they_claim():
    w = B.scene_truth("wrap17")[0][0]
    assert np.count_nonzero(np.abs(w) > 32768.0) >= 1000 and np.count_nonzero(np.abs(w) > 98304.0) > 0
    w = B.scene_truth("wrap_gain8")[0][0]
    assert np.count_nonzero(np.abs(w) > 32768.0) >= 500
    for want, bar, floor, _ in B.scene_truth("cancel"):
        assert not want.any() and np.all(bar > 1000)              # the exact sum is 0, the bar 2 P
    t = B.scene_truth("signed_zero")
    assert np.abs(t[1][0][:, :64]).max() > 100 and np.abs(t[1][0][:, -1]).max() < 0.01 * np.abs(t[1][0]).max() and not t[2][0].any() and not t[2][2].any() and not t[3][2].any()
    assert R.bits(t[1][3][2])[0] == 0 and R.bits(t[2][3][2])[0] == 0x80000000
    for want, bar, floor, _ in B.scene_truth("one_ear"):
        assert not want[1, :1024].any() and want[0, :1024].any()
    assert np.abs(B.scene_truth("one_ear")[1][0][1, 1024:1536]).max() > 10       # mix 1 fades INTO the two-eared direction
    t = B.scene_truth("seam_fade_noise1")[1]
    assert t[2][0] > 10 * t[1][0]                                  # on the seam the floor carries the bar
    for n, moved in B.MANY:
        w = np.concatenate([t[0] for t in B.scene_truth("many%d_moved%d" % (n, moved))], axis=1)
        assert np.abs(w).max() < 30000.0, (n, moved)
