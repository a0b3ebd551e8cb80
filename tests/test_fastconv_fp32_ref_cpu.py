"""What plain FP32 makes of the convolver's hard streams (CPU): fastconv_cases.restate32 -- numpy's float32 rfft,
complex64 spectra, never upcast -- on every (filter, family) pair of fastconv_cases, against the oracle and both bars.

These are conditions on the CHOICE OF INPUTS, not measurements of the library: if plain FP32 stays under a quarter of
both bars on a pair, a device miss on that pair is a kernel defect and not FP32's limit.  A pair that fails here is to be
changed, not the bar.  Also asserted: the wrap filters really wrap (pre-cast values past +-32768 and past +-98304 on the
full-scale square), and the local bar really is two orders of magnitude under the global one on the quiet stretches of
loud_then_quiet.

The table this prints (pytest -s) is recorded beside the device's figures in profiles/r20_fastconv_streams.txt.
"""
import numpy as np
import pytest

import fastconv_cases as K

QUARTER = 0.25


def pairs():
    return [(fname, fam) for fname in K.filters() for fam in K.FAMILIES]


@pytest.fixture(scope="module")
def table(oracle):
    """(filter, family) -> (fraction of the global bar, of the local bar, int16 samples off their own cast, int16
    samples more than one step from the oracle's), the worst over the filter's rows"""
    rows = {}
    for fname, fam in pairs():
        n_fft, h = K.filters()[fname]
        x = K.stream(fname, fam)
        worst = [0.0, 0.0, 0, 0]
        for f in range(h.shape[0]):
            t = K.truth(oracle, fname, fam, f)
            y = K.restate32(x, h[f], n_fft)
            g, loc = K.ratios_of(y, t)
            own, far = K.int16_rules(K.cast_i16(y), y, t)
            worst = [max(worst[0], g), max(worst[1], loc), worst[2] + own, worst[3] + far]
        rows[fname, fam] = tuple(worst)
    print("\nplain FP32 overlap-save, worst fraction of each bar (filter, family: global, local, int16 > 1 step off)")
    for (fname, fam), (g, loc, own, far) in rows.items():
        print("  %-15s %-19s %8.4f %8.4f %6d" % (fname, fam, g, loc, far))
    return rows


def test_every_stream_has_output_and_every_filter_stays_inside_int32(oracle):
    for fname, (n_fft, h) in K.filters().items():
        s = K.shape_for(fname)
        assert s.n_blocks - s.hist_blocks >= 8, (fname, s)
        assert 32768.0 * np.abs(h).sum(axis=1).max() < 2.0 ** 31, fname
    assert K.shape_for("taps200x3").block == 825 and K.shape_for("taps7000").block == 1193
    assert K.shape_for("taps7681x2").block == 512 and K.shape_for("dense7169").block == 1024
    assert K.shape_for("hrir2").block == 769 and abs(K.filters()["highpass"][1].sum()) < 1e-12


def test_restatement_is_the_oracles_convolution(oracle):
    """the restatement in FP64 arithmetic is the oracle to FP64 round-off: segments, silent head and kept samples are right"""
    for fname in ("hrir2", "taps1024", "taps7000"):
        n_fft, h = K.filters()[fname]
        x = K.stream(fname, "white")
        s = K.shape_for(fname)
        H = np.fft.rfft(np.concatenate([h[0], np.zeros(n_fft - h.shape[1])]))
        y = np.fft.irfft(np.fft.rfft(K.segments(x, s).astype(np.float64), axis=1) * H, n=n_fft, axis=1)[:, h.shape[1] - 1:]
        t = K.truth(oracle, fname, "white")
        assert np.abs(y.reshape(-1) - t.pre).max() < 1e-9 * np.abs(t.pre).max()


@pytest.mark.parametrize("fname,fam", pairs())
def test_plain_fp32_meets_both_bars_with_room(table, fname, fam):
    g, loc, own, far = table[fname, fam]
    assert g <= QUARTER and loc <= QUARTER, (fname, fam, g, loc)


def test_silence_is_exact(oracle, table):
    for fname in K.filters():
        t = K.truth(oracle, fname, "silence")
        assert not t.pre.any() and not t.out.any() and not t.local_bar.any()
        assert table[fname, "silence"][:2] == (0.0, 0.0)


def test_the_wrap_filters_wrap(oracle):
    for fname in K.WRAP_FILTERS:
        n_fft, h = K.filters()[fname]
        for f in range(h.shape[0]):
            w = K.truth(oracle, fname, "full_square", f).pre
            assert np.count_nonzero(np.abs(w) > 32768.0) >= 1000, (fname, f)
            assert np.count_nonzero(np.abs(w) > 98304.0) > 0, (fname, f)


def test_the_local_bar_is_tighter_where_the_stream_is_quiet(oracle):
    for fname in K.filters():
        t = K.truth(oracle, fname, "loud_then_quiet")
        gain = t.global_bar / t.local_bar.min()
        print("%-15s loud_then_quiet: the local bar is up to %.0f times under the global one" % (fname, gain))
        # 1024 taps: blocks of one sample, and every one of the stream's 177 outputs has the loud stretch inside its
        # 1024-sample segment -- that shape has no quiet stretch to judge
        assert gain >= 100.0 or fname == "taps1024", (fname, gain)


@pytest.mark.parametrize("fname", K.LONG_8192)
def test_long_8192_streams_put_quiet_output_behind_the_loud_stretch(oracle, fname):
    """the 8192-point streams on which the loud sixth comes first: plain FP32 under a quarter of both bars there too,
    and the local bar two orders under the global one on output whose whole segment follows the loud stretch"""
    n_fft, h = K.filters()[fname]
    nb = K.LONG_8192[fname]
    s = K.shape_for(fname, nb)
    lo, hi = K.loud_span(s)
    assert lo >= (s.hist_blocks + 2) * s.block and hi < s.n_blocks * s.block - s.n_fft - 2 * s.block
    x = K.stream(fname, "loud_then_quiet", nb)
    t = K.truth(oracle, fname, "loud_then_quiet", 0, n_blocks=nb)
    g, loc = K.ratios_of(K.restate32(x, h[0], n_fft), t)
    after = t.local_bar[hi + s.n_fft - s.hist_blocks * s.block:]
    print("\n  %-15s loud_then_quiet %d blocks %8.4f %8.4f; behind the loud stretch the local bar is %.0f times under the "
          "global one" % (fname, nb, g, loc, t.global_bar / after.min()))
    assert g <= QUARTER and loc <= QUARTER
    assert after.size >= s.block and t.global_bar / after.min() >= 100.0
