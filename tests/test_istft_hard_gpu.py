"""STFT synthesis (jdsp_istft_*) on the spectra white noise does not reach (istft_cases.py holds the cases and the bars;
test_istft_hard_cpu.py shows on the CPU what plain FP32 makes of them): a basis sweep over every bin, shaped single
frames, non-Hermitian rows, loud frames beside frames 60-120 dB lower, a loud stretch under call cuts and launch
geometries, zero rows, one row at several positions, power-of-two scaling, non-finite values and the white control, at
all six (n, hop), both layouts and every window pair create accepts.

Bars, each on every sample of the float32 output and tail: the stream bar 1e-5 P g (as test_istft_gpu.py) and the frame
bar 1e-5 g sum_f P_f |w_s[t - hop f]|, which holds a quiet frame to its own peak; int16 = the cast of the device's own
float, bit for bit, and within +-1 LSB of the cast of the restatement on every sample.  The bit-identities the header
promises (call cuts, frames_per_wave, host = device, batch = fresh handles, live = single stream) are asserted on these
streams too.

Figures, worst per family as (stream bar, frame bar), plain FP32 on the CPU first and the device second
(profiles/r28_istft_hard.txt has the table per case): basis sweep 0.044, 0.029 / 0.047, 0.037; shaped frames 0.029,
0.033 / 0.033, 0.037; non-Hermitian rows 0.024, 0.024 / 0.027, 0.024; loud beside quiet 0.038, 0.034 / 0.043, 0.038; the
loud stretch 0.027, 0.021 / 0.033, 0.024; zero rows among loud ones 0.018, 0.021 / 0.018, 0.024; position 0.020, 0.022 /
0.021, 0.025; the clean twins of the non-finite runs 0.025, 0.022 / 0.022, 0.022; the white control 0.029, 0.023 / 0.035,
0.029.  No case came near a bar and no kernel changed.

Non-finite values.  "No sample of the poisoned frame stays finite" is asserted as it stands for a NaN or +Inf in the
real part of bin 0 or n/2, which enters every sample with weight +-1.  For a value in a bin in between it is asserted
wherever the component's weight cos / sin (2 pi k i / n) is not exactly zero; where it is zero the sample must be
non-finite or equal the clean twin's bit for bit.  The 512-point inverse turns by +-j with a swap and multiplies by no
zero, so there 2 of 512 samples (odd k; 8 for k = 64) keep their clean value; the 1024-point frames go through the
pre-split's products and come out non-finite everywhere (istft_cases.py, family 9, has the reasoning).
"""
import numpy as np
import pytest

import istft_cases as K
from test_istft_gpu import cast_i16, rows, run
from test_istft_batch_gpu import SENT_F, SENT_I, Batch, cfg_of, run_batch
from test_istft_streams_gpu import Streams, feed
from test_stftmask_streams_gpu import N_STREAMS, flush_all, plan_of

pytestmark = pytest.mark.gpu

CASES = K.cases()
IDS = [c["name"] for c in CASES]
SUBSET = K.subset()
COMBOS = [(n, hop, layout) for n, hop in K.CONFIGS for layout in K.LAYOUTS]
_OUT = {}


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def ibits(a):
    return np.ascontiguousarray(a).view(np.int32)


def whole(eng, spec, cfg):
    """(int16, float32) of a fresh handle's process + flush of `spec`, tail included"""
    o, f, to, tf = run(eng, np.array(spec), **cfg)
    return np.concatenate([o, to]), np.concatenate([f, tf])


def device_out(eng, ci):
    """whole() of case ci under its own windows, computed once and shared (read-only)"""
    if ci not in _OUT:
        _OUT[ci] = whole(eng, CASES[ci]["spec"], K.cfg_of_case(CASES[ci]))
        for a in _OUT[ci]:
            a.setflags(write=False)
    return _OUT[ci]


def fpws(R):
    return sorted({max(R - 1, 1), 3, 7, 0})


def check(got_f, got_i, bars, what):
    """Both bars and the two int16 rules; prints the figures before it asserts."""
    want = bars[0]
    rs, rf = K.ratios_of(got_f, bars)
    print("%s: %.4f of the stream bar, %.4f of the frame bar, largest |g s| %.1f" % (what, rs, rf, np.abs(want).max() if want.size else 0))
    assert rs <= 1.0 and rf <= 1.0, (what, rs, rf)
    assert np.array_equal(got_i, cast_i16(got_f.astype(np.float32))), what        # the device's own float, bit for bit
    d = got_i.astype(np.int64) - cast_i16(want).astype(np.int64)
    assert np.all(np.abs(d) <= 1), (what, np.abs(d).max())                         # every sample, no exclusions
    return rs, rf


def exactly_zero(f, i):
    """no bit set apart from the sign; the int16 samples zero"""
    return not (ibits(f) & 0x7FFFFFFF).any() and not np.asarray(i).any()


# ---- 1. every case, both bars --------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_case_holds_both_bars(eng, ci):
    c = CASES[ci]
    n, hop = c["n"], c["hop"]
    got_i, got_f = device_out(eng, ci)
    check(got_f.astype(np.float64), got_i, K.truth(ci), c["name"])
    if c["fam"] == 6:
        if len(c["zero_rows"]) == c["F"]:
            assert exactly_zero(got_f, got_i)
        else:                                                  # hop = n: a zero row is a block of exact zeros
            for f in c["zero_rows"]:
                assert exactly_zero(got_f[n * f:n * f + n], got_i[n * f:n * f + n]), f
            assert got_f.any()
    if c["fam"] == 3:
        (f,) = c["zero_rows"]
        if hop == n:                                           # nothing else adds into the anti-Hermitian row's block
            assert np.all(got_f[n * f:n * f + n] == 0) and not got_i[n * f:n * f + n].any()
        zeroed = np.array(c["spec"])
        zeroed[f] = 0                                          # it adds exact zeros wherever it adds
        zi, zf = whole(eng, zeroed, K.cfg_of_case(c))
        assert np.array_equal(zi, got_i) and np.all(zf == got_f)
        assert np.array_equal(ibits(zf) & 0x7FFFFFFF, ibits(got_f) & 0x7FFFFFFF)


# ---- 2. position and neighbours (family 7) ---------------------------------------------------------------------------
POSITION = [i for i, c in enumerate(CASES) if c["fam"] == 7]


@pytest.mark.parametrize("ci", POSITION, ids=[IDS[i] for i in POSITION])
def test_a_row_gives_the_same_samples_wherever_it_stands(eng, ci):
    import torch
    c = CASES[ci]
    n, hop, layout = c["n"], c["hop"], c["layout"]
    R = n // hop
    cfg = K.cfg_of_case(c)
    pos = c["positions"]
    ref = device_out(eng, ci)[1][hop * pos[0]: hop * pos[0] + n]
    assert np.abs(ref).max() > 100.0

    def same(f, first, what):
        for p in pos:
            seg = f[first + hop * p: first + hop * p + n]
            assert np.all(seg == ref), (what, p, int(np.count_nonzero(seg != ref)))     # ==: -0.0 equals +0.0

    spec = torch.from_numpy(np.array(c["spec"])).cuda()
    ist = eng.istft(**cfg)
    for fpw in fpws(R):
        ist.set_option("frames_per_wave", fpw)
        _, f = ist.process(spec, want_f32=True)
        _, tf = ist.flush(want_f32=True)
        torch.cuda.synchronize()
        same(torch.cat([f, tf]).cpu().numpy(), 0, ("stream", fpw))
    # the batch entry: the stream as the third of four utterances, behind loud frames and an empty utterance
    b = Batch(np.random.default_rng(ci), n, hop, layout, [5, 0, c["F"], 1])
    b.spec = np.ascontiguousarray(np.concatenate([c["spec"][:5], c["spec"], c["spec"][:1]]))
    for fpw in fpws(R):
        _, f = run_batch(ist, b, fpw)
        same(f, int(b.offs[2]), ("batch", fpw))
    # the live entry: the stream in three chunks, a loud stream's chunks beside them in the same calls
    F = c["F"]
    cut = [pos[0] + 1, pos[1] - pos[0], F - pos[1] - 1]         # a call ends on the row, the next starts behind it
    ist.open_streams(2)
    for fpw in fpws(R):
        ist.set_option("frames_per_wave", fpw)
        parts, at = [], 0
        for k, m in enumerate(cut):
            loud = np.array(CASES[ci]["spec"][:3])
            chunk = np.array(c["spec"][at:at + m])
            order = [(1, loud), (0, chunk)] if k % 2 == 0 else [(0, chunk), (1, loud)]
            _, f = ist.process_streams(torch.from_numpy(np.concatenate([r for _, r in order])).cuda(),
                                       [s for s, _ in order], [r.shape[0] for _, r in order], want_f32=True)
            torch.cuda.synchronize()
            f = f.cpu().numpy()
            first = 0 if order[0][0] == 0 else hop * 3
            parts.append(f[first:first + hop * m].copy())
            at += m
        _, ff = flush_all(ist, 2)
        same(np.concatenate(parts + [ff[0]]), 0, ("live", fpw))
    ist.close()


# ---- 3. power-of-two scale (family 8) --------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,k", K.scale_runs(), ids=["%s@%+d" % (IDS[i], k) for i, k in K.scale_runs()])
def test_power_of_two_scale_is_exact(eng, ci, k):
    c = CASES[ci]
    base = device_out(eng, ci)[1]
    _, got = whole(eng, K.scaled(c["spec"], k), K.cfg_of_case(c))
    want = np.ldexp(base, k).astype(np.float32)
    assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= K.TINY).all()
    bad = ibits(got) != ibits(want)
    assert not bad.any(), (c["name"], k, int(bad.sum()), int(np.flatnonzero(bad)[0]))


# ---- 4. non-finite values (family 9) -----------------------------------------------------------------------------------
POISON = [i for i, c in enumerate(CASES) if c["fam"] == 9]


def check_poisoned(a_i, a_f, b_i, b_f, lo, hi, what, zero_weight=None):
    """A against B: bit-identical outside [lo, hi); inside, no finite float and int16 0 wherever the float is NaN.
    zero_weight (bool [hi - lo]): the samples the poisoned component enters with weight exactly zero -- there the
    sample may instead equal B's, bit for bit."""
    out = np.ones(a_f.size, bool)
    out[lo:hi] = False
    assert np.array_equal(a_i[out], b_i[out]), (what, "int16 outside")
    assert np.array_equal(ibits(a_f)[out], ibits(b_f)[out]), (what, "float32 outside")
    finite = np.isfinite(a_f[lo:hi])
    print("%s: %d of %d samples inside are finite" % (what, int(finite.sum()), hi - lo))
    if zero_weight is None:
        assert hi > lo and not finite.any(), (what, int(finite.sum()), "finite inside")
    else:
        assert not finite[~zero_weight].any(), (what, int(finite[~zero_weight].sum()), "finite under a weight that is not zero")
        assert np.array_equal(ibits(a_f[lo:hi])[finite], ibits(b_f[lo:hi])[finite]), (what, "finite and not the clean value")
        assert np.array_equal(a_i[lo:hi][finite], b_i[lo:hi][finite]), (what, "finite and not the clean int16")
    assert not a_i[lo:hi][np.isnan(a_f[lo:hi])].any(), (what, "int16 of a NaN")
    assert np.isfinite(b_f).all()


@pytest.mark.parametrize("ci", POISON, ids=[IDS[i] for i in POISON])
def test_a_non_finite_value_stays_in_its_frame(eng, ci):
    import torch
    c = CASES[ci]
    n, hop, layout = c["n"], c["hop"], c["layout"]
    cfg = K.cfg_of_case(c)
    f = c["poison"][0]
    A, B = K.poisoned(c), np.array(c["spec"])
    b_i, b_f = device_out(eng, ci)
    a_i, a_f = whole(eng, A, cfg)
    check_poisoned(a_i, a_f, b_i, b_f, hop * f, hop * f + n, (c["name"], c["poison"]))
    m_i, m_f = whole(eng, K.poisoned(c, "poison_mid"), cfg)    # a bin in between: weight zero in some samples
    check_poisoned(m_i, m_f, b_i, b_f, hop * f, hop * f + n, (c["name"], c["poison_mid"]),
                   K.zero_weight(n, *c["poison_mid"][1:3]))
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()

    def clean(ist, what):
        o, fl = ist.process(dB, want_f32=True)
        to, tf = ist.flush(want_f32=True)
        torch.cuda.synchronize()
        assert np.array_equal(torch.cat([o, to]).cpu().numpy(), b_i), (what, "int16")
        assert np.array_equal(ibits(torch.cat([fl, tf]).cpu().numpy()), ibits(b_f)), (what, "float32")

    # the handle after the poisoned stream: the call ends on the poisoned row, so the carried tail holds it
    ist = eng.istft(**cfg)
    ist.process(dA[:f + 1])
    ist.reset()
    clean(ist, "after reset")
    ist.process(dA[:f + 1])
    ist.flush()
    clean(ist, "after flush")
    # one live stream poisoned, a second fed clean rows in the same calls
    k = f + 1
    for how in ("flush", "reset"):
        ist.open_streams(2)
        _, f1 = ist.process_streams(torch.cat([dA[:k], dB[:k]]), [0, 1], [k, k], want_f32=True)
        if how == "flush":
            ist.flush_streams([0])
        else:
            ist.reset_streams([0])
        F = c["F"]
        o2, f2 = ist.process_streams(torch.cat([dB[k:], dB]), [1, 0], [F - k, F], want_f32=True)
        fi, ff = flush_all(ist, 2)
        f1, o2, f2 = f1.cpu().numpy(), o2.cpu().numpy(), f2.cpu().numpy()
        one = np.concatenate([f1[hop * k:], f2[:hop * (F - k)], ff[1]])
        assert np.array_equal(ibits(one), ibits(b_f)), (how, "the clean stream beside the poisoned one")
        again = np.concatenate([f2[hop * (F - k):], ff[0]])
        assert np.array_equal(ibits(again), ibits(b_f)), (how, "the poisoned stream, started again")
        assert np.array_equal(np.concatenate([o2[hop * (F - k):], fi[0]]), b_i), (how, "int16")
    ist.close()
    # a batch whose last utterance's last row is poisoned
    frames = [5, 0, 1, 9]
    bt = Batch(np.random.default_rng(ci), n, hop, layout, frames)
    clean_rows = np.ascontiguousarray(np.delete(B, f, axis=0)[:15])
    bad = clean_rows.copy()
    bad[14] = A[f]
    clean_rows[14] = 0
    ist = eng.istft(**cfg)
    bt.spec = clean_rows
    bb_i, bb_f = run_batch(ist, bt)
    bt.spec = bad
    ba_i, ba_f = run_batch(ist, bt)
    ist.close()
    at = int(bt.offs[3]) + hop * 8
    check_poisoned(ba_i, ba_f, bb_i, bb_f, at, at + n, (c["name"], "batch"))
    if layout == "half":                                       # Im of bins 0 and n/2 is ignored, whatever it holds
        poked = B.copy()
        poked.imag[::2, 0], poked.imag[1::2, 0] = np.nan, -np.inf
        poked.imag[::3, n // 2], poked.imag[1::3, n // 2] = np.inf, np.nan
        assert not np.isfinite(poked[:, 0].imag).any() and np.array_equal(poked.real, B.real)
        p_i, p_f = whole(eng, poked, cfg)
        assert np.array_equal(p_i, b_i) and np.array_equal(ibits(p_f), ibits(b_f))


# ---- 5. the bit-identities on these streams ----------------------------------------------------------------------------
@pytest.mark.parametrize("ci", SUBSET, ids=[IDS[i] for i in SUBSET])
def test_cuts_geometries_and_host_bit_identical(eng, ci):
    import torch
    c = CASES[ci]
    F, R = c["F"], c["n"] // c["hop"]
    spec = torch.from_numpy(np.array(c["spec"])).cuda()
    ist = eng.istft(**K.cfg_of_case(c))
    o1, f1 = ist.process(spec, want_f32=True)
    t1, tf1 = ist.flush(want_f32=True)
    torch.cuda.synchronize()
    ref_i, ref_f = device_out(eng, ci)
    assert np.array_equal(torch.cat([o1, t1]).cpu().numpy(), ref_i)

    def same(parts, fparts, t2, tf2, what):
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts), o1), what
        assert torch.equal(torch.cat(fparts).view(torch.int32), f1.view(torch.int32)), what
        assert torch.equal(t2, t1) and torch.equal(tf2.view(torch.int32), tf1.view(torch.int32)), what

    def in_calls(cuts, what):
        parts, fparts, j = [], [], 0
        for k in cuts:
            o, f = ist.process(spec[j:j + k], want_f32=True)
            parts.append(o)
            fparts.append(f)
            j += k
        assert j == F
        same(parts, fparts, *ist.flush(want_f32=True), what=what)

    for k in range(1, F):                                      # one cut, at every frame
        in_calls([k, F - k], ("cut at", k))
    in_calls([1] * F, "one frame per call")
    for fpw in fpws(R):
        ist.set_option("frames_per_wave", fpw)
        o, f = ist.process(spec, want_f32=True)
        same([o], [f], *ist.flush(want_f32=True), what=("frames_per_wave", fpw))
    ist.set_option("frames_per_wave", 0)
    oh, fh = ist.process(np.array(c["spec"]), want_f32=True)   # the host entry
    th, tfh = ist.flush(want_f32=True)
    assert np.array_equal(np.concatenate([oh, th]), ref_i)
    assert np.array_equal(ibits(np.concatenate([fh, tfh])), ibits(ref_f))
    ist.close()


# ---- 6. the loud stretch under cuts and run boundaries (family 5) ------------------------------------------------------
STRETCH = [i for i, c in enumerate(CASES) if c["fam"] == 5]


@pytest.mark.parametrize("ci", STRETCH, ids=[IDS[i] for i in STRETCH])
def test_loud_stretch_under_cuts_and_run_boundaries(eng, ci):
    """Frames 8..15 are loud.  A call that starts at frame 16 or 17 recomputes loud frames in its halo and emits quiet
    ones; one that starts at 8 or 9 has a quiet halo under loud frames; runs of R - 1, R and 5 frames put run boundaries
    at the same places inside a call."""
    import torch
    c = CASES[ci]
    F, R = c["F"], c["n"] // c["hop"]
    spec = torch.from_numpy(np.array(c["spec"])).cuda()
    ref_i, ref_f = device_out(eng, ci)
    ist = eng.istft(**K.cfg_of_case(c))
    plans = [[F], [7, 1, 1, 6, 1, 1, F - 17]] + [[k, F - k] for k in (7, 8, 9, 15, 16, 17)]
    for fpw in sorted({max(R - 1, 1), R, 5, 0}):
        ist.set_option("frames_per_wave", fpw)
        for cuts in plans:
            parts, fparts, j = [], [], 0
            for k in cuts:
                o, f = ist.process(spec[j:j + k], want_f32=True)
                parts.append(o)
                fparts.append(f)
                j += k
            t, tf = ist.flush(want_f32=True)
            torch.cuda.synchronize()
            assert np.array_equal(torch.cat(parts + [t]).cpu().numpy(), ref_i), (fpw, cuts)
            assert np.array_equal(ibits(torch.cat(fparts + [tf]).cpu().numpy()), ibits(ref_f)), (fpw, cuts)
    ist.close()


# ---- 7. the batch and the live entries ---------------------------------------------------------------------------------
def rows_of(n, hop, layout, fam, name=None):
    """The spectrum rows of the first case of a family at a configuration, in the layout's bins"""
    c = next(c for c in CASES if (c["n"], c["hop"], c["layout"], c["fam"]) == (n, hop, layout, fam)
             and (name is None or c["name"].startswith(name)))
    return np.array(c["spec"][:, :K.bins_of(n, layout)])


@pytest.mark.parametrize("n,hop,layout", COMBOS)
def test_batch_equals_fresh_handles(eng, n, hop, layout):
    R = n // hop
    utts = [rows_of(n, hop, layout, 4, "loudquiet_white"), rows_of(n, hop, layout, 10), rows_of(n, hop, layout, 2)[:1],
            rows_of(n, hop, layout, 10)[:0], rows_of(n, hop, layout, 5), rows_of(n, hop, layout, 4, "loudquiet_tone"),
            rows_of(n, hop, layout, 6, "zeros-"), rows_of(n, hop, layout, 7)]
    b = Batch(np.random.default_rng(0), n, hop, layout, [u.shape[0] for u in utts])
    b.spec = np.ascontiguousarray(np.concatenate(utts))
    cfg = cfg_of(n, hop, layout)
    ref = b.reference(eng, cfg)
    ist = eng.istft(**cfg)
    for fpw in fpws(R):
        o, f = run_batch(ist, b, fpw)
        b.check(o, f, ref, SENT_I, SENT_F, (n, hop, layout, "frames_per_wave", fpw))
    ist.close()


@pytest.mark.parametrize("n,hop,layout", COMBOS)
def test_live_streams_equal_single_streams(eng, n, hop, layout):
    R = n // hop
    cfg = cfg_of(n, hop, layout)
    st = Streams(np.random.default_rng(0), n, hop, layout, [23, 9, 4, 1, 2 * R + 1, 0])
    quiet = rows_of(n, hop, layout, 5)
    st.spec = [rows_of(n, hop, layout, 4, "loudquiet_white")[:23],              # loud, every other frame 60-120 dB down
               np.ascontiguousarray(np.concatenate([quiet[:8], quiet[16:17]])),   # quiet: 80 dB under the others
               rows_of(n, hop, layout, 2)[:4], rows_of(n, hop, layout, 10)[:1], rows_of(n, hop, layout, 7)[:2 * R + 1],
               rows(np.random.default_rng(1), 1, n, st.bins)]
    assert [s.shape[0] for s in st.spec[:5]] == st.totals[:5]
    plan = plan_of(R)
    ref = st.reference(eng, cfg)
    ist = eng.istft(**cfg)
    ist.open_streams(N_STREAMS)
    for fpw in fpws(R):
        ist.set_option("frames_per_wave", fpw)
        st.rewind()
        for k, chunks in enumerate(plan):
            feed(ist, st, chunks, (n, hop, layout, fpw, "call", k))
        fi, ff = flush_all(ist, N_STREAMS)
        st.check(fi, ff, ref, (n, hop, layout, "frames_per_wave", fpw))
    ist.close()
