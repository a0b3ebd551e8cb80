"""Batched reverberation on the device (jdsp_reverb_batch*, include/jdsp.h "batched reverberation"): every bank's batch of
reverb_cases against the FP64 direct convolution under both bars and the int16 rules; the independence promises,
compared as bytes in both outputs; the partitioned jdsp_fastconv path beside it on the same stream; every error and edge
the header names.  What plain FP32 makes of the same cases: test_reverb_fp32_ref_cpu.py.

Figures printed here (pytest -s) are recorded in profiles/r29_reverb_batch.txt."""
import ctypes as C

import numpy as np
import pytest

import fastconv_cases as F
import reverb_cases as K
import reverb_ref

pytestmark = pytest.mark.gpu
SENT_I = np.int16(0x5A5A)
SENT_F = np.float32(-7.25e11)


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def handles(eng):
    """one handle per bank, made on first use and shared"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = eng.reverb(K.banks()[name])
        return made[name]
    yield get
    for h in made.values():
        h.close()


def run(rv, pcm, sample_first, block_first, ir, gain, sentinel=True):
    """the device entry on sentinel-filled outputs: (int16, float32) numpy, pcm's length"""
    import torch
    n = pcm.size
    o16 = torch.full((max(n, 1),), int(SENT_I), dtype=torch.int16, device="cuda")
    o32 = torch.full((max(n, 1),), float(SENT_F), dtype=torch.float32, device="cuda")
    if not sentinel:
        o16.zero_(), o32.zero_()
    a, b = rv.process_batch(torch.from_numpy(np.ascontiguousarray(pcm)).cuda(), sample_first, block_first,
                            np.asarray(ir, np.int32), None if gain is None else np.asarray(gain, np.float32),
                            want_f32=True, out=o16, out_f32=o32)
    torch.cuda.synchronize()
    return a.cpu().numpy(), b.cpu().numpy()


def spans_of(utts, first):
    return [(int(a), int(a) + x.size) for x, a in zip(utts, first)]


def outside_is_sentinel(o16, o32, spans):
    keep = np.ones(o16.size, bool)
    for a, b in spans:
        keep[a:b] = False
    assert np.all(o16[keep] == SENT_I), "int16 written outside the spans"
    assert np.all(o32[keep].view(np.int32) == SENT_F.view(np.int32)), "float32 written outside the spans"


def per_utt(o16, o32, spans):
    return [(o16[a:b].tobytes(), o32[a:b].tobytes()) for a, b in spans]


# ---- 3: accuracy and the int16 rules ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.banks()))
def test_every_utterance_holds_both_bars_and_the_int16_rules(handles, name):
    b = K.batch(name)
    rv = handles(name)
    assert rv.n_part == K.n_part(b.taps.shape[1]) and rv.block == K.B and rv.n_irs == b.taps.shape[0]
    xs = [u.x for u in b.utts]
    pcm, first, bf = K.pack(xs, K.gaps_of(len(xs)), fill=32767, tail=514)      # loud samples between the spans
    o16, o32 = run(rv, pcm, first, bf, [u.ir for u in b.utts], [u.gain for u in b.utts])
    spans = spans_of(xs, first)
    outside_is_sentinel(o16, o32, spans)
    worst = [0.0, 0.0]
    for k, (u, (s0, s1)) in enumerate(zip(b.utts, spans)):
        g16, g32 = o16[s0:s1], o32[s0:s1]
        g, loc = K.ratios_of(g32, u)
        own, far = K.int16_rules(g16, g32, u)
        worst = [max(worst[0], g), max(worst[1], loc)]
        what = (name, k, u.family, u.x.size // K.B, u.ir, u.gain)
        assert g <= 1.0 and loc <= 1.0, (what, g, loc)
        assert own == 0 and far == 0, (what, own, far)
        if K.must_be_zero(u):                                  # silence in, or gain 0: exact zeros, either sign
            assert not g32.any() and not g16.any(), what
    print("\n  %-10s P = %2d, %2d utterances, %4d blocks: worst fraction of the global bar %.4f, of the local bar %.4f"
          % (name, rv.n_part, len(xs), int(bf[-1]), worst[0], worst[1]))


def test_the_host_entry_gives_the_same_bytes_and_zeros_outside_the_spans(handles):
    b = K.batch("taps513")
    rv = handles("taps513")
    xs = [u.x for u in b.utts]
    ir, gain = [u.ir for u in b.utts], [u.gain for u in b.utts]
    pcm, first, bf = K.pack(xs, K.gaps_of(len(xs)), fill=-32768, tail=100)
    d16, d32 = run(rv, pcm, first, bf, ir, gain, sentinel=False)
    h16, h32 = rv.process_batch(pcm, first, bf, ir, gain, want_f32=True)
    assert h16.tobytes() == d16.tobytes() and h32.tobytes() == d32.tobytes()
    keep = np.ones(pcm.size, bool)
    for s0, s1 in spans_of(xs, first):
        keep[s0:s1] = False
    assert keep.sum() > 1000 and not h16[keep].any() and not h32[keep].any()
    only16 = rv.process_batch(pcm, first, bf, ir, gain)
    assert only16.tobytes() == h16.tobytes()


# ---- 4: independence, as bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["taps513", "dense7680"])
def test_an_utterance_does_not_depend_on_its_company(handles, name):
    b = K.batch(name)
    rv = handles(name)
    xs = [u.x for u in b.utts]
    ir = np.array([u.ir for u in b.utts], np.int32)
    gain = np.array([u.gain for u in b.utts], np.float32)
    n = len(xs)
    pcm, first, bf = K.pack(xs)
    base = per_utt(*run(rv, pcm, first, bf, ir, gain), spans_of(xs, first))
    assert len({t for t in base if t[0]}) > n // 2              # the utterances do differ

    # alone, at sample 0
    for k in range(n):
        p1, f1, b1 = K.pack([xs[k]])
        got = per_utt(*run(rv, p1, f1, b1, ir[k:k + 1], gain[k:k + 1]), spans_of([xs[k]], f1))
        assert got[0] == base[k], ("alone", name, k)

    # permuted
    perm = np.random.default_rng(7).permutation(n)
    xp = [xs[i] for i in perm]
    pp, fp, bp = K.pack(xp)
    got = per_utt(*run(rv, pp, fp, bp, ir[perm], gain[perm]), spans_of(xp, fp))
    for j, i in enumerate(perm):
        assert got[j] == base[i], ("permuted", name, i)

    # gaps of loud samples between the spans, sentinels in the outputs
    pg, fg, bg = K.pack(xs, K.gaps_of(n)[::-1], fill=-32768, tail=258)
    o16, o32 = run(rv, pg, fg, bg, ir, gain)
    outside_is_sentinel(o16, o32, spans_of(xs, fg))
    assert per_utt(o16, o32, spans_of(xs, fg)) == base, ("gaps", name)

    # split into two calls
    cut = n // 2 + 1
    got = []
    for lo, hi in ((0, cut), (cut, n)):
        ps, fs, bs = K.pack(xs[lo:hi])
        got += per_utt(*run(rv, ps, fs, bs, ir[lo:hi], gain[lo:hi]), spans_of(xs[lo:hi], fs))
    assert got == base, ("split", name)

    # the neighbours' responses and gains changed
    for parity in (0, 1):
        ir2, gain2 = ir.copy(), gain.copy()
        others = np.arange(n) % 2 != parity
        ir2[others] = (ir[others] + 1) % rv.n_irs
        gain2[others] = gain[others] * np.float32(-0.5) + np.float32(0.125)
        got = per_utt(*run(rv, pcm, first, bf, ir2, gain2), spans_of(xs, first))
        for k in range(n):
            if k % 2 == parity:
                assert got[k] == base[k], ("neighbours changed", name, k)
        assert any(got[k] != base[k] for k in range(n) if k % 2 != parity)


def test_null_gain_is_gain_one_and_the_device_clamps_ir(handles):
    b = K.batch("taps1025")
    rv = handles("taps1025")
    xs = [u.x for u in b.utts if u.x.size][:6]
    pcm, first, bf = K.pack(xs, K.gaps_of(len(xs)))
    ir = np.array([0, 1, 2, 2, 1, 0], np.int32)
    ones = run(rv, pcm, first, bf, ir, np.ones(6, np.float32))
    null = run(rv, pcm, first, bf, ir, None)
    assert ones[0].tobytes() == null[0].tobytes() and ones[1].tobytes() == null[1].tobytes()
    wild = run(rv, pcm, first, bf, np.array([-5, 1, 99, 2 ** 31 - 1, 1, -2 ** 31], np.int32), None)
    assert wild[0].tobytes() == null[0].tobytes() and wild[1].tobytes() == null[1].tobytes()


# ---- 5: beside the partitioned jdsp_fastconv path -----------------------------------------------------------------------
@pytest.mark.parametrize("n_taps_conv", [7169, 7681])
def test_beside_the_partitioned_fastconv_path(eng, n_taps_conv):
    """One stream (fastconv_cases' silence_then_white: its head is silent, which is what the reference's silent head
    assumes) through jdsp_fastconv, n_fft 8192, partitioned, and through the batch entry as one utterance with the same
    taps.  The reverberator takes 7680 taps at most, so the 7681-tap convolver (blocks of 512, 16 partitions) gets the
    7680 taps and a zero behind them: the same convolution.  Both hold the bars against the FP64 value; whether the
    bits are equal is printed, not asserted."""
    n_taps = min(n_taps_conv, 7680)
    h = F._dense(n_taps, 1, 2030 + n_taps_conv, 1200.0)[0]
    h_conv = np.concatenate([h, np.zeros(n_taps_conv - n_taps)])
    s = F.shape_of(8192, n_taps_conv)
    x = F.family("silence_then_white", s)
    assert not x[:s.hist_blocks * s.block].any() and x.size % K.B == 0
    w = reverb_ref.reverb(x, h)
    g, loc = K.bars_of(x, h, 1.0, w)
    u = K.Utt(x, 0, 1.0, "silence_then_white", w, g, loc)
    rv = eng.reverb(h[None])
    pcm, first, bf = K.pack([x])
    r16, r32 = run(rv, pcm, first, bf, [0], None)
    fc = eng.fastconv(h_conv, 8192)
    assert fc.block == s.block
    c16, c32 = fc.process(x, want_precast=True)
    head = s.hist_blocks * s.block
    c16 = np.concatenate([np.zeros(head, np.int16), c16[0]])
    c32 = np.concatenate([np.zeros(head, np.float32), c32[0]])
    assert c32.shape == r32.shape and not r32[:head].any()
    for what, o16, o32 in (("reverb_batch", r16, r32), ("fastconv", c16, c32)):
        gr, lr = K.ratios_of(o32, u)
        own, far = K.int16_rules(o16, o32, u)
        print("\n  %d taps, %-12s: %.4f of the global bar, %.4f of the local bar" % (n_taps_conv, what, gr, lr))
        assert gr <= 1.0 and lr <= 1.0 and own == 0 and far == 0, (what, gr, lr, own, far)
    same = r32.tobytes() == c32.tobytes() and r16.tobytes() == c16.tobytes()
    print("  %d taps: reverb_batch and fastconv bit-equal: %s (%d of %d floats differ)"
          % (n_taps_conv, same, int((r32.view(np.int32) != c32.view(np.int32)).sum()), r32.size))
    fc.close()
    rv.close()


# ---- 6: errors and edges -------------------------------------------------------------------------------------------------
def _err(eng):
    from jeicyboodsp_amd.engine import L
    return L.jdsp_last_error(eng._h).decode()


def test_create_refuses_what_the_header_excludes(eng):
    from jeicyboodsp_amd.engine import L
    EINVAL = -1
    taps = np.zeros(7681)
    for n_irs, n_taps, p in ((1, 0, taps), (1, 7681, taps), (0, 16, taps), (16385, 1, np.zeros(16385)), (1, 16, None)):
        h = C.c_void_p()
        rc = L.jdsp_reverb_create(eng._h, None if p is None else p.ctypes.data_as(C.c_void_p), n_irs, n_taps, C.byref(h))
        assert rc == EINVAL and not h.value and "jdsp_reverb_create" in _err(eng), (n_irs, n_taps)
    rv = eng.reverb(np.ones((2, 7680)))
    assert (rv.n_part, rv.block, rv.n_irs) == (15, 512, 2)
    rv.close()


def test_errors_of_the_batch_entries(eng):
    import torch
    import jeicyboodsp_amd
    from jeicyboodsp_amd.engine import L
    EINVAL = -1
    rv = eng.reverb(K.banks()["taps513"])
    x = K.utterance("white", 5, 90)
    pcm_h, first_h, bf_h = K.pack([x[:2 * K.B], x[2 * K.B:]], [0, 4])
    pcm = torch.from_numpy(pcm_h).cuda()
    first, bf = torch.from_numpy(first_h).cuda(), torch.from_numpy(bf_h).cuda()
    ir = torch.zeros(2, dtype=torch.int32, device="cuda")
    gain = torch.ones(2, dtype=torch.float32, device="cuda")
    o16 = torch.zeros(pcm_h.size + 8, dtype=torch.int16, device="cuda")
    o32 = torch.zeros(pcm_h.size + 8, dtype=torch.float32, device="cuda")
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    eng._use_torch_stream()

    def dev(n_utts=2, n_total=5, p=None, sf=None, bfp=None, irp=None, gp=None, a=None, b=None):
        return L.jdsp_reverb_batch_dev(rv._h, p or vp(pcm), sf or vp(first), bfp or vp(bf), irp or vp(ir), gp or vp(gain),
                                       n_utts, n_total, a or vp(o16), b or vp(o32))

    # before the reservation: a batch with work is refused, empty ones are not
    assert dev() == EINVAL and "jdsp_reverb_batch_reserve" in _err(eng)
    assert dev(n_utts=0, n_total=0) == 0 and dev(n_utts=2, n_total=0) == 0
    for bad in ((-1, 1), (1, -1), (2 ** 31, 1)):
        assert L.jdsp_reverb_batch_reserve(rv._h, *bad) == EINVAL and "jdsp_reverb_batch_reserve" in _err(eng)
    rv.reserve_batch(5, 2)
    assert dev() == 0
    # past the reservation, in blocks and in utterances
    assert dev(n_total=6) == EINVAL and "exceeds" in _err(eng)
    assert dev(n_utts=3) == EINVAL and "exceeds" in _err(eng)
    assert dev(n_utts=-1) == EINVAL and dev(n_total=-1) == EINVAL
    # misaligned pointers
    for kw in (dict(p=vp(pcm, 2)), dict(a=vp(o16, 2)), dict(b=vp(o32, 4)), dict(sf=vp(first, 4)), dict(bfp=vp(bf, 4)),
               dict(irp=vp(ir, 2)), dict(gp=vp(gain, 2))):
        assert dev(**kw) == EINVAL and "aligned" in _err(eng), kw
    # NULL inputs with work to do
    assert L.jdsp_reverb_batch_dev(rv._h, None, vp(first), vp(bf), vp(ir), None, 2, 5, vp(o16), None) == EINVAL
    assert L.jdsp_reverb_batch_dev(rv._h, vp(pcm), vp(first), vp(bf), None, None, 2, 5, vp(o16), None) == EINVAL
    assert "NULL" in _err(eng)
    # both outputs NULL: nothing is done, and it is no error
    assert L.jdsp_reverb_batch_dev(rv._h, vp(pcm), vp(first), vp(bf), vp(ir), None, 2, 5, None, None) == 0
    torch.cuda.synchronize()

    # the host entry: everything jdsp_denoise_batch checks, ir in range, finite gains
    def host(first=first_h, bf=bf_h, ir=(0, 2), gain=(1.0, 1.0), pcm=pcm_h):
        with pytest.raises(jeicyboodsp_amd.JdspError) as e:
            rv.process_batch(pcm, first, bf, ir, gain)
        assert e.value.code == EINVAL and "jdsp_reverb_batch" in str(e.value)
        return str(e.value)
    assert "even" in host(first=first_h + 1)
    assert "[0] must be 0" in host(bf=bf_h + 1)
    assert "must not decrease" in host(bf=np.array([0, 3, 2], np.int64))
    assert "overlap" in host(first=np.array([0, 512], np.int64))
    assert "past n_samples" in host(pcm=pcm_h[:-2])
    assert "outside [0, n_irs)" in host(ir=(0, 3)) and "outside [0, n_irs)" in host(ir=(-1, 0))
    assert "finite" in host(gain=(1.0, np.nan)) and "finite" in host(gain=(np.inf, 1.0))
    rv.process_batch(pcm_h, first_h, bf_h, (0, 2), (1.0, 1.0))
    rv.close()


def test_empty_batches_launch_nothing(eng):
    rv = eng.reverb(K.banks()["tap1"])
    pcm = np.full(2048, 1234, np.int16)
    zero2 = np.zeros(3, np.int64)
    for first, bf, ir in ((np.zeros(0, np.int64), np.zeros(1, np.int64), []), (np.array([0, 512], np.int64), zero2, [0, 1])):
        o16, o32 = run(rv, pcm, first, bf, ir, None)
        outside_is_sentinel(o16, o32, [])
        h16, h32 = rv.process_batch(pcm, first, bf, ir, None, want_f32=True)
        assert not h16.any() and not h32.any() and h16.size == pcm.size
    # an empty pcm too
    assert rv.process_batch(np.zeros(0, np.int16), np.zeros(0, np.int64), np.zeros(1, np.int64), []).size == 0
    # empty utterances among others: the others are what they are alone
    x = K.utterance("white", 3, 91)
    p, f, b = K.pack([x[:0], x, x[:0], x[:0], x[:K.B], x[:0]], [0, 2, 2, 0, 6, 2])
    o16, o32 = run(rv, p, f, b, [0, 1, 2, 0, 1, 2], None)
    outside_is_sentinel(o16, o32, [(2, 2 + x.size), (2 + x.size + 2 + 6, 2 + x.size + 8 + K.B)])
    want = -0.5 * x.astype(np.float64)                         # response 1 of the bank is the single tap -0.5
    assert np.abs(o32[2:2 + x.size] - want).max() <= K.TOL * np.abs(want).max()
    assert np.abs(o32[x.size + 10:x.size + 10 + K.B] - want[:K.B]).max() <= K.TOL * np.abs(want).max()
    rv.close()
