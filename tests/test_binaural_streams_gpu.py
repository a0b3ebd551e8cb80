"""Live binaural rendering (jdsp_binaural_*) on the streams white noise does not reach, against the FP64 reference and
the floored bar of tests/binaural_cases.py (include/jdsp.h, "binaural rendering", guarantee 1):

    |got - want| <= 1e-5 sum_c max(P_c, 0.05 S_c) per output block, exact zeros where that is 0,
    the int16 the cast of the float bit for bit and within one step of the cast of the FP64 value ACROSS THE WRAP,

and the header's earlier unfloored bar 1e-5 sum_c P_c as well wherever plain FP32 (binaural_cases.Restate32) held it with a
factor of 2 to spare.  test_binaural_fp32_ref_cpu.py shows that plain FP32 stays under half of the floored bar on every
case here, so a miss is a defect of the kernel and not FP32's limit.

Families x banks, the wrap, mixes (a source 60 dB under another, g and -g on one span, one span from two directions,
gains -1, 1e-3, 1e3), fades (1000 <-> 0.001, +0.0f -> -0.0f, out of a one-eared direction, on a loud-to-quiet seam),
mixes of 64, 65 and 130 chunks (the fade scan's second trip), the largest bank (n_dirs = 16384) and the device entry's
clamps, the ear whose taps are all zero, and the optional outputs.  Gains in the denormal range are out of scope: the
renderer's FP32 products flush or lose bits there and no bar of this form describes them.

Every test prints the worst error / bar of the device beside plain FP32's (pytest -s); one run is recorded in
profiles/r22_binaural_streams.txt.
"""
import ctypes as C

import numpy as np
import pytest

import binaural_cases as B

pytestmark = pytest.mark.gpu

BLOCK = 512


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def as_np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def render(h, pcm, args, device, i16=True, f32=True):
    """one delivery through the host entry (numpy) or the device entry (torch)"""
    import torch
    if device:
        pcm = torch.from_numpy(np.ascontiguousarray(pcm)).cuda()
    out = h.render(pcm, *args, want_i16=i16, want_f32=f32)
    if device:
        torch.cuda.synchronize()
    if out is None:
        return None
    return tuple(as_np(o) for o in out) if isinstance(out, tuple) else as_np(out)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def state_is(h, ref_state, ids):
    hist, d, g, st = h.streams_state(ids)
    rh, rd, rg, rs = ref_state
    return np.array_equal(hist, rh[ids]) and np.array_equal(d, rd[ids]) and same_bits(g, rg[ids]) and np.array_equal(st, rs[ids])


def run_scene(eng, name, flip=0):
    """every delivery of binaural_cases.scene(name) against its truth, host and device entries in turn; the carried
    state behind the last delivery against the reference's.  -> (handle, [(o16, o32)])"""
    s, truth, fp32 = B.scene(name), B.scene_truth(name), B.scene_fp32(name)
    h = eng.binaural(s.bank)
    h.open_streams(s.n_streams)
    outs = []
    for k, ((pcm, args), (want, bar, floor, state)) in enumerate(zip(s.deliveries, truth)):
        o16, o32 = render(h, pcm, args, device=bool((k + flip) & 1))
        held = fp32[k][1] <= 0.5
        qf, qu = B.ratios(o32, want, floor), B.ratios(o32, want, bar)
        print("binaural scene %-20s delivery %d: device %8.4f of the floored bar, %10.4f of the unfloored | plain FP32 "
              "%8.4f, %10.4f%s" % (name, k, B.worst(qf), B.worst(qu), fp32[k][0], fp32[k][1], "" if held else "  (floored only)"))
        B.check_outputs(o16, o32, want, bar, floor, (name, k), unfloored=held)
        outs.append((o16, o32))
    assert state_is(h, truth[-1][3], np.arange(s.n_streams)), name
    return h, outs


# ---- families x banks, one source per mix ----------------------------------------------------------------------------
@pytest.mark.parametrize("bname", B.FAMILY_BANKS)
def test_families(eng, bname):
    """every family one mix through one bank: ten blocks in one delivery, then the same streams as 1 + 3 + 6 blocks (the
    loud block once inside the chunk, once the carried history); both cuts against the bars, and against each other bit
    for bit (guarantee 2 on these streams)"""
    bank = B.banks()[bname]
    want, bar, floor = B.family_truth(bname)
    fp32 = B.family_fp32(bname)
    k = len(B.FAMILIES)
    flip = B.FAMILY_BANKS.index(bname) & 1
    h = eng.binaural(bank)
    h.open_streams(k)
    got = {}
    for cuts in ([B.N_BLOCKS], [1, 3, 6]):
        h.reset_streams()
        i16, f32 = np.zeros((2, k, B.N_BLOCKS, BLOCK), np.int16), np.zeros((2, k, B.N_BLOCKS, BLOCK), np.float32)
        first = 0
        for n, nb in enumerate(cuts):
            pcm, args = B.family_delivery(bname, first, nb)
            o16, o32 = render(h, pcm, args, device=bool((n + flip + len(cuts)) & 1))
            i16[:, :, first:first + nb] = o16.reshape(2, k, nb, BLOCK)
            f32[:, :, first:first + nb] = o32.reshape(2, k, nb, BLOCK)
            first += nb
        got[len(cuts)] = (i16, f32)
        for i, fam in enumerate(B.FAMILIES):
            sl = slice(BLOCK * B.N_BLOCKS * i, BLOCK * B.N_BLOCKS * (i + 1))
            bl = slice(B.N_BLOCKS * i, B.N_BLOCKS * (i + 1))
            o16, o32 = i16[:, i].reshape(2, -1), f32[:, i].reshape(2, -1)
            held = B.holds_unfloored(bname, fam)
            print("binaural streams %-15s %-19s cuts %-9s: device %8.4f of the floored bar, %12.4f of the unfloored | plain "
                  "FP32 %8.4f, %12.4f%s" % (bname, fam, cuts, B.worst(B.ratios(o32, want[:, sl], floor[bl])),
                                            B.worst(B.ratios(o32, want[:, sl], bar[bl])), fp32[fam][0], fp32[fam][1],
                                            "" if held else "  (floored only)"))
            B.check_outputs(o16, o32, want[:, sl], bar[bl], floor[bl], (bname, fam, cuts), unfloored=held)
            if fam == "silence":
                assert not o32.any() and not o16.any()
            if bname == "one_ear" and i % 3 != 2:              # heard from a direction deaf on ear 1
                assert not o32[1].any() and not o16[1].any() and o32[0].any() == (fam != "silence"), fam
    assert np.array_equal(got[1][0], got[3][0]) and same_bits(got[1][1], got[3][1])
    h.close()


# ---- the wrap, mixes, fades ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wrap17", "wrap_gain8"])
def test_wrap(eng, name):
    """pre-cast values far past +-32,768: the int16 is the low 16 bits of the truncated float, one step at most from
    the cast of the FP64 value modulo 65536"""
    h, outs = run_scene(eng, name, flip=1)
    o16, o32 = outs[0]
    assert np.count_nonzero(np.abs(o32) > 32768.0) >= 500 and np.array_equal(o16, B.cast_i16(o32))
    h.close()


@pytest.mark.parametrize("name", ["loud_plus_quiet", "cancel", "two_dirs", "gains"])
def test_mixes(eng, name):
    h, outs = run_scene(eng, name, flip=len(name) & 1)
    h.close()


@pytest.mark.parametrize("name", ["fade_gain", "seam_fade_noise1", "seam_fade_noise200"])
def test_fades(eng, name):
    h, outs = run_scene(eng, name, flip=len(name) & 1)
    h.close()


def test_plus_zero_to_minus_zero_is_a_faded_block_of_zeros(eng):
    """gain 1 -> +0.0f fades out; +0.0f -> -0.0f differs as a bit pattern: a faded block, zeros, and the stream then
    carries -0.0f; -0.0f -> -0.0f is the plain form, zeros"""
    h, outs = run_scene(eng, "signed_zero")
    truth = B.scene_truth("signed_zero")
    assert np.abs(outs[1][1][:, :64]).max() > 100                 # it was audible before it faded
    for k in (2, 3):
        assert not outs[k][0].any() and not outs[k][1].any()
    assert h.streams_state([0])[2].view(np.uint32)[0] == 0x80000000 and h.streams_state([0])[3][0] == 1
    # the carried bits behind every delivery, on a second pass
    h.reset_streams()
    for k, (pcm, args) in enumerate(B.scene("signed_zero").deliveries):
        render(h, pcm, args, device=True)
        assert state_is(h, truth[k][3], np.array([0])), k
    h.close()


def test_the_zero_ear_is_exact_zeros(eng):
    """mix 0 stays on directions whose ear 1 has no taps while it swaps directions (a faded block), steps a gain (a
    faded block) and rests (plain blocks): ear 1 is exact zeros in both outputs -- the two ears share one staggered
    inverse transform and must not leak into each other -- while ear 0 meets the bar (run_scene).  mix 1 fades out of a
    one-eared direction into a two-eared one and back."""
    h, outs = run_scene(eng, "one_ear", flip=1)
    for k, (o16, o32) in enumerate(outs):
        assert not o32[1, :2 * BLOCK].any() and not o16[1, :2 * BLOCK].any(), k
        assert np.abs(o32[0, :2 * BLOCK]).max() > 100, k
    assert np.abs(outs[1][1][1, 2 * BLOCK:3 * BLOCK]).max() > 10   # mix 1, fading into the two-eared direction
    assert not outs[3][1][1, 2 * BLOCK:].any()                     # mix 1 back on the one-eared direction, plain
    h.close()


# ---- more than 64 chunks in a mix --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,moved", B.MANY)
def test_many_chunks(eng, n, moved):
    """the fade scan walks the chunks 64 at a time: the one chunk that moved is the first or the last of a trip.  The
    faded block meets the reference; in the delivery behind it nothing changes, and its bits are those of a fresh handle
    on which the chunk never moved (the plain form depends on the samples alone)"""
    name = "many%d_moved%d" % (n, moved)
    h, outs = run_scene(eng, name, flip=(n + moved) & 1)
    h.close()
    want = B.scene_truth(name)
    assert np.abs(want[1][0][:, :BLOCK] - want[2][0][:, :BLOCK]).max() > 1     # different blocks, and the fade is audible
    s = B.scene_many(n, moved, never_changed=True)
    h = eng.binaural(s.bank)
    h.open_streams(s.n_streams)
    for k, (pcm, args) in enumerate(s.deliveries):
        o16, o32 = render(h, pcm, args, device=bool(k & 1))
    assert np.array_equal(o16, outs[2][0]) and same_bits(o32, outs[2][1])
    h.close()


# ---- the largest bank; the device entry's clamps -----------------------------------------------------------------
def raw_dev(eng, h, pcm, ids, sf, dirs, gains, cf, bf, o16, o32, plane):
    """jdsp_binaural_render_dev on the caller's own output buffers (torch, on the device); returns the code"""
    import torch
    from jeicyboodsp_amd.engine import L, _vp
    t = [torch.from_numpy(np.ascontiguousarray(a, ty)).cuda() for a, ty in
         ((ids, np.int64), (sf, np.int64), (dirs, np.int32), (gains, np.float32), (cf, np.int64), (bf, np.int64))]
    eng._use_torch_stream()
    rc = L.jdsp_binaural_render_dev(h._h, _vp(pcm), _vp(t[0]), _vp(t[1]), _vp(t[2]), _vp(t[3]), _vp(t[4]), _vp(t[5]),
                                    len(cf) - 1, len(ids), int(bf[-1]), C.c_void_p(o16.data_ptr()) if o16 is not None else None,
                                    C.c_void_p(o32.data_ptr()) if o32 is not None else None, plane)
    torch.cuda.synchronize()
    return rc


def test_directions_up_to_16383_and_the_clamps(eng):
    """bank + d * 1280 at the largest documented n_dirs: directions 0, 1, 8191, 16382 and 16383 against the reference,
    each alone and all in one mix.  Through the DEVICE entry dir = 16384 and dir = -1 give the bits of 16383 and 0, ids
    n_streams and -1 those of n_streams - 1 and 0 (the header's clamp), with nothing written outside the blocks; the
    HOST entry refuses the same values."""
    import torch
    from jeicyboodsp_amd._lib import EINVAL, JdspError
    h, outs = run_scene(eng, "directions")
    assert h.n_dirs == 16384
    o32 = outs[0][1].reshape(2, 6, 2 * BLOCK)
    for a in range(5):
        for b in range(a + 1, 5):
            assert np.abs(o32[:, a] - o32[:, b]).max() > 1.0     # every direction's own taps were heard
    # the clamps: four single-source mixes on one span, one block each
    x = np.array(B.family("white")[:BLOCK])
    pcm = torch.from_numpy(x).cuda()
    plane, pad, n_total = 4 * BLOCK + 64, 32, 4
    lay = (np.zeros(4, np.int64), None, np.float32([1.0] * 4), np.arange(5), np.arange(5))

    def clamped(ids, dirs):
        h.reset_streams()
        o16 = torch.full((pad + 2 * plane + pad,), 0x5a5a, dtype=torch.int16, device="cuda")
        o32 = torch.full((pad + 2 * plane + pad,), -7.25, dtype=torch.float32, device="cuda")
        rc = raw_dev(eng, h, pcm, ids, lay[0], dirs, lay[2], lay[3], lay[4], o16[pad:], o32[pad:], plane)
        assert rc == 0
        a16, a32 = o16.cpu().numpy(), o32.cpu().numpy()
        for a, fill in ((a16, 0x5a5a), (a32, np.float32(-7.25))):
            body = a[pad:pad + 2 * plane].reshape(2, plane)
            assert np.all(a[:pad] == fill) and np.all(a[pad + 2 * plane:] == fill) and np.all(body[:, BLOCK * n_total:] == fill)
        return (a16[pad:pad + 2 * plane].reshape(2, plane)[:, :BLOCK * n_total].reshape(2, 4, BLOCK),
                a32[pad:pad + 2 * plane].reshape(2, plane)[:, :BLOCK * n_total].reshape(2, 4, BLOCK))

    i16, f32 = clamped([0, 1, 2, 3], [16384, -1, 16383, 0])
    assert np.array_equal(i16[:, 0], i16[:, 2]) and same_bits(f32[:, 0], f32[:, 2])
    assert np.array_equal(i16[:, 1], i16[:, 3]) and same_bits(f32[:, 1], f32[:, 3])
    assert np.abs(f32[:, 0] - f32[:, 1]).max() > 1.0
    ref = B.RefFloored(B.big_bank(), 10)
    want, bar, floor = ref.render3(x, [0, 1, 2, 3], lay[0], [16383, 0, 16383, 0], lay[2], lay[3], lay[4])
    B.check_outputs(i16.reshape(2, -1), f32.reshape(2, -1), want, bar, floor, "clamped dirs", unfloored=True)
    hist, d, g, st = h.streams_state([0, 1, 2, 3])
    assert d.tolist() == [16383, 0, 16383, 0] and np.all(st == 1)          # the clamped value is the one carried
    # ids: n_streams -> n_streams - 1 and -1 -> 0 (two mixes, then two idle ones)
    j16, j32 = clamped([10, -1, 4, 5], [16383, 0, 16383, 0])
    assert np.array_equal(j16, i16) and same_bits(j32, f32)
    hist, d, g, st = h.streams_state(np.arange(10))
    assert st.tolist() == [1, 0, 0, 0, 1, 1, 0, 0, 0, 1] and np.array_equal(hist[9], x) and np.array_equal(hist[0], x)
    assert d[9] == 16383 and d[0] == 0
    # the host entry refuses all four, and changes nothing
    before = h.streams_state(np.arange(10))
    for ids, dirs in (([0, 1, 2, 3], [16384, 0, 0, 0]), ([0, 1, 2, 3], [0, -1, 0, 0]), ([10, 1, 2, 3], [0] * 4), ([0, -1, 2, 3], [0] * 4)):
        with pytest.raises(JdspError) as e:
            h.render(x, ids, lay[0], dirs, lay[2], lay[3], lay[4], want_i16=True, want_f32=True)
        assert e.value.code == EINVAL
    for p, q in zip(before, h.streams_state(np.arange(10))):
        assert same_bits(p, q)
    h.close()


# ---- outputs optional ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
def test_each_output_alone_gives_the_same_bits_and_neither_still_advances(eng, device):
    s, truth = B.scene("one_ear"), B.scene_truth("one_ear")
    h = eng.binaural(s.bank)
    h.open_streams(s.n_streams)
    ids = np.arange(s.n_streams)

    def run(i16, f32, upto):
        h.reset_streams()
        return [render(h, pcm, args, device, i16=i16, f32=f32) for pcm, args in s.deliveries[:upto]]

    both = run(True, True, 3)
    only32, only16 = run(False, True, 3), run(True, False, 3)
    for k in range(3):
        assert same_bits(only32[k], both[k][1]) and np.array_equal(only16[k], both[k][0]), k
    # neither: the streams advance all the same (two deliveries, the second one fades), and the next block is right
    assert run(False, False, 2) == [None, None]
    assert state_is(h, truth[1][3], ids)
    pcm, args = s.deliveries[2]
    o16, o32 = render(h, pcm, args, device)
    assert np.array_equal(o16, both[2][0]) and same_bits(o32, both[2][1])
    B.check_outputs(o16, o32, *truth[2][:3], what="behind two deliveries without outputs", unfloored=True)
    h.close()
