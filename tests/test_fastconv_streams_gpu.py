"""The overlap-save convolver on the streams white noise does not reach, on each of its four kernels
(fastconv_kernels.hip), against the CPU oracle:

  a. every input family of fastconv_cases on every kernel: the global bar (test_fastconv_gpu.py's check()), the local
     bar (a quiet stretch judged on its own scale), and the int16 rules on EVERY sample -- out is the cast of the float
     the kernel stored, bit for bit, and at most one step from the oracle's int16 modulo 65536
  b. the wrap: filters that take the pre-cast values far past +-32768 (the cast is defined there: truncate to int32,
     keep the low 16 bits), same rules, nothing excluded
  c. alignment: the entry promises natural alignment (2 bytes for pcm and out, 4 for precast; include/jdsp.h); every
     pointer is swept over the offsets at which a kernel's load or store path changes, inside sentinel-guarded
     allocations, and must give the aligned call's bits and leave the sentinels alone
  d. call cuts: one call, a cut at every block, one block per call and the host entry give the same bits

The kernels and the shapes that reach them (launch_fastconv / jdsp_fastconv_create):
  pairs      n_fft 1024, 256 taps, one or two filters            fastconv1024_pairs_kernel
  generic    n_fft 1024, any other shape                          fastconv1024_kernel
  part       n_fft 8192, block a multiple of 512                  conv_stage_kernel + fastconv_upols4_kernel
  k8192      n_fft 8192, any other block, or the switch off       fastconv8192_kernel
Every test runs under test_fastconv_gpu.py's conv_impl fixture (JDSP_FASTCONV_PARTITIONED, read when a handle is
created), so the 8192-point shapes whose block is a multiple of 512 run on both kernels; a shape that has one kernel
only runs on it under either setting.  kernel_of() names the kernel a case reached; it is printed with every figure.

Measured figures: profiles/r20_fastconv_streams.txt.
"""
import ctypes as C
import os

import numpy as np
import pytest

import fastconv_cases as K
from graph_replay_cases import FILL
from test_fastconv_gpu import conv_impl  # noqa: F401  (autouse: every test here runs under both settings of the switch)

pytestmark = pytest.mark.gpu

FAMILY_FILTERS = ("hrir1", "hrir2", "highpass", "taps200x3", "one_tap", "taps1024", "rir", "dense7169", "taps7681x2",
                  "taps7000")
WRAP_FILTERS = K.WRAP_FILTERS
FOUR = ("hrir2", "taps200x3", "dense7169")     # pairs, generic, and under the switch partitioned and 8192-point
MARGIN = 1 << 16                               # sentinel bytes on both sides of every region


def kernel_of(fname):
    """the kernel a handle of this filter, created now, launches (launch_fastconv / jdsp_fastconv_create)"""
    n_fft, h = K.filters()[fname]
    s = K.shape_for(fname)
    if n_fft == 1024:
        return "pairs" if h.shape[1] == 256 and h.shape[0] <= 2 else "generic"
    return "part" if s.block % 512 == 0 and os.environ.get("JDSP_FASTCONV_PARTITIONED", "1")[:1] != "0" else "k8192"


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def handles(eng):
    """(filter, kernel) -> convolver handle, made once, inside a test and so under that test's conv_impl setting"""
    made = {}

    def get(fname):
        key = (fname, kernel_of(fname))
        if key not in made:
            n_fft, h = K.filters()[fname]
            fc = eng.fastconv(h, n_fft)
            s = K.shape_for(fname)
            assert fc.block == s.block and fc.hist_blocks == s.hist_blocks
            made[key] = fc
        fc = made[key]
        fc.reset()
        return fc, "%s-%s" % key[::-1]

    yield get
    for fc in made.values():
        fc.close()


def judge(what, out, pre, oracle, fname, fam, **kw):
    """both bars and both int16 rules for every filter row; the figures are printed before anything is asserted"""
    n_filters = K.filters()[fname][1].shape[0]
    rows = []
    for f in range(n_filters):
        t = K.truth(oracle, fname, fam, f, **kw)
        assert out[f].shape == t.out.shape and pre[f].shape == t.pre.shape
        rows.append(K.ratios_of(pre[f], t) + K.int16_rules(out[f], pre[f], t))
    g, loc = max(r[0] for r in rows), max(r[1] for r in rows)
    own, far = sum(r[2] for r in rows), sum(r[3] for r in rows)
    print("FRACTIONS %-22s %-19s global %.4f local %.4f cast-mismatch %d off-by-more-than-1 %d"
          % (what, fam, g, loc, own, far))
    assert g <= 1.0, (what, fam, "global bar", g)
    assert loc <= 1.0, (what, fam, "local bar", loc)
    assert own == 0, (what, fam, "out is not the cast of the stored float", own)
    assert far == 0, (what, fam, "int16 more than one step from the oracle's, modulo 65536", far)


# ---- a. every family on every kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", K.FAMILIES)
@pytest.mark.parametrize("fname", FAMILY_FILTERS)
def test_family_on_kernel(handles, oracle, fname, fam):
    fc, what = handles(fname)
    x = K.stream(fname, fam)
    out, pre = fc.process(x, want_precast=True)
    judge(what, out, pre, oracle, fname, fam)
    if fam == "silence":
        assert not out.any() and not pre.any()
    if fam == "silence_then_white":
        s = K.shape_for(fname)
        assert not x[:(s.hist_blocks + 2) * s.block].any() and x.any() and out.any()


@pytest.mark.parametrize("fname", K.LONG_8192)
def test_quiet_blocks_after_a_loud_history_8192(handles, oracle, fname):
    """history + 8 blocks of an 8192-point shape hold no quiet output whose whole segment FOLLOWS the loud stretch; these
    streams do: the loud sixth starts a quarter in, and the local bar judges the quiet blocks behind it on their own
    scale (a leak from an earlier segment, a wrong discard boundary)"""
    fc, what = handles(fname)
    nb = K.LONG_8192[fname]
    s = K.shape_for(fname, nb)
    lo, hi = K.loud_span(s)
    assert hi < s.n_blocks * s.block - s.n_fft - 2 * s.block and lo >= (s.hist_blocks + 2) * s.block
    x = K.stream(fname, "loud_then_quiet", nb)
    out, pre = fc.process(x, want_precast=True)
    t = K.truth(oracle, fname, "loud_then_quiet", 0, n_blocks=nb)
    after = t.local_bar[hi + s.n_fft - s.hist_blocks * s.block:]
    assert after.size >= s.block and t.global_bar / after.min() >= 100.0
    judge(what + "-long", out, pre, oracle, fname, "loud_then_quiet", n_blocks=nb)


# ---- b. the wrap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["full_square", "sine_fs_on", "sine_fs_off", "white"])
@pytest.mark.parametrize("fname", WRAP_FILTERS)
def test_wrap_like_the_oracle_cast(handles, oracle, fname, fam):
    fc, what = handles(fname)
    kw = dict(sigma=9000.0) if fam == "white" else {}
    x = K.stream(fname, fam, **kw)
    out, pre = fc.process(x, want_precast=True)
    past = int(np.count_nonzero(np.abs(pre) > 32768.0))
    print("WRAP %-22s %-12s: %d of %d device pre-cast samples past +-32768, peak %.0f" % (what, fam, past, pre.size, np.abs(pre).max()))
    judge(what, out, pre, oracle, fname, fam, **kw)
    assert past >= 1000


# ---- c. alignment ------------------------------------------------------------------------------------------------------
class Guarded:
    """One device allocation: MARGIN sentinel bytes, the region, MARGIN + 64 sentinel bytes.  Every address a test forms
    from it (the region's start plus a few elements) lies inside it."""

    def __init__(self, nbytes, content=None):
        import torch
        self.nbytes = int(nbytes)
        self.t = torch.full((MARGIN + self.nbytes + MARGIN + 64,), FILL, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 256 == 0
        self.content = None
        if content is not None:
            self.content = np.ascontiguousarray(content).view(np.uint8).reshape(-1).copy()

    def place(self, off_bytes):
        """sentinels everywhere, the content (if any) at off_bytes past the region's start; -> the device address there"""
        import torch
        assert 0 <= off_bytes <= 64
        self.t.fill_(FILL)
        if self.content is not None:
            lo = MARGIN + off_bytes
            self.t[lo:lo + self.content.size] = torch.from_numpy(self.content).cuda()
        return self.t.data_ptr() + MARGIN + off_bytes

    def read(self, off_bytes, nbytes):
        """(the nbytes at off_bytes, whether every other byte of the allocation still holds the sentinel)"""
        a = self.t.cpu().numpy()
        lo = MARGIN + off_bytes
        rest = np.concatenate([a[:lo], a[lo + nbytes:]])
        return a[lo:lo + nbytes].copy(), bool(np.all(rest == FILL))


def _aligned_sweep():
    """(pcm offset in samples, out offset in samples, precast offset in floats or None for a NULL pointer): one offset
    at a time, then four cases with every offset odd"""
    cases = [(p, 0, 0) for p in range(8)]
    cases += [(0, o, 0) for o in range(1, 4)]
    cases += [(0, 0, q) for q in range(1, 4)] + [(0, 0, None)]
    cases += [(1, 1, 1), (3, 3, 3), (5, 1, 3), (7, 3, 1)]
    return cases


def interior_blocks(s, lo, hi):
    """output blocks of the call over input blocks [lo, hi) whose whole segment lies inside the call's buffer and past
    the stream's silent head: the blocks on which the kernels take their address-dependent load paths"""
    first = max(lo, s.hist_blocks)
    return [b for b in range(first, hi)
            if (b + 1) * s.block - s.n_fft >= max(lo, s.hist_blocks) * s.block]


@pytest.mark.parametrize("fname", FOUR)
def test_natural_alignment_is_enough(eng, handles, fname):
    import torch
    from jeicyboodsp_amd.engine import L
    fc, kernel = handles(fname)
    # Two calls, so that the history the first leaves is read by a misaligned second one too (and, for the odd block
    # lengths, the second call's pointer has another alignment than the first's).  Both are long enough to hold
    # blocks whose whole segment lies inside the call's buffer past the silent head: only there do fastconv8192_kernel
    # (its 4-byte test), fastconv1024_kernel and the pairs kernel leave conv_sample() for their plain loads, so only
    # there can an odd pcm offset take another path than the aligned call.
    H = fc.hist_blocks
    s = K.shape_for(fname, 3 * H + 4)
    B, nf = s.block, fc.n_filters
    x = K.family("white", s)
    calls = [(0, 2 * H + 2), (2 * H + 2, s.n_blocks)]
    n_outs = [H + 2, H + 2]
    for lo, hi in calls:
        assert len(interior_blocks(s, lo, hi)) >= 2, (kernel, lo, hi)
    pcm = Guarded(x.nbytes, x)
    outs = [Guarded(nf * n * B * 2) for n in n_outs]
    pres = [Guarded(nf * n * B * 4) for n in n_outs]

    def run(po, oo, qo):
        fc.reset()
        base = pcm.place(2 * po)
        got = []
        for (lo, hi), n, ob, pb in zip(calls, n_outs, outs, pres):
            o_ptr = ob.place(2 * oo)
            p_ptr = pb.place(4 * (qo or 0))
            n_out = C.c_long(-1)
            eng._use_torch_stream()
            eng._ck(L.jdsp_fastconv_process_dev(fc._h, C.c_void_p(base + 2 * lo * B), hi - lo, C.c_void_p(o_ptr),
                                                C.c_void_p(p_ptr) if qo is not None else None, C.byref(n_out)))
            torch.cuda.synchronize()
            assert n_out.value == n
            o, o_clean = ob.read(2 * oo, nf * n * B * 2)
            p, p_clean = pb.read(4 * (qo or 0), nf * n * B * 4 if qo is not None else 0)
            assert o_clean, (kernel, po, oo, qo, "int16 output written outside its planes")
            assert p_clean, (kernel, po, oo, qo, "pre-cast output written outside its planes (or through a NULL request)")
            got.append((o.tobytes(), p.tobytes()))
        data, clean = pcm.read(2 * po, x.nbytes)
        assert clean and data.tobytes() == x.tobytes(), (kernel, "the input was written")
        return got

    want = run(0, 0, 0)
    assert all(np.frombuffer(o, np.int16).any() for o, _ in want)
    for po, oo, qo in _aligned_sweep()[1:]:
        got = run(po, oo, qo)
        for (go, gp), (wo, wp) in zip(got, want):
            assert go == wo, (kernel, po, oo, qo, "int16 differs from the aligned call")
            assert qo is None or gp == wp, (kernel, po, oo, qo, "pre-cast differs from the aligned call")
    print("ALIGN %-22s %d placements of pcm / out / precast, two calls each: the aligned call's bits, sentinels intact"
          % (kernel, len(_aligned_sweep()) - 1))


# ---- d. call cuts ------------------------------------------------------------------------------------------------------
def _feed(fc, x, B, cuts, dev):
    """process() over consecutive slices of `cuts` blocks -> (int16 [F, n], pre-cast bits uint32 [F, n])"""
    import torch
    outs, pres, pos = [], [], 0
    for n in cuts:
        piece = x[pos * B:(pos + n) * B]
        o, p = fc.process(torch.from_numpy(piece.copy()).cuda() if dev else piece, want_precast=True)
        if dev:
            torch.cuda.synchronize()
            o, p = o.cpu().numpy(), p.cpu().numpy()
        outs.append(o); pres.append(p); pos += n
    assert pos * B == x.size
    return np.concatenate(outs, axis=1), np.ascontiguousarray(np.concatenate(pres, axis=1)).view(np.uint32)


# (filter, blocks past the history).  Ten everywhere; the partitioned kernel's oldest frame starts 512 samples before
# the oldest sample the taps reach (512 * 15 - 7168 at 7169 taps, 512 * 16 - 7680 at 7681), and a cut shows there only
# once that stretch lies past the stream's silent head: from cut 15 of 17 at block 1024, and from cut 31 at block 512
# -- hence the long case.
CUT_CASES = [(f, 10) for f in FOUR + ("one_tap", "taps7681x2", "taps7000")] + [("taps7681x2", 21)]


@pytest.mark.parametrize("fam", ["loud_then_quiet", "full_square"])
@pytest.mark.parametrize("fname,past", CUT_CASES)
def test_call_cuts_bit_identical(handles, oracle, fname, past, fam):
    fc, kernel = handles(fname)
    s = K.shape_for(fname, fc.hist_blocks + past)
    x = K.family(fam, s)
    nb, B = s.n_blocks, s.block
    one, one_pre = _feed(fc, x, B, [nb], True)
    assert one.shape == (fc.n_filters, past * B) and one.any()
    t = K.truth_of(oracle, x, K.filters()[fname][1][0], s.n_fft)          # the one-call stream is the right one
    g, loc = K.ratios_of(one_pre[0].view(np.float32), t)
    print("CUTS %-22s %-16s one call: global %.4f local %.4f" % (kernel, fam, g, loc))
    assert g <= 1.0 and loc <= 1.0
    plans = [("cut at %d" % c, [c, nb - c]) for c in range(1, nb)] + [("one block per call", [1] * nb)]
    for what, cuts in plans:
        fc.reset()
        got, got_pre = _feed(fc, x, B, cuts, True)
        assert np.array_equal(got, one), (kernel, fam, what, "int16")
        assert np.array_equal(got_pre, one_pre), (kernel, fam, what, "pre-cast bits")
    for what, cuts in (("host entry", [nb]), ("host entry, three calls", [1, nb // 2, nb - 1 - nb // 2])):
        fc.reset()
        got, got_pre = _feed(fc, x, B, cuts, False)
        assert np.array_equal(got, one), (kernel, fam, what, "int16")
        assert np.array_equal(got_pre, one_pre), (kernel, fam, what, "pre-cast bits")
