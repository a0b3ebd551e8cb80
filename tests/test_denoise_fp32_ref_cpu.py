"""What single precision can and cannot hold in a spectral-subtraction frame, on the CPU (no GPU needed).

The device kernels transform in FP32.  Spectral subtraction's output in a bin far below the noise estimate has the
size of the estimate and the direction of the bin's phase, and FP32 leaves that phase arbitrary once the bin is at the
transform's own rounding: exactly periodic input is where that shows, white noise is where it cannot.  This module
restates the chain (denoise_fp32_ref.py: textbook radix-2, complex64 throughout) on the streams the device test uses,
shows which miss the project's bars and which do not, and checks the kernels' per-frame criterion against both.

Measured here (profiles/r11_denoise_periodic.txt has every stream):
  oracle against numpy's complex128 chain    <= 3.4e-8 absolute (bar 1e-6)
  FP32, non-periodic streams, mode 0         <= 0.61 of the per-block bar, <= 3.3e-6 of the stream's peak
  FP32, every stream, mode 1, one frame per transform   <= 0.05 of the per-block bar
  FP32, exactly periodic streams, mode 0     21 .. 72 LSB before the cast at 1024 points; at 512 points 0.49 .. 5.1
                                             alone and 4.0 .. 137 with two frames per transform
  smallest rho of a frame that misses half its bar      9.9e-6 (threshold 5e-6)
"""
import numpy as np
import pytest

import denoise_fp32_ref as R
from test_denoise_gpu import speechlike, speechlike256

CASES = R.cases()
IDS = [c["name"] for c in CASES]


def _forms(c, fr, nz, mode):
    """(name, y32 [f, n], rho [f]) of every restated form of a stream: alone, and at 512 points in both pairings."""
    out = [("alone", R.chain32(fr, nz, mode), R.criterion(fr, nz))]
    if c["n_fft"] == 512:
        for i, pr in enumerate(R.pairings(fr.shape[0])):
            out.append(("paired%d" % i, R.stream32_paired(fr, nz, mode, pr), R.criterion_paired(fr, nz, pr)))
    return out


def _setup(ci, mode):
    c = CASES[ci]
    t = R.trace(ci, mode)
    return c, t, R.stream_frames(c["pcm"], c["block"]), R.frame_noise(t)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_oracle_is_a_valid_target_and_stays_inside_the_cast(ci):
    """The FP64 reference is well defined on these streams: numpy's complex128 transform and a complex128 radix-2 give
    its pre-cast output to 1e-6 absolute (3.4e-8 seen).  And every stream stays inside +-32767 before the cast, so the
    (short) conversion of out-of-range values plays no part."""
    for mode in (0, 1):
        c, t, fr, nz = _setup(ci, mode)
        o_pre = t[1]
        assert o_pre.size == (c["pcm"].size // c["block"] - 2) * c["block"]
        assert np.abs(o_pre).max() <= 32767.0
        assert t[3].shape[0] >= 2 or c["n_fft"] == 512            # 1024 points: the estimate latched in the lead-in
        for chain in (R.chain64, R.chain64_r2):
            got = R.overlap_add(chain(fr, nz, mode), c["block"])
            err = np.abs(got - o_pre).max()
            print("%s mode %d %s: oracle against it %.2e" % (c["name"], mode, chain.__name__, err))
            assert err <= 1e-6


def _stream_figures(c, t, y32):
    o_pre = t[1]
    err = np.abs(R.overlap_add(y32, c["block"]) - o_pre)
    blk = (err.reshape(-1, c["block"]).max(axis=1) / R.block_bars(o_pre, c["block"])).max()
    return err.max(), err.max() / np.abs(o_pre).max(), blk


@pytest.mark.parametrize("ci", [i for i, c in enumerate(CASES) if not c["periodic"] and "square" not in c["name"]
                                and "dithered" not in c["name"]],
                         ids=lambda i: IDS[i])
def test_fp32_alone_holds_the_non_periodic_streams(ci):
    """White, off-bin, coloured, DC, impulse and vowel streams, one frame per transform: plain FP32 is within the
    per-block bar (0.61 of it at worst: the quietest stretches) and within 3.3e-6 of the stream's peak -- a third of
    the project's bar; the assertion allows half.  Sharing a transform with a loud neighbour is what FP32 does not survive, at any input."""
    c, t, fr, nz = _setup(ci, 0)
    absolute, rel, blk = _stream_figures(c, t, R.chain32(fr, nz, 0))
    print("%s: %.3g absolute, %.2e of the peak, %.2f of the per-block bar" % (c["name"], absolute, rel, blk))
    assert blk <= 0.8 and rel <= 5e-6 and absolute < 0.2


@pytest.mark.parametrize("ci", [i for i, c in enumerate(CASES) if c["periodic"]], ids=lambda i: IDS[i])
def test_fp32_alone_cannot_hold_the_periodic_streams(ci):
    """Exactly periodic stretches (tones on a bin, two of them) in mode 0: plain FP32 is off by more than the +-1 LSB
    the cast is allowed (at 512 points: when two frames share a transform), and by tens to thousands of per-block bars
    in every form.  This is the mechanism, not a device figure."""
    c, t, fr, nz = _setup(ci, 0)
    worst = 0.0
    for name, y32, _ in _forms(c, fr, nz, 0):
        absolute, rel, blk = _stream_figures(c, t, y32)
        print("%s %s: %.3g absolute, %.2e of the peak, %.0f per-block bars" % (c["name"], name, absolute, rel, blk))
        worst = max(worst, absolute)
        assert blk > 20.0 and rel > 1e-5                      # every form misses both relative bars
    assert worst > 2.0                                        # ... and at 512 points the paired forms miss the cast's


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_wiener_is_the_control(ci):
    """Mode 1's gain goes to zero in weak bins: every stream, one frame per transform, within 0.05 of the per-block
    bar in plain FP32."""
    c, t, fr, nz = _setup(ci, 1)
    absolute, rel, blk = _stream_figures(c, t, R.chain32(fr, nz, 1))
    print("%s: %.3g absolute, %.2e of the peak, %.2f of the per-block bar" % (c["name"], absolute, rel, blk))
    assert blk <= 0.1 and rel <= 1e-6


@pytest.mark.parametrize("ci", [i for i, c in enumerate(CASES) if c["n_fft"] == 512], ids=lambda i: IDS[i])
def test_wiener_shares_the_pair_leak(ci):
    """Two 512-point frames in one transform: a quiet frame takes its loud partner's rounding whatever the gain is, so
    mode 1 misses the per-block bar too where a quiet stretch meets a loud one (up to 3.4 bars), and the same figure
    with Wiener's own term, (1 + 2 r) eps per bin, names every frame over half its bar."""
    c, t, fr, nz = _setup(ci, 1)
    y64 = R.chain64(fr, nz, 1)
    bars = R.frame_bars(t[1], c["block"], fr.shape[0])
    for i, pr in enumerate(R.pairings(fr.shape[0])):
        y32 = R.stream32_paired(fr, nz, 1, pr)
        rho = R.criterion_paired(fr, nz, pr, mode=1)
        bad = np.abs(y32 - y64).max(axis=1) > 0.5 * bars
        print("%s paired%d: %.2f per-block bars, %d frames over half their bar, smallest rho %.3g"
              % (c["name"], i, _stream_figures(c, t, y32)[2], bad.sum(), rho[bad].min() if bad.any() else 0.0))
        assert not (bad & ~(rho > R.RHO)).any()


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_criterion_flags_every_frame_fp32_cannot_hold(ci):
    """Every frame whose plain-FP32 error exceeds half its bar, in every restated form, has rho above the threshold
    with a margin of 1.9: the smallest such rho over the list is 9.9e-6."""
    c, t, fr, nz = _setup(ci, 0)
    y64 = R.chain64(fr, nz, 0)
    bars = R.frame_bars(t[1], c["block"], fr.shape[0])
    for name, y32, rho in _forms(c, fr, nz, 0):
        bad = np.abs(y32 - y64).max(axis=1) > 0.5 * bars
        if bad.any():
            print("%s %s: %d frames over half their bar, smallest rho %.3g" % (c["name"], name, bad.sum(), rho[bad].min()))
            assert rho[bad].min() > 1.9 * R.RHO
        if c["periodic"]:
            assert bad.sum() >= 7


@pytest.mark.parametrize("w", R.WHITE_STREAMS, ids=R.white_id)
def test_criterion_on_the_white_streams_of_the_other_tests(w):
    """Every speechlike / speechlike256 stream test_denoise_gpu.py names: the number of frames over the threshold, per
    restated form, is exactly what denoise_fp32_ref.WHITE_STREAMS records -- 0 on every stream of up to 333 blocks at
    1024 points and up to 8 at 512; 12 of 9,499 on the pause-heavy one; at 512 points the quiet frames that share a
    transform with a loud one.  (That NO white frame is ever listed cannot hold together with a bar taken from a
    block's own neighbourhood: test_white_streams_are_not_exempt.)"""
    block, seed, n_blocks, pattern, counts, bound = w
    if n_blocks < 2:
        assert counts == (0,) * len(counts) and bound == 0      # no frame at all
        return
    pcm = R.white_pcm(w)
    t = R._oracle().denoise_trace(0, pcm, block=block)
    fr, nz = R.stream_frames(pcm, block), R.frame_noise(t)
    rho = [R.criterion(fr, nz)]
    if block == 256:
        rho += [R.criterion_paired(fr, nz, pr) for pr in R.pairings(fr.shape[0])]
    got = tuple(int((r > R.RHO).sum()) for r in rho)
    half = max(int((r > R.RHO / 2).sum()) for r in rho)
    print("over the threshold %s, over half of it %d, largest rho %.3g" % (got, half, max(r.max() for r in rho)))
    assert got == counts and half == bound


@pytest.mark.parametrize("block", [512, 256])
def test_white_streams_are_not_exempt(block):
    """The condition that NO frame of any white stream is ever flagged cannot hold together with a bar taken from a
    block's own neighbourhood: a white frame has a bin a thousand times under the estimate once in a few thousand
    frames, and a quiet 512-point frame that shares a transform with a loud one takes its partner's rounding.  On the
    pause-heavy stream of test_denoise_gpu.py (9,500 blocks) plain FP32 misses half the bar in a few frames, and the
    criterion names those and not many more: 12 of 9,499 frames at 1024 points; at 512 points 64 alone and 360 paired
    (the quiet frames at the 1,400 loud boundaries).  What it must not do is pass a frame FP32 cannot hold."""
    gen = speechlike if block == 512 else speechlike256
    pcm = gen(77, 9500, pattern=[40, 3, 25, 1, 90, 2, 11, 5])
    t = R._oracle().denoise_trace(0, pcm, block=block)
    fr, nz = R.stream_frames(pcm, block), R.frame_noise(t)
    y64 = R.chain64(fr, nz, 0)
    bars = R.frame_bars(t[1], block, fr.shape[0])
    forms = [(R.chain32(fr, nz, 0), R.criterion(fr, nz))]
    if block == 256:
        forms += [(R.stream32_paired(fr, nz, 0, pr), R.criterion_paired(fr, nz, pr)) for pr in R.pairings(fr.shape[0])]
    for y32, rho in forms:
        err = np.abs(y32 - y64).max(axis=1)
        bad = (err > 0.5 * bars) & (bars > 1e-200)
        flagged = rho > R.RHO
        print("block %d: %d frames over half their bar, %d flagged of %d" % (block, bad.sum(), flagged.sum(), rho.size))
        assert not (bad & ~flagged).any()
        assert flagged.mean() < (0.002 if block == 512 else 0.05)


def test_real_bins_and_silence():
    """Bins 0 and n/2 of a real frame cannot turn: a DC-free frame's bin 0 is counted only at the rounding itself.  An
    all-zero frame is exact in FP32 (rho 0); a zero bin under a non-zero estimate is never passed (rho inf)."""
    n = 1024
    noise = np.full((1, n), 900.0)
    assert R.criterion(np.zeros((1, n), np.int16), noise)[0] == 0.0
    rng = np.random.default_rng(1)
    x = R.white(rng, n, 3000.0)[None]
    X = R.spectrum32(x)
    e = R.frame_energy(x)
    base = R.rho_of(X, noise, e)[0]
    Xz = X.copy()
    Xz[0, 7] = 0
    assert np.isinf(R.rho_of(Xz, noise, e)[0])
    Xd = X.copy()
    Xd[0, 0] = 1.0                                            # a real bin 900 times under its estimate, far above 16 eps
    assert R.rho_of(Xd, noise, e)[0] <= base * 1.001
    Xd[0, 0] = np.float32(1e-3)                               # ... and one at the rounding itself
    assert R.rho_of(Xd, noise, e)[0] > 100 * base
