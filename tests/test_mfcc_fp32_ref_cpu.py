"""The coloured-frame case list does what the device test needs of it (CPU only; mfcc_fp32_ref.py).

1. Every frame of the list, ALONE in a single-precision transform, is within 4e-6 of the FP64 oracle: 1e-5 on the
   device is then a fair bar for an FP32 chain on these inputs (low-pass noise with a -80 dB stopband, for one, is
   not: FP32 itself runs out there at 1e-5, so the list stops at -60 dB).
2. At least a quarter of the quiet coloured frames 20 dB or more under their partner miss 1e-5 when the two frames
   share one transform and nothing separates them: the list really holds the frames test_mfcc_coloured_gpu.py is
   about.
3. White against white at equal level, packed, equals the single-frame chain to 1e-6 (the restatement's own sanity).
"""
import numpy as np
import pytest

import mfcc_fp32_ref as R

ALONE_TOL = 4e-6
BAR = 1e-5

CONFIGS = {
    # name: (oracle cfg overrides, n_bins, frame length, sample rate)
    "pair_400_512fft_40mel": (dict(win_len=400, hop=160, n_fft=512, n_chan=40, n_cep=13, half_rate=8000.0), 256, 400, 16000.0),
    "one_512_512fft_64mel": (dict(win_len=512, hop=256, n_fft=512, n_chan=64, n_cep=13, half_rate=8000.0), 256, 512, 16000.0),
    "native_1024": (dict(), 512, 1024, 44100.0),
}


def _cfg(oracle, name):
    kw, n_bins, n, fs = CONFIGS[name]
    return oracle.mfcc_cfg(n_bins=n_bins, **kw), n, fs


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_every_frame_alone_is_within_4e6_of_the_oracle(oracle, name):
    """The three configurations the device test runs the list through, each at its own frame length and rate."""
    cfg, n, fs = _cfg(oracle, name)
    worst = {}
    for c in R.cases(n, fs):
        for who, fr in (("quiet", c["a"] if c["slot"] == 0 else c["b"]), ("loud", c["b"] if c["slot"] == 0 else c["a"])):
            key = (c["kind"], c["db"]) if who == "quiet" else ("partner " + c["partner"], 0)
            worst[key] = max(worst.get(key, 0.0), R.rel(R.single(cfg, fr), R.want(cfg, fr)))
    for key in sorted(worst):
        print("%-22s alone %-16s %2d dB: %.2e" % (name, key[0], key[1], worst[key]))
    bad = {k: v for k, v in worst.items() if not v < ALONE_TOL}
    assert not bad, bad


def test_a_quarter_of_the_quiet_coloured_frames_need_separating(oracle):
    cfg, n, fs = _cfg(oracle, "pair_400_512fft_40mel")
    errs = []
    for c in R.cases(n, fs):
        if c["kind"] == "white" or c["db"] < 20:
            continue
        pa, pb = R.paired(cfg, c["a"], c["b"])
        quiet, got = (c["a"], pa) if c["slot"] == 0 else (c["b"], pb)
        errs.append(R.rel(got, R.want(cfg, quiet)))
    errs = np.array(errs)
    assert errs.size == 5 * 3 * 2 * 2 * R.N_SEEDS
    share = float((errs > BAR).mean())
    print("quiet coloured frames >= 20 dB under their partner: %d, packed error above 1e-5: %.0f %%, worst %.2e"
          % (errs.size, 100 * share, errs.max()))
    assert share >= 0.25, share


def test_packed_white_against_white_equals_the_single_chain(oracle):
    cfg, n, fs = _cfg(oracle, "pair_400_512fft_40mel")
    for seed in range(4):
        rng = np.random.default_rng([77, seed])
        a, b = R.white(rng, n, 3000.0), R.white(rng, n, 3000.0)
        pa, pb = R.paired(cfg, a, b)
        for fr, got in ((a, pa), (b, pb)):
            alone = R.single(cfg, fr)
            assert np.abs(got - alone).max() / np.abs(alone).max() < 1e-6
            assert R.rel(got, R.want(cfg, fr)) < ALONE_TOL


def test_a_plain_fp32_transform_rounds_four_times_coarser_than_numpys():
    """The constant behind the pair kernel's criterion: rms error per bin over the rms of the output, 512 points.
    numpy's complex64 transform: 2.5e-8.  The kernels' three radix-8 passes, restated in numpy float32: 1.0e-7, which
    the criterion takes as 2^-23 = 1.19e-7."""
    rng = np.random.default_rng(512)
    got = {"numpy": [], "radix8": []}
    for _ in range(16):
        z = (rng.normal(size=512) + 1j * rng.normal(size=512)).astype(np.complex64)
        exact = np.fft.fft(z.astype(np.complex128))
        for name, f in (("numpy", R.fft32), ("radix8", R.fft32_radix8)):
            got[name].append(np.sqrt(np.mean(np.abs(f(z) - exact) ** 2) / np.mean(np.abs(exact) ** 2)))
    numpy_err, radix8_err = np.mean(got["numpy"]), np.mean(got["radix8"])
    print("rms rounding per bin / rms output: numpy complex64 %.2e, three FP32 radix-8 passes %.2e" % (numpy_err, radix8_err))
    assert numpy_err < 4e-8
    assert 0.7e-7 < radix8_err < 2.0 ** -23


def test_the_transform_stays_in_single_precision():
    z = (np.arange(512) % 7).astype(np.complex64)
    assert R.fft32(z).dtype == np.complex64
    assert len(R.cases()) == 480 and R.frames_of(R.cases()).shape == (960, 400)
    assert R.frames_of(R.cases()).dtype == np.int16
