"""GPU parity: MFCC vectors of COLOURED frames, whatever frame shares their transform.

The 512-FFT configurations put frames 2j and 2j+1 of a call into one complex FP32 transform (mfcc512_pair_kernel).
The two spectra come apart exactly only in exact arithmetic: the partner's rounding lands in this frame's bins, and
ln() of a mel channel divides it by the channel's own sum.  White noise -- what every other MFCC test feeds -- is the
one input that cannot show this; a quiet voiced frame next to a loud one is the input that does.  The kernel has to
notice such pairs itself and compute them apart (MFCC; measured: profiles/r10_mfcc_pair_leak.txt).

The case list, the input families and the FP32 restatement are in mfcc_fp32_ref.py; test_mfcc_fp32_ref_cpu.py shows on
the CPU that every frame of the list, alone in an FP32 chain, is within 4e-6 of the oracle, and that packed without
separation more than a quarter of the quiet coloured ones miss 1e-5.

A case is one frame; a call is a buffer of concatenated frames with frame_start = n i, so that frames 2j and 2j+1 are
exactly the intended pair, and pre-emphasis restarts at x[0] = 0 in every frame: frames are independent.
"""
import numpy as np
import pytest

import mfcc_fp32_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
KW4 = dict(win_len=400, hop=160, n_fft=512, n_chan=40, n_cep=13, half_rate=8000.0)      # BASELINE config 4


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def _check(got, want):
    peak = np.abs(want).max(axis=1, keepdims=True)
    assert (np.abs(got - want) / peak).max() < TOL


def _errors(got, want):
    return (np.abs(got - want) / np.abs(want).max(axis=1, keepdims=True)).max(axis=1)


def _call(m, frames):
    """One call over the frames [k, n], each framed on its own."""
    n = frames.shape[1]
    return m.frames(np.ascontiguousarray(frames).reshape(-1), frame_start=n * np.arange(frames.shape[0], dtype=np.int64))


_want_cache = {}


def _want(oracle, key, ocfg, frames):
    """The oracle's vectors of the frames, computed once per configuration and left unchanged."""
    if key not in _want_cache:
        w = np.stack([oracle.mfcc_frames(ocfg, fr, 1)[0] for fr in frames])
        w.setflags(write=False)
        _want_cache[key] = w
    return _want_cache[key]


def _report(tag, err, case_list, first=0):
    """Worst error of the quiet frames per kind and level, and of the loud partners (err[first + 2 j + slot])."""
    worst = {}
    for j, c in enumerate(case_list):
        q, l = err[first + 2 * j + c["slot"]], err[first + 2 * j + 1 - c["slot"]]
        worst[(c["kind"], c["db"])] = max(worst.get((c["kind"], c["db"]), 0.0), q)
        worst[("partner", 0)] = max(worst.get(("partner", 0), 0.0), l)
    for kind in R.KINDS:
        print("%-24s %-9s" % (tag, kind) + "".join("  %2d dB %.2e" % (db, worst[(kind, db)]) for db in R.LEVELS_DB))
    print("%-24s loud partners %.2e, all frames %.2e, frames above 1e-5: %d of %d"
          % (tag, worst[("partner", 0)], err.max(), int((err >= TOL).sum()), err.size))


def _shifted(frames, n):
    """The list behind one extra white frame: every frame meets its other neighbour, the last one is alone."""
    extra = R.white(np.random.default_rng(4242), n, 3000.0)
    return np.concatenate([extra[None], frames])


@pytest.mark.parametrize("n_chan", [40, 20])
def test_coloured_frame_within_tolerance_whatever_its_partner(eng, oracle, n_chan):
    """All 480 pairs in one call, every vector within 1e-5 of the oracle; then the same list one frame later.  n_chan = 20
    is the wider-piece instantiation of the pair kernel (pieces longer than 8 bins)."""
    kw = dict(KW4, n_chan=n_chan)
    ocfg = oracle.mfcc_cfg(n_bins=256, **kw)
    case_list = R.cases(400, 16000.0)
    frames = R.frames_of(case_list)
    shifted = _shifted(frames, 400)
    want = _want(oracle, ("pair", n_chan), ocfg, shifted)
    m = eng.mfcc(**kw)
    got = _call(m, frames)
    got_shifted = _call(m, shifted)
    m.close()
    assert got.shape == (960, 13) and got_shifted.shape == (961, 13)
    _report("pair %d mel" % n_chan, _errors(got, want[1:]), case_list)
    _report("pair %d mel, shifted" % n_chan, _errors(got_shifted, want), case_list, first=1)
    _check(got, want[1:])
    _check(got_shifted, want)


@pytest.mark.parametrize("name,kw,n_bins,n,fs", [
    # one frame per wave (mfcc_kernel: 65 channel indices do not fit one piece per lane)
    ("one frame per wave", dict(win_len=512, hop=256, n_fft=512, n_chan=64, n_cep=13, half_rate=8000.0), 256, 512, 16000.0),
    # the reference-native configuration (mfcc_x2_kernel: two frames per wave, a transform each)
    ("native 1024", dict(), 512, 1024, 44100.0),
])
def test_coloured_frames_on_the_kernels_that_do_not_pair(eng, oracle, name, kw, n_bins, n, fs):
    """The controls: the same families at these configurations' frame length and rate, through the two kernels that
    give every frame a transform of its own, at the same 1e-5.  Nothing leaks between frames here, but a frame's OWN
    transform rounds too: with every frame left in FP32 these kernels miss the bar on high-pass noise and tones, at
    every level (1.78e-5 and 4.08e-5: profiles/r10_mfcc_pair_leak.txt), because a plain FP32 transform rounds four
    times coarser than the numpy one the CPU test runs.  They judge each frame by the pair kernel's bound
    (mfcc_leak_one) and hand the ones that fail to the same FP64 pass."""
    ocfg = oracle.mfcc_cfg(n_bins=n_bins, **kw)
    case_list = R.cases(n, fs)
    frames = R.frames_of(case_list)
    want = _want(oracle, name, ocfg, frames)
    m = eng.mfcc(**kw)
    got = _call(m, frames)
    m.close()
    _report(name, _errors(got, want), case_list)
    _check(got, want)


def test_pair_result_equals_alone_result_when_separated(eng, oracle):
    """Pairs the kernel has to separate (a coloured frame 35 dB under its partner): each of their frames again, alone, as
    a one-frame call.  A one-frame call runs mfcc512_pair_kernel with the frame in both slots of its transform, and
    a frame without a partner always goes onto the list of pairs to compute apart; the separated pair is on that list
    too.  Both routes end in mfcc_redo_f64_kernel, one frame at a time, so the results are equal bit for bit -- and they
    are not if the criterion leaves one of these pairs packed."""
    case_list = [c for c in R.cases(400, 16000.0)
                 if c["db"] == 35 and c["kind"] != "white" and c["partner"] == "white" and c["seed"] == 0]
    assert len(case_list) == 10                                                 # five kinds, quiet frame in either slot
    frames = R.frames_of(case_list)
    m = eng.mfcc(**KW4)
    together = _call(m, frames)
    alone = np.concatenate([_call(m, fr[None]) for fr in frames])
    m.close()
    diff = _errors(alone, together)
    for j, c in enumerate(case_list):
        print("alone vs paired  %-9s slot %d: quiet %.2e loud %.2e" % (c["kind"], c["slot"], diff[2 * j + c["slot"]],
                                                                       diff[2 * j + 1 - c["slot"]]))
    assert np.array_equal(alone.view(np.int64), together.view(np.int64)), diff.max()


def test_redo_list_grows_across_calls_with_coloured_input(eng, oracle):
    """One handle's list of pairs to compute apart: sized by a 3-frame call, outgrown by 961 frames most of whose pairs
    go onto it, reused by 2 frames.  Every call against the oracle; the large one twice, to the same bits."""
    ocfg = oracle.mfcc_cfg(n_bins=256, **KW4)
    frames = _shifted(R.frames_of(R.cases(400, 16000.0)), 400)
    want = _want(oracle, ("pair", 40), ocfg, frames)
    m = eng.mfcc(**KW4)
    _check(_call(m, frames[:3]), want[:3])
    big = _call(m, frames)
    _check(big, want)
    assert np.array_equal(_call(m, frames).view(np.int64), big.view(np.int64))
    _check(_call(m, frames[5:7]), want[5:7])
    m.close()
    m = eng.mfcc(**KW4)                                                         # a grown handle is gone; a fresh one starts from nothing
    _check(_call(m, frames[-2:]), want[-2:])
    m.close()
