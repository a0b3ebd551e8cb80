"""GPU parity: FFT-autocorrelation pitch (PitchEstimation_method1.cpp).
Autocorrelation within 1e-5 of r[0]; the arg-max lag equals the oracle's wherever the oracle's
maximum is unique to within that tolerance (FP32 cannot order values closer than its round-off;
in that case the returned lag must still be one of the tied maxima)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def voiced(seed, n_blocks, f0=137.0, fs=16000.0):
    rng = np.random.default_rng(seed)
    t = np.arange(n_blocks * 512)
    f = f0 * (1 + 0.05 * np.sin(2 * np.pi * 0.7 * t / fs))
    ph = 2 * np.pi * np.cumsum(f) / fs
    x = 5000 * np.sin(ph) + 2500 * np.sin(2 * ph + 0.3) + 1200 * np.sin(3 * ph + 1.0) + rng.normal(0, 200, t.size)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def check(arg, rmax, ac, o_arg, o_max, o_ac):
    scale = o_ac[:, 0:1].max(axis=1, keepdims=True) + 1.0
    assert (np.abs(ac - o_ac) / scale).max() < 1e-5
    tol = 1e-5 * scale[:, 0]
    assert np.all(np.abs(rmax - o_max) <= tol)
    same = arg == o_arg
    # where they differ, the oracle's value at OUR lag must tie with its maximum
    at_ours = o_ac[np.arange(len(arg)), arg]
    assert np.all(same | (o_max - at_ours <= tol))
    assert same.mean() > 0.98
    assert np.all((arg > 100) & (arg < 512))


@pytest.mark.parametrize("n_blocks", [1, 2, 50])
def test_pitch_matches_oracle(eng, oracle, n_blocks):
    pcm = voiced(n_blocks, n_blocks)
    o_arg, o_max, o_ac = oracle.pitch_stream(pcm)
    arg, rmax, ac = eng.pitch(pcm, want_autocorr=True)
    check(arg, rmax, ac, o_arg, o_max, o_ac)
    if n_blocks == 50:
        est = 16000.0 / arg[5:]
        assert np.median(np.abs(est - 137.0)) < 6.0 or np.median(np.abs(est - 68.5)) < 3.0   # f0 or its sub-octave


def test_pitch_noise_device_path_and_prev_block(eng, oracle):
    import torch
    rng = np.random.default_rng(0)
    pcm = np.clip(np.rint(rng.normal(0, 3000, 300 * 512)), -32768, 32767).astype(np.int16)
    o_arg, o_max, o_ac = oracle.pitch_stream(pcm)
    t = torch.from_numpy(pcm).cuda()
    arg, rmax, ac = eng.pitch(t, want_autocorr=True)
    torch.cuda.synchronize()
    check(arg.cpu().numpy(), rmax.cpu().numpy(), ac.cpu().numpy(), o_arg, o_max, o_ac)
    # streaming: second half with the keep buffer handed over
    a2, m2 = eng.pitch(t[150 * 512:], prev_block=t[149 * 512:150 * 512].clone())
    torch.cuda.synchronize()
    assert torch.equal(a2, arg[150:]) and torch.equal(m2, rmax[150:])


def test_pitch_silence_and_compat_calcpitch(eng, oracle, tmp_path):
    z = np.zeros(4 * 512, np.int16)
    arg, rmax = eng.pitch(z)
    o_arg, o_max, _ = oracle.pitch_stream(z)
    assert np.array_equal(arg, o_arg) and np.all(rmax == 0)          # all-equal zeros: smallest lag 101 wins
    pcm = voiced(9, 12)
    pcm.tofile(tmp_path / "in.raw")
    exe = os.path.join(ROOT, "jeicyboodsp_amd", "compat", "compat_selftest")
    subprocess.run([exe, "pitch", str(tmp_path / "in.raw"), str(tmp_path / "out.bin")], check=True,
                   stdout=subprocess.DEVNULL, timeout=120)
    got = np.fromfile(tmp_path / "out.bin", np.int32)
    o_arg, o_max, o_ac = oracle.pitch_stream(pcm)
    at_ours = o_ac[np.arange(12), got]
    assert np.all((got == o_arg) | (o_max - at_ours <= 1e-5 * o_ac[:, 0]))


# ---- the input families of the time-domain pitch entries (timedomain_ref.pitch_families), and a DC offset ----------
ORDERED = ("voiced", "white", "mixed", "dc_offset")        # families whose maxima FP32 can order: the share is asserted


def families(n_blocks):
    import timedomain_ref as T
    fam = dict(T.pitch_families(n_blocks))
    fam["dc_offset"] = (T.voiced(11, n_blocks).astype(np.int32) + 12000).astype(np.int16)
    assert np.abs(fam["dc_offset"].astype(np.int32) - 12000).max() < 20000          # nothing clipped or wrapped
    return fam


def check_family(name, arg, rmax, ac, o_arg, o_max, o_ac):
    """check()'s rules; the share of equal lags only where the family has an order to find (on constant, silence and
    full_scale every lag may tie with the maximum within the tolerance, and the tie rule is the whole check)"""
    scale = o_ac[:, 0] + 1.0
    err = float((np.abs(ac - o_ac) / scale[:, None]).max())
    tol = 1e-5 * scale
    same = arg == o_arg
    at_ours = o_ac[np.arange(len(arg)), arg]
    print("PITCH %-10s %2d blocks: autocorr %.3g of r[0] + 1, rmax %.3g, lags equal %d of %d"
          % (name, len(arg), err, float((np.abs(rmax - o_max) / scale).max()), int(same.sum()), len(arg)))
    assert err < 1e-5
    assert np.all(np.abs(rmax - o_max) <= tol)
    assert np.all(same | (o_max - at_ours <= tol))
    assert np.all((arg >= 101) & (arg <= 511))
    if name in ORDERED:
        assert same.mean() > 0.98
    if name == "silence":
        assert np.all(arg == 101) and not rmax.any() and not ac.any()


@pytest.mark.parametrize("n_blocks", [1, 2, 50])
def test_pitch_families_host_and_device_with_hand_over(eng, oracle, n_blocks):
    import torch
    for name, pcm in families(n_blocks).items():
        o_arg, o_max, o_ac = oracle.pitch_stream(pcm)
        arg, rmax, ac = eng.pitch(pcm, want_autocorr=True)                                 # host entry
        check_family(name, arg, rmax, ac, o_arg, o_max, o_ac)
        t = torch.from_numpy(pcm).cuda()
        d_arg, d_max, d_ac = eng.pitch(t, want_autocorr=True)                              # device entry
        torch.cuda.synchronize()
        d_arg, d_max, d_ac = d_arg.cpu().numpy(), d_max.cpu().numpy(), d_ac.cpu().numpy()
        check_family(name, d_arg, d_max, d_ac, o_arg, o_max, o_ac)
        assert np.array_equal(d_arg, arg) and np.array_equal(d_max.view(np.uint32), rmax.view(np.uint32))
        assert np.array_equal(d_ac.view(np.uint32), ac.view(np.uint32))
        if n_blocks < 2:
            continue
        # a cut with the keep buffer handed over: the blocks after it are the one-call stream's, bit for bit
        c = n_blocks // 2
        prev = pcm[(c - 1) * 512:c * 512]
        h_arg, h_max, h_ac = eng.pitch(pcm[c * 512:], prev_block=prev, want_autocorr=True)
        assert np.array_equal(h_arg, arg[c:]) and np.array_equal(h_max.view(np.uint32), rmax[c:].view(np.uint32))
        assert np.array_equal(h_ac.view(np.uint32), ac[c:].view(np.uint32))
        c_arg, c_max, c_ac = eng.pitch(t[c * 512:], prev_block=t[(c - 1) * 512:c * 512].clone(), want_autocorr=True)
        torch.cuda.synchronize()
        assert np.array_equal(c_arg.cpu().numpy(), arg[c:])
        assert np.array_equal(c_max.cpu().numpy().view(np.uint32), rmax[c:].view(np.uint32))
        assert np.array_equal(c_ac.cpu().numpy().view(np.uint32), ac[c:].view(np.uint32))
