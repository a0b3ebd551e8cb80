"""GPU parity: MFCC front end against the CPU oracle.  MelFilterBankInit's tables
are double-precision host work -> exact vs the oracle (and vs the known answers
SURVEY.md quotes); feature vectors within 1e-5 relative to the vector's peak."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def _pcm(seed, n, sigma=3000.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0.0, sigma, n)), -32768, 32767).astype(np.int16)


def _check(got, want):
    peak = np.abs(want).max(axis=1, keepdims=True)
    assert (np.abs(got - want) / peak).max() < TOL


def test_mel_tables_exact_and_known_answers(eng, oracle):
    m = eng.mfcc()
    mel, fi, fb = m.tables()
    omel, ofi, ofb = oracle.mel_init(oracle.mfcc_native_cfg())
    assert np.array_equal(mel, omel) and np.array_equal(fi, ofi) and np.array_equal(fb, ofb)
    assert abs(mel[0] - 65.357) < 5e-4 and abs(mel[-1] - 22050.0) < 1e-9
    assert np.bincount(fi, minlength=39)[38] == 46
    m.close()


@pytest.mark.parametrize("n_blocks", [1, 2, 9, 40])
def test_native_stream_matches_oracle(eng, oracle, n_blocks):
    """One file as the reference reads it: blocks of 1024, 2B-1 vectors (MFCC:86-104)."""
    pcm = _pcm(n_blocks, n_blocks * 1024)
    want = oracle.mfcc_stream(oracle.mfcc_native_cfg(), pcm)
    m = eng.mfcc()
    got = m.frames(pcm)                       # hop-512 framing of the file = the 2B-1 kept vectors
    assert got.shape == want.shape == (2 * n_blocks - 1, 12)
    _check(got, want)
    m.close()


def test_speechlike_levels_and_device_path(eng, oracle):
    import torch
    rng = np.random.default_rng(3)
    n = 64 * 1024
    t = np.arange(n)
    x = (6000 * np.sin(2 * np.pi * 220 * t / 44100) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t / 44100))
         + rng.normal(0, 30, n))
    pcm = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    want = oracle.mfcc_stream(oracle.mfcc_native_cfg(), pcm)
    m = eng.mfcc()
    got = m.frames(torch.from_numpy(pcm).cuda())
    torch.cuda.synchronize()
    _check(got.cpu().numpy(), want)
    m.close()


def test_baseline_config_400_160_512fft_40mel(eng, oracle):
    """BASELINE config 4: 25 ms / 10 ms framing at 16 kHz, 512-FFT, 40 mel channels."""
    kw = dict(win_len=400, hop=160, n_fft=512, n_chan=40, n_cep=13, half_rate=8000.0)
    ocfg = oracle.mfcc_cfg(n_bins=256, **kw)
    pcm = _pcm(5, 16000)
    m = eng.mfcc(**kw)
    nf = m.n_frames(pcm.size)
    assert nf == 98
    got = m.frames(pcm)
    want = oracle.mfcc_frames(ocfg, pcm, nf)
    _check(got, want)
    mel, fi, fb = m.tables()
    omel, ofi, ofb = oracle.mel_init(ocfg)
    assert np.array_equal(mel, omel) and np.array_equal(fi, ofi) and np.array_equal(fb, ofb)
    m.close()
    # one handle's list of frame pairs to redo: sized by 3 frames (2 pairs), exceeded by 98, reused by 2
    m = eng.mfcc(**kw)
    for n in (720, 16000, 560):
        nf = m.n_frames(n)
        _check(m.frames(pcm[:n]), oracle.mfcc_frames(ocfg, pcm[:n], nf))
    assert nf == 2
    m.close()
    eng.mfcc(**kw).close()                    # a grown handle is gone; the next one starts from nothing


def test_utterance_batch_with_frame_starts(eng, oracle):
    """Ragged utterances packed back to back; every utterance framed on its own."""
    cfg = oracle.mfcc_native_cfg()
    lens = [1024, 5000, 2048, 1023, 12345, 3072]
    pcm = _pcm(8, sum(lens))
    starts, want = [], []
    off = 0
    for n in lens:
        nf = (n - 1024) // 512 + 1 if n >= 1024 else 0          # empty for the 1023-sample utterance
        starts += [off + 512 * j for j in range(nf)]
        if nf:
            want.append(oracle.mfcc_frames(cfg, pcm[off:off + n], nf))
        off += n
    m = eng.mfcc()
    got = m.frames(pcm, frame_start=np.array(starts, np.int64))
    _check(got, np.concatenate(want))
    with pytest.raises(Exception):
        m.frames(pcm, frame_start=np.array([pcm.size - 100], np.int64))      # frame runs off the buffer
    m.close()


def test_silent_frame_gives_minus_inf_like_reference(eng, oracle):
    pcm = np.zeros(2048, np.int16)
    want = oracle.mfcc_stream(oracle.mfcc_native_cfg(), pcm)
    m = eng.mfcc()
    got = m.frames(pcm)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and not np.isfinite(got).any()
    m.close()


@pytest.mark.parametrize("kw,n_bins", [
    (dict(n_chan=64, n_cep=20), 512),                                   # 65 channel indices: more pieces than lanes,
    (dict(win_len=512, hop=256, n_fft=512, n_chan=64, n_cep=13, half_rate=8000.0), 256),   # the one-frame kernel runs
    (dict(n_chan=12, n_cep=12), 512),                                   # wide channels: several 16-bin pieces each
    (dict(n_chan=1, n_cep=1), 512),
    (dict(n_chan=38, n_cep=20), 512),                                   # more than 16 cepstra: two lane groups, DCT tail loop
    (dict(n_chan=26, n_cep=13), 512),                                   # pieces of 16 bins (38 channels: 12)
    (dict(win_len=400, hop=160, n_fft=512, n_chan=20, n_cep=13, half_rate=8000.0), 256),   # pair kernel, pieces longer than 8
    (dict(win_len=1000, hop=250, n_chan=38, n_cep=12), 512),            # window shorter than the transform: clamped loads
])
def test_filterbank_shapes_and_odd_frame_counts(eng, oracle, kw, n_bins):
    """Both MFCC kernels (two frames per wave with one filterbank piece per lane; one frame per wave when the
    pieces do not fit 64 lanes) and frame counts that leave the last wave half empty."""
    ocfg = oracle.mfcc_cfg(n_bins=n_bins, **kw)
    m = eng.mfcc(**kw)
    win, hop = m.cfg.win_len, m.cfg.hop
    for nf in (1, 2, 7):
        pcm = _pcm(40 + nf, win + hop * (nf - 1))
        got = m.frames(pcm)
        assert got.shape == (nf, m.cfg.n_cep)
        _check(got, oracle.mfcc_frames(ocfg, pcm, nf))
    m.close()


def test_baseline_config4_ten_thousand_ragged_utterances(eng, oracle):
    """BASELINE config 4 as worded: 25 ms / 10 ms framing (400/160 at 16 kHz), 512-FFT, 40 mel + DCT, on a
    10,000-utterance batch (ragged, 1-6 s each, packed back to back, every utterance framed on its own through
    frame_start).  All ~3.5 M frames are computed on the device in one call; a sample of utterances (the first,
    the last, the shortest, the longest and 20 seeded ones) is compared frame by frame with the oracle, and
    every vector of the batch must be finite (the input has no silent frame)."""
    import torch
    kw = dict(win_len=400, hop=160, n_fft=512, n_chan=40, n_cep=13, half_rate=8000.0)
    ocfg = oracle.mfcc_cfg(n_bins=256, **kw)
    rng = np.random.default_rng(2024)
    n_utts = 10000
    lens = rng.integers(16000, 6 * 16000 + 1, n_utts)
    offs = np.concatenate([[0], np.cumsum(lens)])
    total = int(offs[-1])
    # speech-like content without building 350 M normal deviates: a seeded 4 M-sample noise table, tiled
    table = np.clip(np.rint(rng.normal(0, 3000, 1 << 22)), -32768, 32767).astype(np.int16)
    pcm = np.tile(table, total // table.size + 1)[:total]
    nf = (lens - 400) // 160 + 1
    first = np.concatenate([[0], np.cumsum(nf)])
    starts = np.concatenate([offs[u] + 160 * np.arange(nf[u], dtype=np.int64) for u in range(n_utts)])
    assert starts.size == first[-1] and 3_000_000 < starts.size < 4_000_000
    m = eng.mfcc(**kw)
    d_pcm = torch.from_numpy(pcm).cuda()
    d_starts = torch.from_numpy(starts).cuda()
    feats = m.frames(d_pcm, frame_start=d_starts)
    torch.cuda.synchronize()
    assert feats.shape == (starts.size, 13)
    assert bool(torch.isfinite(feats).all())
    pick = sorted(set([0, n_utts - 1, int(np.argmin(lens)), int(np.argmax(lens))] +
                      rng.integers(0, n_utts, 20).tolist()))
    for u in pick:
        got = feats[first[u]:first[u + 1]].cpu().numpy()
        want = oracle.mfcc_frames(ocfg, pcm[offs[u]:offs[u + 1]], int(nf[u]))
        _check(got, want)
    # an utterance's vectors do not depend on its neighbours beyond rounding: recomputed alone through the host entry
    # its frames pair up differently inside the shared transforms (mfcc512_run_kernel: two frames per transform), which
    # moves results by FP32 rounding only
    u = pick[len(pick) // 2]
    alone = m.frames(pcm[offs[u]:offs[u + 1]])
    batch = feats[first[u]:first[u + 1]].cpu().numpy()
    assert (np.abs(alone - batch) / np.abs(batch).max(axis=1, keepdims=True)).max() < 2e-6
    m.close()


def test_paired_frames_of_very_different_level_and_silence(eng, oracle):
    """512-FFT configurations put two frames into one transform.  A loud frame's rounding must not show in a quiet
    partner (separate passes: test_mfcc_coloured_gpu.py has the coloured cases), and an all-zero frame keeps the
    reference's ln 0 = -inf whatever it is paired with."""
    kw = dict(win_len=400, hop=160, n_fft=512, n_chan=40, n_cep=13, half_rate=8000.0)
    ocfg = oracle.mfcc_cfg(n_bins=256, **kw)
    rng = np.random.default_rng(31)
    n = 400 + 160 * 39
    pcm = np.rint(rng.normal(0, 2.0, n)).astype(np.int16)                   # a few LSB of noise ...
    pcm[160 * 20 + 240:] = np.clip(np.rint(rng.normal(0, 9000, n - 160 * 20 - 240)), -32768, 32767).astype(np.int16)   # ... then 73 dB louder
    pcm[160 * 4:160 * 4 + 400 + 160] = 0                                    # frames 4 and 5 all zero; 3 and 6 partly
    m = eng.mfcc(**kw)
    for first_frame in (0, 1):                                              # both pairings of every neighbour
        x = pcm[160 * first_frame:]
        nf = (x.size - 400) // 160 + 1
        got = m.frames(x)
        want = oracle.mfcc_frames(ocfg, x, nf)
        fin = np.isfinite(want).all(axis=1)
        assert np.array_equal(np.isfinite(got).all(axis=1), fin) and (~fin).sum() == 2
        _check(got[fin], want[fin])
    m.close()


# ---- MelFilterBank / DCT / Liftering as functions of their own (MFCC:154-192) ----------------------
STEP_TOL = 1e-12          # FP64 in the reference's order; only log() can differ from the CPU, in its last place


@pytest.mark.parametrize("kw,n_bins", [(dict(), 512), (dict(win_len=400, hop=160, n_fft=512, n_chan=40, n_cep=13, half_rate=8000.0), 256)])
def test_mfcc_sub_steps_match_the_oracle(eng, oracle, kw, n_bins):
    ocfg = oracle.mfcc_cfg(n_bins=n_bins, **kw)
    m = eng.mfcc(**kw)
    rng = np.random.default_rng(9)
    mag = np.abs(rng.normal(0, 5e4, (37, n_bins))) + 1.0
    mel = m.mel_filterbank(mag)
    want_mel = oracle.mel_filterbank(ocfg, mag)
    assert mel.shape == want_mel.shape and np.abs(mel - want_mel).max() <= STEP_TOL * np.abs(want_mel).max()
    cep = m.dct(want_mel)
    want_cep = oracle.dct(ocfg, want_mel)
    assert np.abs(cep - want_cep).max() <= STEP_TOL * np.abs(want_cep).max()
    # the reference's DCT accumulates (:180 `+=`): a pre-filled output comes back as pre-fill + DCT
    pre = rng.normal(0, 100, want_cep.shape)
    acc = m.dct(want_mel, accumulate_into=pre)
    assert np.abs(acc - oracle.dct(ocfg, want_mel, accumulate_into=pre)).max() <= STEP_TOL * np.abs(pre).max()
    assert np.abs(acc - cep).max() > 1.0
    lif = m.liftering(want_cep)
    assert np.array_equal(lif, oracle.liftering(ocfg, want_cep))            # one multiply by a host-built constant
    # chained, the three steps are MFCCFeatureExtraction's tail (:223-226): equal to the fused kernel's vectors
    pcm = _pcm(21, m.cfg.win_len + m.cfg.hop * 4)
    fused = m.frames(pcm)
    spec_n = m.cfg.n_fft
    frames = np.stack([pcm[m.cfg.hop * j:m.cfg.hop * j + m.cfg.win_len].astype(np.float64) for j in range(5)])
    x = np.zeros((5, spec_n))
    x[:, 1:m.cfg.win_len] = frames[:, 1:] - m.cfg.preemph * frames[:, :-1]
    x[:, :m.cfg.win_len] *= oracle.hamming(m.cfg.win_len)
    mag2 = np.abs(np.fft.fft(x, axis=1))[:, :n_bins]
    chained = m.liftering(m.dct(m.mel_filterbank(mag2)))
    _check(fused, chained)
    m.close()


def test_mel_filterbank_empty_channel_gives_minus_inf(eng, oracle):
    m = eng.mfcc()
    mel = m.mel_filterbank(np.zeros((1, 512)))
    assert np.all(np.isneginf(mel))                                         # ln(0), as the reference (:171)
    m.close()
