"""The cases the batched n-microphone MVDR tests share (jdsp_mvdrn_batch*, include/jdsp.h): the scenes, the packing of
a batch on n_mics planes, the oracle per utterance and the bars.  No GPU import: tests/test_mvdrn_batch_cpu.py uses the
same scenes to show that the GPU comparison is not vacuous.

Bars (tests/test_mvdr_multi_gpu.py's): precast within 1e-5 of the utterance's own peak, int16 within 1 LSB, finite
masks equal, each utterance against oracle.mvdrn_stream on it alone."""
import numpy as np

B = 512                                                   # samples per block of a 1024-point handle
TOL = 1e-5
P = 128                                                   # kMvnBatchEvents (csrc/jdsp_internal.h): estimation frames per chunk
COUNTS = [0, 1, 2, 3, 0, 5, 12, 40, 1, 70, 0]             # the oracle-per-utterance batch
N_MICS = [2, 3, 5, 8]
LOADING = 1e-3


def array_scene(seed, n_mics, n_blocks, src_delay=1, quiet=((0, 14), (30, 12))):
    """tests/test_mvdr_multi_gpu.py's recipe: a loud source delayed by src_delay samples per microphone, a weak
    interferer and sensor noise; `quiet` lists (first block, blocks) stretches without the source."""
    rng = np.random.default_rng(seed)
    n = n_blocks * 512
    src = rng.normal(0, 3000, n)
    interf = rng.normal(0, 30, n)
    pcm = np.stack([np.roll(src, src_delay * m) for m in range(n_mics)])
    for b0, nb in quiet:
        if b0 + nb <= n_blocks:
            pcm[:, b0 * 512:(b0 + nb) * 512] = 0
    pcm = pcm + rng.normal(0, 20, (n_mics, n)) + np.stack([np.roll(interf, -2 * m) for m in range(n_mics)])
    return np.clip(np.rint(pcm), -32768, 32767).astype(np.int16), src, -src_delay * np.arange(n_mics) / 16000.0


def delays_of(n_mics):
    return -np.arange(n_mics) / 16000.0


def utterance(seed, n_mics, n_blocks, quiet=None):
    """int16 [n_mics, 512 n_blocks].  An utterance of three blocks or more starts with a quiet lead of min(6, n_blocks)
    blocks unless `quiet` says otherwise, so its first estimation frame is block 1."""
    if quiet is None:
        quiet = ((0, min(6, n_blocks)),) if n_blocks >= 3 else ()
    return array_scene(seed, n_mics, n_blocks, quiet=quiet)[0]


def oracle_batch_utts(n_mics):
    """the utterances of the oracle-per-utterance case: seeds 100 n_mics + u"""
    return [utterance(100 * n_mics + u, n_mics, n) for u, n in enumerate(COUNTS)]


def boundary_pair():
    """3 microphones: A (8 blocks) ends in two quiet blocks, B (8 blocks) starts with two.  As one stream A's last block,
    B's first and B's second are estimation frames and B's first frame reads A's last block; alone, B has one estimation
    frame (its block 1) and silence in front of it."""
    a = utterance(1, 3, 8, quiet=((6, 2),))
    b = utterance(2, 3, 8, quiet=((0, 2),))
    return a, b


def events_run(seed, n_events, n_mics=3, tail=4):
    """one utterance with exactly n_events estimation frames: a quiet run of n_events + 1 blocks from block 0 (block 0
    is never one, every later quiet block is), then `tail` loud blocks"""
    return utterance(seed, n_mics, n_events + 1 + tail, quiet=((0, n_events + 1),))


def pack(utts, gaps=None, pad=0):
    """The planes of a batch: utterance u at sample_first[u], gaps[u] samples (even) in front of it, the total rounded up
    to a multiple of 8 plus `pad` samples.  Returns (pcm [n_mics, n_samples], counts, sample_first); what lies between the
    spans is loud noise, so a kernel that reads it shows."""
    n_mics = utts[0].shape[0]
    gaps = [0] * len(utts) if gaps is None else list(gaps)
    counts = np.array([u.shape[1] // B for u in utts], np.int64)
    first, pos = [], 0
    for u, g in zip(utts, gaps):
        pos += g
        first.append(pos)
        pos += u.shape[1]
    n_samples = (pos + 7) // 8 * 8 + pad
    pcm = np.random.default_rng(len(utts) + n_samples).integers(-9000, 9000, (n_mics, n_samples)).astype(np.int16)
    for u, s in zip(utts, first):
        pcm[:, s:s + u.shape[1]] = u
    return pcm, counts, np.array(first, np.int64)


def oracle_flags(orc, utt):
    """the VAD decision of every block on microphone 0"""
    return np.array([orc.mvdr_vad_block(utt[0, b * B:(b + 1) * B])[0] for b in range(utt.shape[1] // B)], np.uint8)


def events_of(flags):
    """the estimation frames of a fresh stream with these decisions: quiet blocks behind a quiet block"""
    quiet = np.asarray(flags) == 0
    return int(np.count_nonzero(quiet[1:] & quiet[:-1]))


def oracle_utt(orc, utt, loading=LOADING):
    """(out int16, precast float64) of the utterance alone: max(B_u - 1, 0) blocks"""
    if utt.shape[1] == 0:
        return np.zeros(0, np.int16), np.zeros(0, np.float64)
    return orc.mvdrn_stream(utt, delays_of(utt.shape[0]), loading)


def span_of(x, sample_first, n_blocks):
    """the emitted samples of an utterance out of a time-aligned plane: its blocks 1 .. n_blocks - 1"""
    return x[sample_first + B:sample_first + n_blocks * B]


def check(out, pre, o_out, o_pre, held=None):
    """Returns the share of the 1e-5 bar the worst finite sample takes (0 without finite samples).  `held` (bool per
    sample, tests/mvdrn_cases.py's held_mask) names the samples that count; None: all of them."""
    assert out.shape == o_out.shape and pre.shape == o_pre.shape
    if held is not None:
        assert held.shape == pre.shape
        out, pre, o_out, o_pre = out[held], pre[held], o_out[held], o_pre[held]
    fin = np.isfinite(o_pre)
    assert np.array_equal(np.isfinite(pre), fin)
    worst = 0.0
    if fin.any():
        worst = float(np.abs(pre[fin] - o_pre[fin]).max() / (TOL * max(np.abs(o_pre[fin]).max(), 1.0)))
        assert worst < 1.0, worst
    assert out.size == 0 or np.abs(out.astype(np.int32) - o_out.astype(np.int32)).max() <= 1
    return worst


def check_batch(orc, utts, sample_first, out, pre, flags=None, loading=LOADING):
    """every utterance of a time-aligned result against its own oracle; returns the worst share of the bar"""
    worst, pos = 0.0, 0
    for u, s in zip(utts, sample_first):
        nb = u.shape[1] // B
        o_out, o_pre = oracle_utt(orc, u, loading)
        worst = max(worst, check(span_of(out, int(s), nb) if nb else out[:0], span_of(pre, int(s), nb) if nb else pre[:0],
                                 o_out, o_pre))
        if flags is not None:
            assert np.array_equal(flags[pos:pos + nb], oracle_flags(orc, u))
        pos += nb
    return worst
