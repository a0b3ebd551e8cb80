"""Data-parallel sharding of the spectral path over the GPUs of one node.

Frames, convolution blocks and utterances are independent once each shard carries
its input halo, so there is NO data-path collective: rank r transforms its own
contiguous slice.  The only collective is the optional gather of the outputs
(RCCL all_gather when the caller wants the whole buffer on every rank).

Pure index arithmetic + torch.distributed calls; works with any backend
(tests run it on CPU with gloo, world_size 2).
"""
from collections import namedtuple

Shard = namedtuple("Shard", "first count sample_first sample_count")


def split_even(n, rank, world):
    """Contiguous, balanced split of n units: the first n % world ranks get one more."""
    base, rem = divmod(n, world)
    first = rank * base + min(rank, rem)
    return first, base + (1 if rank < rem else 0)


def stream_shard(n_streams, rank, world):
    """Streams [first, first+count) of a multi-stream filter (Engine.geq, Engine.nlms): streams never exchange
    anything, so a rank owns whole streams, state included, and there is no halo."""
    return split_even(n_streams, rank, world)


def stft_shard(n_frames, rank, world, n_fft=1024, hop=512):
    """Frames [first, first+count) and the PCM slice they need: frame f covers
    samples [hop*f, hop*f + n_fft), so neighbouring shards overlap by n_fft - hop samples."""
    first, count = split_even(n_frames, rank, world)
    if count == 0:
        return Shard(first, 0, hop * first, 0)
    return Shard(first, count, hop * first, hop * (count - 1) + n_fft)


def fastconv_shard(n_out_blocks, rank, world, block, n_taps):
    """Output blocks [first, first+count) of an overlap-save stream (numbered from the first
    EMITTED block) and the input samples they need: n_taps - 1 samples of history in front."""
    first, count = split_even(n_out_blocks, rank, world)
    if count == 0:
        return Shard(first, 0, first * block, 0)
    return Shard(first, count, first * block - (n_taps - 1), count * block + (n_taps - 1))


def utterance_shard(frames_per_utt, rank, world):
    """Whole utterances per rank, contiguous, balanced by frame count (prefix-sum cut points).
    Returns (first_utt, n_utt)."""
    prefix = [0]
    for f in frames_per_utt:
        prefix.append(prefix[-1] + f)
    total = prefix[-1]
    cuts = [0]
    u = 0
    for r in range(1, world):
        target = total * r / world
        while u < len(frames_per_utt) and abs(prefix[u + 1] - target) <= abs(prefix[u] - target):
            u += 1
        cuts.append(u)
    cuts.append(len(frames_per_utt))
    return cuts[rank], cuts[rank + 1] - cuts[rank]


def all_gather_rows(local, counts, dist, group=None):
    """Gathers row-sharded tensors of unequal length: local is [counts[rank], ...]; returns
    [sum(counts), ...] on every rank.  Shards are padded to the longest so a single
    all_gather_into_tensor moves everything (one large collective, not world_size small ones)."""
    import torch
    world = len(counts)
    longest = max(counts)
    tail = tuple(local.shape[1:])
    padded = local
    if local.shape[0] != longest:
        padded = torch.zeros((longest,) + tail, dtype=local.dtype, device=local.device)
        padded[: local.shape[0]] = local
    out = torch.empty((world * longest,) + tail, dtype=local.dtype, device=local.device)
    real = padded.is_complex()
    if real:
        dist.all_gather_into_tensor(torch.view_as_real(out), torch.view_as_real(padded.contiguous()), group=group)
    else:
        dist.all_gather_into_tensor(out, padded.contiguous(), group=group)
    if all(c == longest for c in counts):
        return out
    return torch.cat([out[r * longest: r * longest + counts[r]] for r in range(world)])


def denoise_shard_range(n_blocks, rank, world):
    """Blocks [b0, b1) a rank owns and the first block it must be given (two halo blocks)."""
    b0, count = split_even(n_blocks, rank, world)
    return max(b0 - 2, 0), b0, b0 + count


def denoise_sharded(denoiser, pcm_ext, ext0, b0, b1, n_total, rank, world, gather):
    """One rank's part of a spectral-subtraction / Wiener run over ONE global stream.

    pcm_ext: torch int16 CUDA tensor with global blocks [ext0, b1).  gather(t, counts) must return
    the concatenation over ranks of each rank's t (counts[r] rows of it): with torch.distributed,
    ``lambda t, c: all_gather_rows(t, c, dist)``.  Three small exchanges (voice flags, one
    (alpha, beta[1024]) pair per rank, one latched estimate per rank); the heavy kernels see
    only the rank's own blocks.  Returns the rank's emitted int16 blocks."""
    own = [split_even(n_total, r, world)[1] for r in range(world)]
    flags_own = denoiser.shard_vad(pcm_ext, ext0, b0, b1, n_total)
    flags_all = gather(flags_own.reshape(-1, 1), own).reshape(-1).contiguous()
    summary = denoiser.shard_summary(flags_all)
    summaries = gather(summary.reshape(1, -1), [1] * world).contiguous()
    last = denoiser.shard_rows(summaries, world, rank)
    lasts = gather(last.reshape(1, -1), [1] * world).contiguous()
    return denoiser.shard_finish(lasts, world, rank)


def istft_frame_shard(n_frames, world, rank, R):
    """STFT synthesis (jdsp_istft) of ONE stream of n_frames spectra over `world` ranks: rank owns frames
    [first, end) and emits their samples [hop*first, hop*end); its output samples also take contributions from the
    R - 1 frames in front (R = n_fft / hop), so it replays frames [halo, first) without output first.
    Returns (halo, first, end).  Concatenating the ranks' outputs (plus the last rank's flush) is the single stream."""
    first, count = split_even(n_frames, rank, world)
    return max(first - (R - 1), 0), first, first + count


def istft_sharded(istft, spec, n_frames, world, rank, want_f32=False):
    """One rank's part of an STFT synthesis stream: reset, prime the halo frames with NULL outputs (the stream advances
    without writing), then the rank's own frames.  spec: the rank-sliceable [n_frames, pitch] spectra (only rows
    [halo, end) are read).  Returns what istft.process returns for the own frames (None when the rank owns none);
    bit-identical to the same samples of a single-call run."""
    halo, first, end = istft_frame_shard(n_frames, world, rank, istft.n_fft // istft.hop)
    istft.reset()
    if end == first:
        return None
    if first > halo:
        istft.process(spec[halo:first], write=False)
    return istft.process(spec[first:end], want_f32=want_f32)


def stftmask_sharded(stftmask, pcm, mask, n_frames, world, rank, want_f32=False):
    """One rank's part of a fused STFT masking stream (jdsp_stftmask): the frame split, the halo and the priming are
    istft_frame_shard's -- reset, run the R - 1 halo frames with NULL outputs, then the rank's own frames.  pcm: the
    stream's samples (only those of frames [halo, end) are read); mask: [n_frames, pitch] rows, or 1-D (one row for
    every frame).  Returns what stftmask.process returns for the own frames (None when the rank owns none);
    bit-identical to the same samples of a single-call run."""
    n, hop = stftmask.n_fft, stftmask.hop
    halo, first, end = istft_frame_shard(n_frames, world, rank, n // hop)
    stftmask.reset()
    if end == first:
        return None

    def part(a, b):
        return pcm[hop * a: hop * (b - 1) + n], (mask if mask.ndim == 1 else mask[a:b]), b - a

    if first > halo:
        stftmask.process(*part(halo, first), write=False)
    return stftmask.process(*part(first, end), want_f32=want_f32)


def stftmask_batch_layout(utt_sample_first, n_fft, hop):
    """A batch of utterances packed at the n_utts + 1 sample offsets utt_sample_first (mfcc_utterance_shard's
    convention), as jdsp_stftmask_batch frames it: utterance u of L_u = offs[u + 1] - offs[u] samples has
    F_u = (L_u - n_fft) // hop + 1 frames when L_u >= n_fft, else none; its mask rows start at frame_first[u].
    Returns (frame_counts [n_utts], frame_first [n_utts + 1]) as numpy int64.  Offsets must be even (the kernel's
    aligned accesses) and must not decrease: ValueError otherwise."""
    import numpy as np
    offs = np.asarray(utt_sample_first, dtype=np.int64).reshape(-1)
    if offs.size < 1:
        raise ValueError("utt_sample_first holds n_utts + 1 offsets")
    if np.any(offs & 1):
        raise ValueError("utterance offsets must be even")
    lens = offs[1:] - offs[:-1]
    if offs[0] < 0 or np.any(lens < 0):
        raise ValueError("utterance offsets must be >= 0 and must not decrease")
    counts = np.where(lens >= n_fft, (lens - n_fft) // hop + 1, 0).astype(np.int64)
    return counts, np.concatenate([np.zeros(1, np.int64), np.cumsum(counts, dtype=np.int64)])


def _pack_back_to_back(counts, n, hop, what):
    """Utterance u of counts[u] >= 0 units (what: their name in the ValueError) takes hop (counts[u] - 1) + n samples,
    none when it has no unit, and the spans follow each other without a gap.  Returns (sample_first [n_utts + 1],
    unit_first [n_utts + 1]) as numpy int64."""
    import numpy as np
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if np.any(counts < 0):
        raise ValueError("%s counts must be >= 0" % what)
    spans = np.where(counts > 0, hop * (counts - 1) + n, 0).astype(np.int64)
    zero = np.zeros(1, np.int64)
    return (np.concatenate([zero, np.cumsum(spans, dtype=np.int64)]),
            np.concatenate([zero, np.cumsum(counts, dtype=np.int64)]))


def istft_batch_layout(frame_counts, n_fft, hop):
    """The back-to-back packing of a batch of synthesis outputs (Istft.process_batch without utt_sample_first):
    utterance u of F_u = frame_counts[u] >= 0 spectrum rows comes out as hop (F_u - 1) + n_fft samples (none when
    F_u = 0), and the spans follow each other without a gap.  Returns (utt_sample_first [n_utts + 1],
    frame_first [n_utts + 1]) as numpy int64; the offsets are even by construction (n_fft and hop are), and
    stftmask_batch_layout(utt_sample_first, n_fft, hop) gives frame_counts and frame_first back.  Negative counts:
    ValueError."""
    packed = _pack_back_to_back(frame_counts, n_fft, hop, "frame")
    if n_fft % 2 or hop % 2:
        raise ValueError("n_fft and hop must be even")
    return packed


def stream_chunks_layout(frame_counts, n_fft, hop, with_pcm):
    """The back-to-back packing of the chunks of one live-streams call (StftMask.process_streams,
    Istft.process_streams): chunk c of F_c = frame_counts[c] >= 0 frames takes, with_pcm (fused masking: the chunk's
    PCM span, of which the first hop F_c samples are its output), hop (F_c - 1) + n_fft samples and none when F_c = 0,
    or, without (synthesis: the output alone), hop F_c samples; the spans follow each other without a gap.  Returns
    (sample_first [n_chunks], frame_first [n_chunks + 1], n_samples) with the two arrays as numpy int64; the offsets
    are even because n_fft and hop are.  A live stream lives on one device: over ranks the stream ids are split with
    stream_shard.  Negative counts, an odd or non-positive hop or n_fft, or n_fft < hop: ValueError."""
    if hop <= 0 or n_fft < hop or n_fft % 2 or hop % 2:
        raise ValueError("n_fft and hop must be even, hop > 0 and n_fft >= hop")
    sample_first, frame_first = _pack_back_to_back(frame_counts, n_fft if with_pcm else hop, hop, "frame")
    return sample_first[:-1].copy(), frame_first, int(sample_first[-1])


def denoise_batch_layout(block_counts, hop):
    """The back-to-back packing of a batch of utterances for Denoiser.process_batch (jdsp_denoise_batch): utterance u
    of B_u = block_counts[u] >= 0 blocks of hop samples takes hop B_u samples, and the spans follow each other
    without a gap.  Returns (sample_first [n_utts], block_first [n_utts + 1], n_samples) with the two arrays as numpy
    int64; the offsets are even because hop is.  Negative counts or an odd hop: ValueError."""
    sample_first, block_first = _pack_back_to_back(block_counts, hop, hop, "block")
    if hop <= 0 or hop % 2:
        raise ValueError("hop must be even and > 0")
    return sample_first[:-1].copy(), block_first, int(sample_first[-1])


def binaural_layout(blocks_per_mix, chunks_per_mix):
    """The back-to-back packing of one binaural delivery (Binaural.render, jdsp_binaural_render): mix m of
    B_m = blocks_per_mix[m] >= 0 output blocks of 512 samples has S_m = chunks_per_mix[m] >= 0 chunks, one per source,
    each 512 B_m new samples long, and the chunks' spans follow each other in list order without a gap.  Returns
    (sample_first [n_chunks], chunk_first [n_mixes + 1], block_first [n_mixes + 1], chunk_mix [n_chunks], n_samples):
    the four arrays as numpy int64, chunk_mix[c] the mix chunk c belongs to.  Input spans may also coincide (two streams
    hearing one source): point their sample_first entries at the same span instead.  Mixes are independent of each
    other, so over ranks a delivery is split by whole mixes: stftmask_batch_shard(blocks_per_mix, rank, world), with a
    mix's streams living on the rank that renders it.  Negative counts or lengths that differ: ValueError."""
    import numpy as np
    blocks = np.asarray(blocks_per_mix, dtype=np.int64).reshape(-1)
    chunks = np.asarray(chunks_per_mix, dtype=np.int64).reshape(-1)
    if blocks.size != chunks.size:
        raise ValueError("one block count and one chunk count per mix")
    if np.any(blocks < 0) or np.any(chunks < 0):
        raise ValueError("block and chunk counts must be >= 0")
    zero = np.zeros(1, np.int64)
    chunk_first = np.concatenate([zero, np.cumsum(chunks, dtype=np.int64)])
    block_first = np.concatenate([zero, np.cumsum(blocks, dtype=np.int64)])
    chunk_mix = np.repeat(np.arange(blocks.size, dtype=np.int64), chunks)
    spans = 512 * blocks[chunk_mix]
    sample_first = np.concatenate([zero, np.cumsum(spans, dtype=np.int64)])
    return sample_first[:-1].copy(), chunk_first, block_first, chunk_mix, int(sample_first[-1])


def denoise_stream_emitted(blocks_seen, block_counts):
    """What the chunks of one Denoiser.process_streams call emit (jdsp_denoise_streams' n_emitted): a stream's first two
    blocks emit nothing (SS:260-263: the reference's call counter), so the chunk of B_c = block_counts[c] blocks of a
    stream that had seen N = blocks_seen[c] blocks emits E_c = B_c - max(0, min(B_c, 2 - N)).  Both arguments are
    per-chunk sequences of equal length (a scalar blocks_seen stands for all chunks).  Returns numpy int64
    [n_chunks].  The layout of the chunks is denoise_batch_layout's with chunks for utterances; a live stream lives on
    one device, so over ranks the stream ids are split with stream_shard.  Negative values or lengths that differ:
    ValueError."""
    import numpy as np
    counts = np.asarray(block_counts, dtype=np.int64).reshape(-1)
    seen = np.asarray(blocks_seen, dtype=np.int64)
    if seen.ndim == 0:
        seen = np.full(counts.shape, int(seen), np.int64)
    seen = seen.reshape(-1)
    if seen.size != counts.size:
        raise ValueError("one blocks_seen value per chunk")
    if np.any(counts < 0) or np.any(seen < 0):
        raise ValueError("blocks_seen and block counts must be >= 0")
    return counts - np.maximum(0, np.minimum(counts, 2 - seen))


def mvdrn_stream_written(blocks_seen, block_counts):
    """Where the chunks of one MvdrMulti.process_streams call start writing (jdsp_mvdrn_streams): emission is
    time-aligned and the only block never written is block 0 of a stream's life, so the chunk of B_c = block_counts[c]
    blocks of a stream that had seen N = blocks_seen[c] blocks writes its blocks from index 1 on when N == 0 and
    B_c > 0, and from index 0 on otherwise.  Both arguments are per-chunk sequences of equal length (a scalar
    blocks_seen stands for all chunks).  Returns numpy int64 [n_chunks].  The layout of the chunks is
    denoise_batch_layout's with chunks for utterances; a live stream lives on one device, so over ranks the stream ids
    are split with stream_shard.  Negative values or lengths that differ: ValueError."""
    import numpy as np
    counts = np.asarray(block_counts, dtype=np.int64).reshape(-1)
    seen = np.asarray(blocks_seen, dtype=np.int64)
    if seen.ndim == 0:
        seen = np.full(counts.shape, int(seen), np.int64)
    seen = seen.reshape(-1)
    if seen.size != counts.size:
        raise ValueError("one blocks_seen value per chunk")
    if np.any(counts < 0) or np.any(seen < 0):
        raise ValueError("blocks_seen and block counts must be >= 0")
    return ((seen == 0) & (counts > 0)).astype(np.int64)


def stftmask_batch_shard(frame_counts, rank, world):
    """Batched fused STFT masking (StftMask.process_batch) over `world` ranks: whole utterances per rank, contiguous,
    balanced by frame count (utterance_shard); an utterance is a stream of its own, so there is no halo and no
    collective.  frame_counts: stftmask_batch_layout's.  Returns (first_utt, n_utt): the rank is given the samples
    utt_sample_first[first_utt] .. utt_sample_first[first_utt + n_utt] and the mask rows
    frame_first[first_utt] .. frame_first[first_utt + n_utt], with the offsets rebased to its first sample.
    The batched analysis and synthesis (Engine.stft_half_batch, Istft.process_batch) share the layout and are split by
    this same function: their spectrum rows take the place of the mask rows.  So is the batched denoiser
    (Denoiser.process_batch): pass its block counts, and rebase denoise_batch_layout's offsets the same way."""
    return utterance_shard([int(f) for f in frame_counts], rank, world)


def fastconv_shard_blocks(n_blocks, hist_blocks, rank, world):
    """Input blocks a rank must be given to produce its share of an overlap-save stream.
    The stream of n_blocks input blocks emits n_blocks - hist_blocks output blocks (the first
    hist_blocks inputs only prime the history); emitted block e is input block e + hist_blocks.
    Returns (first_input_block, n_input_blocks, first_emitted, n_emitted): the rank reads
    hist_blocks halo blocks in front of its own."""
    n_out = max(n_blocks - hist_blocks, 0)
    e0, cnt = split_even(n_out, rank, world)
    if cnt == 0:
        return e0, 0, e0, 0
    return e0, cnt + hist_blocks, e0, cnt


def fastconv_sharded(conv, pcm, n_blocks, rank, world):
    """One rank's emitted blocks of conv applied to the whole stream `pcm` (int16 tensor/array the
    rank can slice: only its own blocks plus the halo are touched).  [n_filters, n_emitted*block]."""
    first_in, n_in, e0, cnt = fastconv_shard_blocks(n_blocks, conv.hist_blocks, rank, world)
    if cnt == 0:
        return None
    conv.set_position(first_in)
    out = conv.process(pcm[first_in * conv.block:(first_in + n_in) * conv.block])
    # position first_in >= hist_blocks: every fed block emits; the first hist_blocks of them saw a silent history
    drop = out.shape[1] - cnt * conv.block
    return out[:, drop:]


def utterance_batch_shard(utt_first, rank, world):
    """GMM scoring / HMM recursion over a batch of utterances (jdsp_gmm_score_dev, jdsp_hmm_viterbi_dev):
    whole utterances per rank, balanced by vector count; no halo, no collective on the data path.
    utt_first: the n_utts + 1 offsets of the whole batch (host sequence).  Returns
    (first_utt, n_utt, vec_lo, vec_hi, local_first): this rank scores vectors [vec_lo, vec_hi) with the
    offsets local_first (rebased to 0); its rows of the [n_utts, n_classes] result are
    [first_utt, first_utt + n_utt).  all_gather_rows() assembles the full table if every rank wants it."""
    lens = [int(utt_first[u + 1]) - int(utt_first[u]) for u in range(len(utt_first) - 1)]
    first_utt, n_utt = utterance_shard(lens, rank, world)
    lo = int(utt_first[first_utt])
    hi = int(utt_first[first_utt + n_utt])
    local_first = [int(utt_first[first_utt + k]) - lo for k in range(n_utt + 1)]
    return first_utt, n_utt, lo, hi, local_first


def mfcc_utterance_shard(utt_sample_first, win_len, hop, rank, world):
    """MFCC over a batch of utterances packed back to back (BASELINE config 4: "10 000-utterance batch sharded across
    1/2/4/8 GPUs"): whole utterances per rank, contiguous, balanced by FRAME count; no halo (an utterance is framed on
    its own, MFCCFeatureExtraction_auto_version1.cpp:68-101 opens one file per utterance), no data-path collective.
    utt_sample_first: the n_utts + 1 sample offsets of the whole batch (host sequence).
    Returns (first_utt, n_utt, sample_lo, sample_hi, frame_lo, frame_hi, local_starts): the rank is given samples
    [sample_lo, sample_hi), computes frames [frame_lo, frame_hi) of the batch's frame list, and local_starts (a numpy
    int64 array) are its frames' first samples relative to sample_lo -- what jdsp_mfcc_frames_dev takes as frame_start."""
    import numpy as np
    offs = np.asarray(utt_sample_first, dtype=np.int64)
    lens = offs[1:] - offs[:-1]
    nf = np.where(lens >= win_len, (lens - win_len) // hop + 1, 0)
    first_utt, n_utt = utterance_shard([int(v) for v in nf], rank, world)
    frame_first = np.concatenate([[0], np.cumsum(nf)])
    lo, hi = int(offs[first_utt]), int(offs[first_utt + n_utt])
    starts = [offs[u] - lo + hop * np.arange(nf[u], dtype=np.int64) for u in range(first_utt, first_utt + n_utt)]
    local_starts = np.concatenate(starts) if starts else np.zeros(0, np.int64)
    return first_utt, n_utt, lo, hi, int(frame_first[first_utt]), int(frame_first[first_utt + n_utt]), local_starts
