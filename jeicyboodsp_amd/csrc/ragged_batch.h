// ragged_batch.h -- the utterance walk of the kernels that take a batch of ragged utterances in one launch:
// stftmask_batch_kernel (stftmask_kernels.hip), istft_batch_kernel (istft_kernels.hip), stft_half_batch_kernel
// (stft_kernels.hip) and, with blocks for frames, vad_flags_batch_kernel, denoise_batch_kernel and
// denoise_redo_f64_batch_kernel (denoise_kernels.hip).  The host half, the check of the offset arrays before they reach
// the device, is ragged_layout.h.  The layout is the one include/jdsp.h gives for jdsp_stftmask_batch_dev: the waves are planned
// over the CONCATENATED frame axis, global frame j is row j of the spectrum (or mask) tensor, it belongs to utterance u
// with frame_first[u] <= j < frame_first[u + 1] and starts at the sample sample_first[u] + hop (j - frame_first[u]).
// A wave finds the utterance of its first frame by a binary search and then walks from utterance to utterance.  All
// of it is uniform across the wave: it lives in scalar registers and costs neither vector registers nor LDS.
#pragma once

namespace jdsp {

// an offset every lane read from the same address, pinned to scalar registers
__device__ __forceinline__ long uniform_i64(const long long *p)
{
    const long long v = *p;
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)v);
    const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return (long)(((long long)hi << 32) | lo);
}

// the utterance of frame j: the last u with frame_first[u] <= j (frame_first[0] = 0 <= j < frame_first[n_utts]), which
// skips the empty ones in front of it
__device__ __forceinline__ long ragged_find_utt(const long long *frame_first, long n_utts, long j)
{
    long u = 0, hi = n_utts;
    while (hi - u > 1) {
        const long mid = (u + hi) >> 1;
        if (uniform_i64(frame_first + mid) <= j) u = mid;
        else hi = mid;
    }
    return u;
}

// after the last frame of utterance u (ue = frame_first[u + 1]), when frame ue exists: on to the non-empty utterance
// that holds it, past the empty ones between; ue becomes that utterance's end
__device__ __forceinline__ void ragged_next_utt(const long long *frame_first, long n_utts, long &u, long &ue)
{
    const long nb = ue;
    do {
        u++;
        ue = uniform_i64(frame_first + u + 1);
    } while (ue == nb && u + 1 < n_utts);
}

}  // namespace jdsp
