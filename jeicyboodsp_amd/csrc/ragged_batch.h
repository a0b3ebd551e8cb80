// ragged_batch.h -- the utterance walk of the kernels that take a batch of ragged utterances in one launch:
// stftmask_batch_kernel (stftmask_kernels.hip), istft_batch_kernel (istft_kernels.hip), stft_half_batch_kernel
// (stft_kernels.hip) and, with blocks for frames, vad_flags_batch_kernel, denoise_batch_kernel and
// denoise_redo_f64_batch_kernel (denoise_kernels.hip).  The host half, the check of the offset arrays before they reach
// the device, is ragged_layout.h.  The layout is the one include/jdsp.h gives for jdsp_stftmask_batch_dev: the waves are planned
// over the CONCATENATED frame axis, global frame j is row j of the spectrum (or mask) tensor, it belongs to utterance u
// with frame_first[u] <= j < frame_first[u + 1] and starts at the sample sample_first[u] + hop (j - frame_first[u]).
// A wave finds the utterance of its first frame by a binary search and then walks from utterance to utterance.  All
// of it is uniform across the wave: it lives in scalar registers and costs neither vector registers nor LDS.
//
// The span walk at the end is that state behind the questions a frame loop asks: RaggedSpan, the above, walked by
// stftmask_batch_kernel, stft_half_batch_kernel, istft_batch_kernel and reverb_analysis (reverb_body.h: the batch and
// live reverberation analysis kernels, with blocks for frames), and StreamSpan, a single stream -- a batch of
// one span [0, n_frames) at sample 0 whose tail is carried by the handle instead of leaving from the registers -- under
// which the same body (istft_run) is istft_run_kernel.  LiveSpan is RaggedSpan over the chunks of live streams: a span
// that starts from a tail carried in memory and ends by writing the tail back (stftmask_live_kernel, istft_live_kernel).
// Bodies: istft_run is all three synthesis kernels; stftmask_ragged is stftmask_batch_kernel and stftmask_live_kernel
// (stftmask_run_kernel keeps a loop of its own); stft_half_batch_kernel has its own.  The host side of the entries that
// launch them, for the two handles with an overlap-add output stream, is the ragged call layer of ola_api.h.
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

// ---- the span walk ---------------------------------------------------------------------------------------------
// The first frame a wave computes when its run starts at j0, r frames overlap and its span starts at frame ub: the
// r - 1 frames before j0 (the halo: added, not emitted), but never a frame of the span before.  For a single stream
// (ub = 0) this is j0 == 0 ? 0 : j0 - (r - 1): the launch keeps run >= r - 1 (plan_ola_run), so a run that does not
// start at 0 starts at r - 1 or later and only j0 = 0 takes the first branch.
__device__ __forceinline__ long span_halo_first(long j0, long ub, int r) { return j0 - ub < r - 1 ? ub : j0 - (r - 1); }

// begin(j0): at the span of frame j0.  first(j0, r): see above.  at(j): the sample where global frame j of the current
// span starts.  last(j): j is the current span's last frame.  next_inside(j): frame j + 1, or at the span's end a frame
// of the span again (where a prefetch may read when nothing follows).  next(): after the span's last frame j, when
// frame j + 1 exists, into the span that holds it.  StreamSpan has what istft_run asks of a stream: its halo stands in
// front of the loop and its prefetch needs no clamp.
template <int HOP> struct StreamSpan {
    static constexpr bool kBatch = false, kLive = false;
    long n_frames;
    __device__ __forceinline__ explicit StreamSpan(long n) : n_frames(n) {}
    __device__ __forceinline__ void begin(long) {}
    __device__ __forceinline__ long at(long j) const { return j * HOP; }
    __device__ __forceinline__ bool last(long j) const { return j + 1 == n_frames; }
    __device__ __forceinline__ void next() {}
};

template <int HOP> struct RaggedSpan {
    static constexpr bool kBatch = true, kLive = false;
    const long long *sample_first, *frame_first;
    long n_utts, u, ub, ue, base;                                // global frame j of utterance u starts at base + j HOP
    __device__ __forceinline__ RaggedSpan(const long long *sf, const long long *ff, long n)
        : sample_first(sf), frame_first(ff), n_utts(n) {}
    __device__ __forceinline__ void begin(long j0)
    {
        u = ragged_find_utt(frame_first, n_utts, j0);
        ub = uniform_i64(frame_first + u);
        ue = uniform_i64(frame_first + u + 1);
        base = uniform_i64(sample_first + u) - ub * HOP;
    }
    __device__ __forceinline__ long first(long j0, int r) const { return span_halo_first(j0, ub, r); }
    __device__ __forceinline__ long at(long j) const { return base + j * HOP; }
    __device__ __forceinline__ bool last(long j) const { return j + 1 == ue; }
    __device__ __forceinline__ long next_inside(long j) const { return j + 1 == ue ? j : j + 1; }
    __device__ __forceinline__ void next()
    {
        ub = ue;
        ragged_next_utt(frame_first, n_utts, u, ue);
        base = uniform_i64(sample_first + u) - ub * HOP;
    }
};

// RaggedSpan's walk over the chunks of live streams (LiveStreams, jdsp_internal.h: the layout of the carried tails and
// why a launch may read and write them without a race), plus the stream and the parity of the current chunk in scalar
// registers.  It answers what the frame loops of a batch never ask: tail_in(), where the sums come from when the first
// frame a wave computes is the chunk's first (starts_span(js)), and tail_out(), where they go after the chunk's last
// frame.
template <int HOP> struct LiveSpan : RaggedSpan<HOP> {
    static constexpr bool kLive = true;
    const long long *stream_id;                                  // the kernel's own __restrict__ arguments, not the
    const int *parity;                                           // struct's members: scalar loads in the walk too
    LiveStreams live;
    long s;                                                      // the current chunk's stream
    int p;                                                       // ... and the tail it starts from
    __device__ __forceinline__ LiveSpan(const long long *sf, const long long *ff, long n, const long long *ids,
                                        const int *par, const LiveStreams &l)
        : RaggedSpan<HOP>(sf, ff, n), stream_id(ids), parity(par), live(l) {}
    __device__ __forceinline__ void load_stream()
    {
        s = uniform_i64(stream_id + this->u);
        p = __builtin_amdgcn_readfirstlane(parity[s]) & 1;
    }
    __device__ __forceinline__ void begin(long j0)
    {
        RaggedSpan<HOP>::begin(j0);
        load_stream();
    }
    __device__ __forceinline__ void next()
    {
        RaggedSpan<HOP>::next();
        load_stream();
    }
    __device__ __forceinline__ bool starts_span(long js) const { return js == this->ub; }
    __device__ __forceinline__ const float *tail_in() const { return live.tails + ((long)p * live.n_streams + s) * live.n_tail; }
    __device__ __forceinline__ float *tail_out() const { return live.tails + ((long)(p ^ 1) * live.n_streams + s) * live.n_tail; }
};

}  // namespace jdsp
