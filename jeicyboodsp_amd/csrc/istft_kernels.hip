// istft_kernels.hip -- STFT synthesis (gfx950): batched inverse transform of caller-given spectra, synthesis window,
// overlap-add and the (short) cast, as one streaming pass (include/jdsp.h, jdsp_istft_*).
//
// One wave per run of consecutive frames; what happens to a frame once it is computed -- the overlap-add, the gain, the
// stores, the tail, the halo and the run order -- is the stream of ola_stream.h.  Per frame:
//   n = 1024  the real frame comes from ONE 512-point complex inverse through the pre-split of frame_io.h: the rows are
//             made Hermitian first, H[k] = (X[k] + conj X[-k]) / 2 (FULL: X[-k] read back from a natural-order image
//             of the row in the wave's LDS, slot 512 - k; HALF: H[n-k] = conj X[k], the row's lower half
//             through the same image), so a non-Hermitian row gives exactly the real part of its full inverse.
//   n = 512   one 512-point complex inverse of H per frame, real part kept.  Never two frames in one transform: a
//             frame's result must not depend on its neighbour, or on where a call or shard cut falls.
// istft_run_kernel (one stream), istft_batch_kernel (a batch of ragged utterances) and istft_live_kernel (the chunks of
// live streams, whose tails the handle carries) are one body, istft_run, over the three forms of ragged_batch.h's span
// walk.  They share the setup, the frame, the staging and the loop's tail; two things stay forked at compile time
// between the stream and the other two, both for speed: the stream's halo runs unrolled in front of the loop where the
// batch's goes through it with emission off, and the stream skips the row prefetch on its run's last frame.  The live
// form is the batch's with a tail loaded where a chunk starts and stored where it ends.
#include "jdsp_internal.h"
#include "ola_stream.h"
#include "ragged_batch.h"

namespace jdsp {

#ifndef JDSP_ISTFT_RESIDENT
// Waves per SIMD the launch plans for (and __launch_bounds__ asks the compiler for).  Registers and LDS would allow three
// at n = 1024 FULL, but with two the same batch is about 16 % faster (125 against 148 us per 65,536 frames, alternated on
// one box); one per SIMD is faster still on 1024/256 and slower on the half spectrum and on 512-point frames
// (profiles/r04_istft_launch_ab.txt)
#define JDSP_ISTFT_RESIDENT 2
#endif

template <int N> struct IstftSample;
template <> struct IstftSample<1024> { typedef float2 T; };
template <> struct IstftSample<512> { typedef float T; };

// streaming (nontemporal) loads: the spectra are read once
#ifndef JDSP_ISTFT_NT_LOAD
#define JDSP_ISTFT_NT_LOAD 1         // 0: plain loads of the spectra (tools/build_variant.sh A/B)
#endif
__device__ __forceinline__ float2 nt_load(const float2 *p)
{
#if JDSP_ISTFT_NT_LOAD
    const f32x2 v = __builtin_nontemporal_load(reinterpret_cast<const f32x2 *>(p));
    return make_float2(v.x, v.y);
#else
    return *p;
#endif
}

// Spectrum values one lane loads per frame: X[lane + 64 q] for q < kLoads (FULL: the whole row; HALF: bins below n/2,
// the Nyquist bin X[n/2] comes separately)
template <int N, int HALF> struct IstftLoad { static constexpr int kLoads = HALF ? N / 128 : N / 64; };

template <int N, int HALF>
__device__ __forceinline__ void istft_load(const float2 *__restrict__ row, int lane, float2 (&x)[IstftLoad<N, HALF>::kLoads],
                                           float2 &nyq)
{
#pragma unroll
    for (int q = 0; q < IstftLoad<N, HALF>::kLoads; q++) x[q] = nt_load(row + lane + 64 * q);
    if (HALF) nyq = nt_load(row + N / 2);
}

// The row into this wave's image (natural order): slot k = X[k], plus slot n = X[0] (FULL) or slot n/2 = X[n/2]
// (HALF, whose loads stop below n/2).  The image's previous reads must be done (fence before).
template <int N, int HALF>
__device__ __forceinline__ void istft_stage(const float2 (&x)[IstftLoad<N, HALF>::kLoads], float2 nyq, float2 *img,
                                            int lane)
{
#pragma unroll
    for (int q = 0; q < IstftLoad<N, HALF>::kLoads; q++) xchg_st(img, lane + 64 * q, x[q]);
    if (lane == 0) img[HALF ? N / 2 : N] = HALF ? nyq : x[0];
}

// H[k], k = lane + 64 D, from the image:
//   FULL  H[k] = (X[k] + conj X[(n - k) mod n]) / 2 -- a power-of-two scale (exact) of a sum that commutes, so a row
//         that is already Hermitian comes out bit for bit as it went in
//   HALF  H[k] = X[k] for k < n/2, conj X[n - k] above; Im of DC and Nyquist ignored
template <int N, int HALF, int D>
__device__ __forceinline__ float2 istft_bin(const float2 *img, int lane)
{
    constexpr int kHalfRegs = N / 128;                       // registers below n/2
    if constexpr (HALF) {
        const float2 x = D < kHalfRegs ? xchg_ld(img, lane + 64 * D) : xchg_ld(img, N - lane - 64 * D);
        const bool real = lane == 0 && (D == 0 || D == kHalfRegs);
        return make_float2(x.x, real ? 0.f : (D < kHalfRegs ? x.y : -x.y));
    } else {
        const float2 x = xchg_ld(img, lane + 64 * D), m = xchg_ld(img, N - lane - 64 * D);
        return make_float2(0.5f * (x.x + m.x), 0.5f * (x.y - m.y));
    }
}

// One frame from the staged image: y[d] = w_s / n * (real inverse of H) at the lane's samples of register d.
// `scratch`: the transform's kWaveLdsComplex elements (not the image).
template <int N, int HALF>
__device__ __forceinline__ void istft_frame(const float2 *img, float2 *scratch, int lane, const WaveTwiddles &tw,
                                            const SplitTwiddles &sw, const typename IstftSample<N>::T (&ws)[8],
                                            typename IstftSample<N>::T (&y)[8])
{
    float2 v[8];
    if constexpr (N == 1024) {
        // Z'[m] from H[m], H[m + 512] (frame_io.h), m = lane + 64 d
#define JDSP_ISTFT_Z(D) v[D] = presplit_inv_reg(istft_bin<N, HALF, D>(img, lane), istft_bin<N, HALF, D + 8>(img, lane), sw.w[D])
        JDSP_ISTFT_Z(0); JDSP_ISTFT_Z(1); JDSP_ISTFT_Z(2); JDSP_ISTFT_Z(3);
        JDSP_ISTFT_Z(4); JDSP_ISTFT_Z(5); JDSP_ISTFT_Z(6); JDSP_ISTFT_Z(7);
#undef JDSP_ISTFT_Z
    } else {
#define JDSP_ISTFT_H(D) v[D] = istft_bin<N, HALF, D>(img, lane)
        JDSP_ISTFT_H(0); JDSP_ISTFT_H(1); JDSP_ISTFT_H(2); JDSP_ISTFT_H(3);
        JDSP_ISTFT_H(4); JDSP_ISTFT_H(5); JDSP_ISTFT_H(6); JDSP_ISTFT_H(7);
#undef JDSP_ISTFT_H
    }
    wave_fft512<true>(v, scratch, lane, tw);
    wave_lds_fence();                                            // the transform's last exchange reads are done
#pragma unroll
    for (int d = 0; d < 8; d++) {
        if constexpr (N == 1024) y[d] = ola_mul(v[d], ws[d]);
        else y[d] = v[d].x * ws[d];
    }
}

// A single stream (jdsp_istft_*) or a batch of independent streams, the utterances, in one launch (jdsp_istft_batch_*):
// the waves are planned over the frame axis (of the batch the concatenated one), global frame j is spectrum row j, and
// the span walk of ragged_batch.h says where its samples go, where a wave's halo stops and where a span ends.
struct IstftArgs {
    const float2 *spec;
    long pitch, n_frames;     // n_frames: of all utterances
    long n_utts;              // a batch
    const float *ws;          // [n]   w_s[i] / n, natural order
    const float *g;           // [hop] WOLA gain (1 without an analysis window)
    short *out;               // may be NULL
    float *out_f32;           // may be NULL
    int run;
    const float *tail_in;     // a stream: [n - hop] partial sums of the samples after the last emitted one
    float *tail_out;
};
// the same under the name the batch kernels' symbols carry (profiles and tools find a kernel by its symbol)
struct IstftBatchArgs : IstftArgs {};

// One wave's run.  The rows are prefetched one frame ahead, on across utterances (a row belongs to no span).  A
// stream's tail is read by the wave that starts at frame 0 and written by the one that owns the call's last frame
// (OlaAcc::shift); after an utterance's last frame the tail leaves from the registers (OlaAcc::emit_tail) and the sums restart: no tail in
// memory, no flush launch, and the handle's own tail is neither read nor written.
template <int N, int HALF, int R, class Span>
__device__ __forceinline__ void istft_run(const IstftArgs &a, const float2 *__restrict__ table, Span span)
{
    typedef typename IstftSample<N>::T T;
    constexpr int HR = 8 / R;                                   // registers per hop
    constexpr int kL = IstftLoad<N, HALF>::kLoads;
    // the row's natural-order image, then the transform's scratch: 12.9 KB per wave at n = 1024 FULL (three waves
    // per SIMD, what its registers allow), 8.8 KB otherwise
    constexpr int kImg = HALF ? N / 2 + 1 : N + 1;
    __shared__ __attribute__((aligned(16))) float2 lds[kImg + 1 + kWaveLdsComplex];
    float2 *const img = lds;
    float2 *const scratch = lds + ((kImg + 1) & ~1);
    const int lane = threadIdx.x;
    long j0, j1;
    if (!ola_run_range(a.run, a.n_frames, j0, j1)) return;
    span.begin(j0);

    WaveTwiddles tw;
    load_wave_twiddles(tw, table, lane);
    SplitTwiddles sw;
    if (N == 1024) load_split_twiddles(sw, table, lane);
    T ws[8];
    const T *ws_t = reinterpret_cast<const T *>(a.ws);
#pragma unroll
    for (int d = 0; d < 8; d++) ws[d] = ws_t[lane + 64 * d];

    OlaAcc<T, HR> ola;
    ola.init(a.g, lane);
    T y[8], o[HR];
    float2 nx[kL], nnyq = make_float2(0.f, 0.f);

    // The halo: transformed and added, not emitted.  A batch's is 0..R-1 frames long and goes through the loop below with
    // the stores off.  A stream's is R - 1 frames wherever j0 > 0 and runs here, in front of the loop, unrolled, with no
    // prefetch: through the loop the stream's half-spectrum leg was 1.2-2 % slower than before in every round measured
    // (profiles/r17_one_frame_walk.txt), so the stream keeps this second copy of the frame.
    long js = j0;
    if constexpr (Span::kBatch) {
        js = span.first(j0, R);
        // live streams: a halo that stops at the chunk's first frame starts from the stream's carried tail
        if constexpr (Span::kLive) {
            if (span.starts_span(js)) ola.load_tail(span.tail_in(), lane);
        }
    } else if (j0 == 0) {
        ola.load_tail(a.tail_in, lane);
    } else {
#pragma unroll
        for (int k = R - 1; k >= 1; k--) {
            istft_load<N, HALF>(a.spec + (j0 - k) * a.pitch, lane, nx, nnyq);
            istft_stage<N, HALF>(nx, nnyq, img, lane);
            wave_lds_fence();
            istft_frame<N, HALF>(img, scratch, lane, tw, sw, ws, y);
            ola.add(y, o);
            ola.shift(false, nullptr, lane);
        }
    }
    istft_load<N, HALF>(a.spec + js * a.pitch, lane, nx, nnyq);
    istft_stage<N, HALF>(nx, nnyq, img, lane);
    wave_lds_fence();
    for (long j = js; j < j1; j++) {
        // the next row, staged one frame from now.  A stream has none on its run's last frame (with the halo in the
        // loop and this load unguarded its full-spectrum legs were 4-5 % slower: one more row per run, in a kernel its
        // reads bound); a batch loads on, unguarded, at a clamped row (past the wave's run it is never used)
        const bool more = Span::kBatch || j + 1 < j1;
        const long jn = Span::kBatch && j + 1 >= a.n_frames ? a.n_frames - 1 : j + 1;
        if (more) istft_load<N, HALF>(a.spec + jn * a.pitch, lane, nx, nnyq);
        istft_frame<N, HALF>(img, scratch, lane, tw, sw, ws, y);
        ola.add(y, o);
        // stage the prefetched row before this frame's stores: vmcnt counts loads and stores in issue order, and a wait
        // for the row at the top of the next iteration would also wait for these stores.  The image's reads are behind
        // istft_frame's fence.
        if (more) istft_stage<N, HALF>(nx, nnyq, img, lane);
        __builtin_amdgcn_sched_barrier(0);
        if (!Span::kBatch || j >= j0) ola.emit(o, a.out, a.out_f32, span.at(j), lane);
        const bool last = span.last(j);
        if constexpr (Span::kLive) {
            // a chunk's last frame leaves the stream's new tail in memory (the other of its two, ragged_batch.h), and
            // the chunk that follows in the run starts from its own stream's
            ola.shift(last, span.tail_out(), lane);
            if (last && j + 1 < j1) {
                span.next();
                ola.load_tail(span.tail_in(), lane);
            }
        } else {
            ola.shift(!Span::kBatch && last, a.tail_out, lane);
            if (Span::kBatch && last) {
                // a halo frame is never an utterance's last (j0 lies in the halo's utterance), so the wave that emits
                // the last frame emits the tail
                ola.emit_tail(a.out, a.out_f32, span.at(j + 1), lane);
                ola.restart();
                if (j + 1 < j1) span.next();                     // frame j + 1 exists, so a non-empty utterance follows
            }
        }
        wave_lds_fence();                                        // the staged row before the next frame reads it
    }
}

template <int N, int HALF, int R>
__global__ __launch_bounds__(64, JDSP_ISTFT_RESIDENT) void istft_run_kernel(IstftArgs a, const float2 *__restrict__ table)
{
    istft_run<N, HALF, R>(a, table, StreamSpan<N / R>(a.n_frames));
}

template <int N, int HALF, int R>
__global__ __launch_bounds__(64, JDSP_ISTFT_RESIDENT) void istft_batch_kernel(
    IstftBatchArgs a, const float2 *__restrict__ table, const long long *__restrict__ sample_first,
    const long long *__restrict__ frame_first)
{
    istft_run<N, HALF, R>(a, table, RaggedSpan<N / R>(sample_first, frame_first, a.n_utts));
}

// the chunks of live streams (jdsp_istft_streams_*): the batch's walk with tails carried in the handle
template <int N, int HALF, int R>
__global__ __launch_bounds__(64, JDSP_ISTFT_RESIDENT) void istft_live_kernel(
    IstftBatchArgs a, const float2 *__restrict__ table, const long long *__restrict__ sample_first,
    const long long *__restrict__ frame_first, const long long *__restrict__ stream_id, const int *__restrict__ parity,
    LiveStreams live)
{
    istft_run<N, HALF, R>(a, table, LiveSpan<N / R>(sample_first, frame_first, a.n_utts, stream_id, parity, live));
}

// ---- the state of live streams (jdsp::OlaStreams, ola_api.h; the layout: LiveStreams, jdsp_internal.h) -----------
// flush of the listed streams: one workgroup per stream writes its n_tail samples, g[t mod hop] * s[t] and the same
// cast, at sample_first[i] onwards and zeroes the tail behind it -- the stream is fresh again, its parity as it is.
// Both outputs NULL: the reset of the listed streams.
__global__ __launch_bounds__(256) void ola_streams_flush_kernel(LiveStreams live, const long long *__restrict__ sample_first,
                                                                const float *__restrict__ g, int hop,
                                                                short *__restrict__ out, float *__restrict__ out_f32)
{
    const long s = uniform_i64(live.stream_id + blockIdx.x);
    const int p = __builtin_amdgcn_readfirstlane(live.parity[s]) & 1;
    float *tail = live.tails + ((long)p * live.n_streams + s) * live.n_tail;
    const long at = out || out_f32 ? uniform_i64(sample_first + blockIdx.x) : 0;
    for (int i = threadIdx.x; i < live.n_tail; i += blockDim.x) {
        const float o = g[i % hop] * tail[i];
        if (out) out[at + i] = (short)cast_i16_bits(o);
        if (out_f32) out_f32[at + i] = o;
        tail[i] = 0.0f;
    }
}

// after a launch over chunks: the streams that were given frames start their next chunk from the tail it wrote
__global__ __launch_bounds__(256) void ola_streams_commit_kernel(const long long *__restrict__ stream_id,
                                                                 const long long *__restrict__ frame_first, long n_chunks,
                                                                 int *__restrict__ parity)
{
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    if (frame_first[c + 1] > frame_first[c]) parity[stream_id[c]] ^= 1;    // ids are distinct within a call
}

// flush: the n - hop samples still in the tail, g[t mod hop] * s[t], then the same cast
__global__ __launch_bounds__(256) void istft_flush_kernel(const float *__restrict__ tail, const float *__restrict__ g,
                                                          int n_tail, int hop, short *__restrict__ out,
                                                          float *__restrict__ out_f32)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tail) return;
    const float o = g[i % hop] * tail[i];
    if (out) out[i] = (short)cast_i16_bits(o);
    if (out_f32) out_f32[i] = o;
}

// sample_first == NULL: a single stream; live != NULL: the chunks of live streams
template <int N, int HALF, int R>
static void launch_one(hipStream_t s, long grid, const IstftArgs &a, const float2 *table, const long long *sample_first,
                       const long long *frame_first, const LiveStreams *live)
{
    if (live)
        hipLaunchKernelGGL((istft_live_kernel<N, HALF, R>), dim3((unsigned)grid), dim3(64), 0, s, IstftBatchArgs{a}, table,
                           sample_first, frame_first, live->stream_id, live->parity, *live);
    else if (sample_first)
        hipLaunchKernelGGL((istft_batch_kernel<N, HALF, R>), dim3((unsigned)grid), dim3(64), 0, s, IstftBatchArgs{a}, table,
                           sample_first, frame_first);
    else
        hipLaunchKernelGGL((istft_run_kernel<N, HALF, R>), dim3((unsigned)grid), dim3(64), 0, s, a, table);
}

template <int N, int HALF>
static void launch_r(hipStream_t s, int r, long grid, const IstftArgs &a, const float2 *table,
                     const long long *sample_first, const long long *frame_first, const LiveStreams *live)
{
    if (r == 1) launch_one<N, HALF, 1>(s, grid, a, table, sample_first, frame_first, live);
    else if (r == 2) launch_one<N, HALF, 2>(s, grid, a, table, sample_first, frame_first, live);
    else launch_one<N, HALF, 4>(s, grid, a, table, sample_first, frame_first, live);
}

static int launch_any(hipStream_t s, int n_cu, int n_fft, int hop, int half, IstftArgs a, const float2 *table,
                      int run_opt, const long long *sample_first, const long long *frame_first,
                      const LiveStreams *live)
{
    const int r = n_fft / hop;
    const OlaRunPlan p = plan_ola_run(n_cu, JDSP_ISTFT_RESIDENT, r, a.n_frames, run_opt);
    a.run = (int)p.run;
    if (n_fft == 1024) {
        if (half) launch_r<1024, 1>(s, r, p.grid, a, table, sample_first, frame_first, live);
        else launch_r<1024, 0>(s, r, p.grid, a, table, sample_first, frame_first, live);
    } else {
        if (half) launch_r<512, 1>(s, r, p.grid, a, table, sample_first, frame_first, live);
        else launch_r<512, 0>(s, r, p.grid, a, table, sample_first, frame_first, live);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_istft(hipStream_t s, int n_cu, int n_fft, int hop, int half, const float2 *spec, long pitch, long n_frames,
                 const float *ws, const float *g, const float *tail_in, float *tail_out, short *out, float *out_f32,
                 const float2 *table, int run_opt)
{
    if (n_frames <= 0) return 0;
    const IstftArgs a = {spec, pitch, n_frames, 1, ws, g, out, out_f32, 0, tail_in, tail_out};
    return launch_any(s, n_cu, n_fft, hop, half, a, table, run_opt, nullptr, nullptr, nullptr);
}

int launch_istft_flush(hipStream_t s, const float *tail, const float *g, int n_tail, int hop, short *out, float *out_f32)
{
    if (n_tail <= 0 || (!out && !out_f32)) return 0;
    hipLaunchKernelGGL(istft_flush_kernel, dim3((unsigned)((n_tail + 255) / 256)), dim3(256), 0, s, tail, g, n_tail, hop,
                       out, out_f32);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_istft_ragged(hipStream_t s, int n_cu, int n_fft, int hop, int half, const float2 *spec, long pitch,
                        long n_frames_total, const long long *sample_first, const long long *frame_first, long n_spans,
                        const LiveStreams *live, const float *ws, const float *g, short *out, float *out_f32,
                        const float2 *table, int run_opt)
{
    if (n_frames_total <= 0 || n_spans <= 0) return 0;
    const IstftArgs a = {spec, pitch, n_frames_total, n_spans, ws, g, out, out_f32, 0, nullptr, nullptr};
    return launch_any(s, n_cu, n_fft, hop, half, a, table, run_opt, sample_first, frame_first, live);
}

int launch_ola_streams_flush(hipStream_t s, const LiveStreams &live, long n_ids, const long long *sample_first,
                             const float *g, int hop, short *out, float *out_f32)
{
    if (n_ids <= 0 || live.n_tail <= 0) return 0;
    hipLaunchKernelGGL(ola_streams_flush_kernel, dim3((unsigned)n_ids), dim3(256), 0, s, live, sample_first, g, hop, out,
                       out_f32);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_ola_streams_commit(hipStream_t s, const long long *stream_id, const long long *frame_first, long n_chunks,
                              int *parity)
{
    if (n_chunks <= 0) return 0;
    hipLaunchKernelGGL(ola_streams_commit_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, s, stream_id,
                       frame_first, n_chunks, parity);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
