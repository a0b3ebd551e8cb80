// ola_stream.h -- the overlap-add output stream of the streaming synthesis kernels: istft_run (istft_kernels.hip, the
// body under istft_run_kernel and istft_batch_kernel) and stftmask_run_kernel / stftmask_batch_kernel
// (stftmask_kernels.hip) compute a windowed frame in their own way and hand it to the one stream defined here.  Its host side, what a handle carries from call to
// call, is jdsp::OlaStream (ola_api.h).
//
// One wave per run of consecutive frames (persistent: the launch picks the run so that the batch is about one round of
// resident waves, in XCD-aware order, as denoise_run_kernel).  Lane l holds frame samples 2 l + 128 d, +1 (n = 1024, one
// float2 per register) or l + 64 d (n = 512, one float per register), d < 8, so a hop of n / R is HR = 8 / R registers in
// both cases and the overlap-add is a register shift: after frame f, registers 0..HR-1 are final (emitted) and the rest
// move down.  Every output sample is the FP32 sum of its frames in ascending order, starting from 0 (or from the tail),
// then one multiply by the gain g, then the cast -- the same operations whatever the call cuts or the launch geometry,
// so results are bit-identical across both.  A wave whose run starts at frame j0 > 0 recomputes the R - 1 frames
// before it (the halo: added and shifted, not emitted; in a batch it stops at the utterance's first frame,
// ragged_batch.h).  A single stream: only the wave with j0 = 0 reads the tail carried in the handle, and the wave that owns
// the call's last frame writes the new tail (ping-pong buffers: another wave may still be reading the old one).  A batch (RaggedSpan) feeds many independent streams from one launch: a stream that ends inside a
// wave's run leaves through emit_tail and the next starts after restart, with no tail in memory at all.  Live streams
// (LiveSpan; stftmask_live_kernel, istft_live_kernel) are the batch with carried tails: load_tail wherever a wave's first
// computed frame is a chunk's first, shift(true, ...) to the stream's OTHER tail buffer after the chunk's last frame
// (LiveStreams, jdsp_internal.h).
#pragma once
#include "frame_io.h"

namespace jdsp {

#ifndef JDSP_ISTFT_MIN_RUN_PER_HALO
#define JDSP_ISTFT_MIN_RUN_PER_HALO 4   // shortest run, in halo frames (plan_ola_run)
#endif

// The launch of n_frames frames with R = r frames overlapping: frames per wave and a grid of whole rounds of the eight
// XCDs.  One round of resident waves (`resident` per SIMD, the kernel's own __launch_bounds__), but never a run
// shorter than JDSP_ISTFT_MIN_RUN_PER_HALO (R - 1) frames: the R - 1 halo frames a wave recomputes (extra reads and
// transforms) are then at most 1 / JDSP_ISTFT_MIN_RUN_PER_HALO of its run whatever R is; a longer minimum leaves fewer
// waves for small batches.  run_opt > 0 is the handles' "frames_per_wave" option, kept >= R - 1: the halo must not
// reach below frame 0.
struct OlaRunPlan { long run, grid; };
inline OlaRunPlan plan_ola_run(int n_cu, int resident, int r, long n_frames, int run_opt)
{
    const long slots = (long)(n_cu > 0 ? n_cu : 256) * 4 * resident;
    long run = (n_frames + slots - 1) / slots;
    const long min_run = r > 1 ? (long)JDSP_ISTFT_MIN_RUN_PER_HALO * (r - 1) : 1;
    if (run < min_run) run = min_run;
    if (run_opt > 0) run = run_opt < r - 1 ? r - 1 : run_opt;
    const long waves = (n_frames + run - 1) / run;
    return {run, (waves + 7) / 8 * 8};
}

// This wave's frames [j0, j1) of the plan above, in XCD-aware run order (speed only); false: none
__device__ __forceinline__ bool ola_run_range(int run, long n_frames, long &j0, long &j1)
{
    const long per_xcd = (gridDim.x + 7) >> 3;
    j0 = ((long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3)) * run;
    j1 = j0 + run < n_frames ? j0 + run : n_frames;
    return j0 < n_frames;
}

__device__ __forceinline__ float2 ola_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float ola_add(float a, float b) { return a + b; }
__device__ __forceinline__ float2 ola_mul(float2 a, float2 b) { return make_float2(a.x * b.x, a.y * b.y); }
__device__ __forceinline__ float ola_mul(float a, float b) { return a * b; }
template <class T> __device__ __forceinline__ T ola_zero();
template <> __device__ __forceinline__ float2 ola_zero<float2>() { return make_float2(0.f, 0.f); }
template <> __device__ __forceinline__ float ola_zero<float>() { return 0.f; }

// streaming (nontemporal) stores: the outputs are written once.  One register is two samples (float2 lanes: a dword
// of int16) or one (float lanes: a halfword)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void nt_store(float2 v, float2 *p)
{
    f32x2 w = {v.x, v.y};
    __builtin_nontemporal_store(w, reinterpret_cast<f32x2 *>(p));
}
__device__ __forceinline__ void nt_store(float v, float *p) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void nt_store_i16(float2 v, short *p)
{
    __builtin_nontemporal_store(cast_i16x2_bits(v.x, v.y), reinterpret_cast<unsigned int *>(p));
}
__device__ __forceinline__ void nt_store_i16(float v, short *p)
{
    __builtin_nontemporal_store((unsigned short)cast_i16_bits(v), reinterpret_cast<unsigned short *>(p));
}

// One lane's share of the stream: T = float2 (n = 1024) or float (n = 512), HR registers per hop.  Per frame:
// add(y, o), then emit(o, ...) unless the frame is halo, then shift(...); the kernel stages its prefetched inputs
// between add and emit.
template <class T, int HR> struct OlaAcc {
    static constexpr int kPer = sizeof(T) / sizeof(float);      // samples per register
    T acc[8], g[HR];

    // g_in: [hop] emission gain; the sums start from 0
    __device__ __forceinline__ void init(const float *g_in, int lane)
    {
        const T *g_t = reinterpret_cast<const T *>(g_in);
#pragma unroll
        for (int d = 0; d < HR; d++) g[d] = g_t[lane + 64 * d];
#pragma unroll
        for (int d = 0; d < 8; d++) acc[d] = ola_zero<T>();
    }
    // ... or, in the wave that starts at frame 0 alone, from the handle's tail: [n - hop] partial sums of the samples
    // after the last emitted one
    __device__ __forceinline__ void load_tail(const float *tail_in, int lane)
    {
        const T *tl = reinterpret_cast<const T *>(tail_in);
#pragma unroll
        for (int d = 0; d < 8 - HR; d++) acc[d] = tl[lane + 64 * d];
    }
    // the frame into the sums; o: the hop that is now final, times the gain
    __device__ __forceinline__ void add(const T (&y)[8], T (&o)[HR])
    {
#pragma unroll
        for (int d = 0; d < 8; d++) acc[d] = ola_add(acc[d], y[d]);
#pragma unroll
        for (int d = 0; d < HR; d++) o[d] = ola_mul(g[d], acc[d]);
    }
    // o to the stream's sample `at` onwards; out and out_f32 may each be NULL
    __device__ __forceinline__ void emit(const T (&o)[HR], short *out, float *out_f32, long at, int lane) const
    {
        if (out) {
#pragma unroll
            for (int d = 0; d < HR; d++) nt_store_i16(o[d], out + at + kPer * (lane + 64 * d));
        }
        if (out_f32) {
            T *dst = reinterpret_cast<T *>(out_f32 + at) + lane;
#pragma unroll
            for (int d = 0; d < HR; d++) nt_store(o[d], dst + 64 * d);
        }
    }
    // one hop down; after the call's last frame what is left is the new tail
    __device__ __forceinline__ void shift(bool last_frame, float *tail_out, int lane)
    {
#pragma unroll
        for (int d = 0; d < 8; d++) acc[d] = d + HR < 8 ? acc[d + HR] : ola_zero<T>();
        if (last_frame) {
            T *tl = reinterpret_cast<T *>(tail_out);
#pragma unroll
            for (int d = 0; d < 8 - HR; d++) tl[lane + 64 * d] = acc[d];
        }
    }
    // A stream that ends inside the wave (a batch of independent streams, the *_batch_kernel): after the shift of
    // its last frame, the n - hop samples left go out from the registers, to the stream's sample `at` onwards -- the
    // flush's g[t mod hop] * s[t] (a hop is HR registers, so register d takes g[d % HR]) and emit's casts and stores
    __device__ __forceinline__ void emit_tail(short *out, float *out_f32, long at, int lane) const
    {
        if (out) {
#pragma unroll
            for (int d = 0; d < 8 - HR; d++) nt_store_i16(ola_mul(g[d % HR], acc[d]), out + at + kPer * (lane + 64 * d));
        }
        if (out_f32) {
            T *dst = reinterpret_cast<T *>(out_f32 + at) + lane;
#pragma unroll
            for (int d = 0; d < 8 - HR; d++) nt_store(ola_mul(g[d % HR], acc[d]), dst + 64 * d);
        }
    }
    // ... and the next stream's sums start from 0, the gain stays
    __device__ __forceinline__ void restart()
    {
#pragma unroll
        for (int d = 0; d < 8; d++) acc[d] = ola_zero<T>();
    }
};

}  // namespace jdsp
