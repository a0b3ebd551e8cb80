// mvdrn_live_kernels.hip -- the n-microphone MVDR beamformer (mvdrn_kernels.hip) over the chunks of LIVE streams: each
// chunk continues a stream whose covariance, last block and quiet bit live on the device (include/jdsp.h,
// jdsp_mvdrn_streams_dev; the state and the workspace: MvnLive, jdsp_internal.h; the layout: ragged_batch.h with chunks
// for utterances).  1024-point frames only.
//
// A delivery is six launches, whatever the number of chunks:
//   mvnl_vad_kernel             the energy test on microphone 0 per block of the concatenated axis (mvnb_vad_kernel's)
//   mvnl_plan_kernel            one wave per chunk: its estimation frames ("events") as a list, and per block the number
//                               of them at or before it.  Block b of a chunk is an event iff it and the block before it
//                               are quiet; before block 0 stands the stream's last block, whose quiet bit is carried
//   mvnl_event_spectra_kernel   X_m[k] of every event's frame; an event at block 0 takes its first half from the carried
//                               block of every microphone
//   mvnl_update_kernel          one wave per chunk and eight bins: the stream's covariance, walked one event at a time
//                               (mvdrn_walk_body.h with `lead`: row 0 of the chunk solves the matrix carried in), written
//                               back in place
//   mvnl_apply_kernel           one wave per block: the beamformed frame (mvdrn_frame_body.h), time-aligned
//   mvnl_state_kernel           one wave per chunk: the chunk's last block of every microphone, the count, the carried word
// The arithmetic is the stream's and the batch's, written once (mvdrn_common.h and the two body fragments); what is
// written here is what a live stream has of its own: where the block before block 0 comes from and where the matrix
// comes from and goes.
//
// The carried word of a stream: bit 0, its last block was quiet; above it the estimation frames of its life, saturated at
// 8.  The count is there for loading 0 alone: a sum of fewer than n_mics outer products is singular by rank, and what
// the elimination makes of it is its own rounding error -- an exact zero pivot in one bin, a tiny one in the next, so
// that which samples come out finite is chance (the stream and batch kernels leave it at that).  Here the rule is
// spelled out: at loading 0 the weights of a version with fewer than n_mics estimation frames behind it are NaN, the
// block's samples are non-finite, and they are so wherever the stream is cut.
//
// The plan is per chunk and not the batch's tiled prefix sum over the concatenated axis: a chunk's update is one wave
// that walks its events in order anyway, so a wave that counts its blocks 64 at a time is never the longer of the two,
// the list and the rows need no global offsets (chunk c has at most B_c events: they fit at block_first[c]), and the
// chunk's first block needs the stream's bit, which only the chunk's wave knows where to find.
//
// No parity.  The covariance of (stream, eight bins) is read and written by one wave of one launch and by nothing else of
// the delivery.  The carried blocks, seen[] and word[] are read by the launches above and written by
// mvnl_state_kernel alone, which reads them from the caller's PCM and the VAD's code behind every reader: no launch both
// reads and writes them, so stream order is all the ordering there is.
#include "frame_io.h"
#include "jdsp_internal.h"
#include "mvdrn_common.h"
#include "ragged_batch.h"

namespace jdsp {

typedef u32x4 u32x4_span __attribute__((aligned(4)));      // sample_first is even: a lane's 16 bytes are 4-byte aligned

// ---- 1. VAD: code[j] = voice, one wave per block ---------------------------------------------------------------------
// mvnb_vad_kernel's decision (vad_flags_kernel's energy test without the zero-crossing count), integer from the cast on
__global__ __launch_bounds__(64) void mvnl_vad_kernel(const short *__restrict__ pcm,
                                                      const long long *__restrict__ sample_first,
                                                      const long long *__restrict__ block_first, long n_chunks,
                                                      long n_blocks, const double *__restrict__ w_vad,
                                                      unsigned char *__restrict__ code, unsigned char *__restrict__ flags)
{
    const int lane = threadIdx.x;
    const long j = blockIdx.x;
    if (j >= n_blocks) return;
    const long c = ragged_find_utt(block_first, n_chunks, j);
    const long at = uniform_i64(sample_first + c) + (j - uniform_i64(block_first + c)) * 512;
    const u32x4 img = reinterpret_cast<const u32x4_span *>(pcm + at)[lane];
    int x[8];
    x[0] = (short)(img.x & 0xffffu); x[1] = (int)img.x >> 16;
    x[2] = (short)(img.y & 0xffffu); x[3] = (int)img.y >> 16;
    x[4] = (short)(img.z & 0xffffu); x[5] = (int)img.z >> 16;
    x[6] = (short)(img.w & 0xffffu); x[7] = (int)img.w >> 16;
    unsigned int qa = 0, qb = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int sv = (int)((double)x[k] * w_vad[8 * lane + k]);  // (short)(short * double), in range
        if (k < 4) qa += (unsigned int)__mul24(sv, sv); else qb += (unsigned int)__mul24(sv, sv);
    }
    const unsigned int cap = 1u << 20;
    const unsigned int e = wave_sum_u32((qa < cap ? qa : cap) + (qb < cap ? qb : cap));
    if (lane == 0) {
        const unsigned char v = e > 700u * 128u * 8u ? 1 : 0;
        code[j] = v;
        if (flags) flags[j] = v;
    }
}

// ---- 2. plan: one wave per chunk, 64 blocks a round ------------------------------------------------------------------
// events[block_first[c] + i] = the chunk's i-th event as a block of the chunk; row[j] = events of the chunk at or before
// block j (0: the chunk's lead row, the matrix carried in); ev_n[c] = their number
__global__ __launch_bounds__(64) void mvnl_plan_kernel(const long long *__restrict__ stream_id,
                                                       const long long *__restrict__ block_first,
                                                       const unsigned char *__restrict__ code,
                                                       const int *__restrict__ word, int *__restrict__ row,
                                                       int *__restrict__ events, int *__restrict__ ev_n)
{
    const int lane = threadIdx.x;
    const long c = blockIdx.x;
    const long cb = uniform_i64(block_first + c), n_own = uniform_i64(block_first + c + 1) - cb;
    if (n_own <= 0) {
        if (lane == 0) ev_n[c] = 0;
        return;
    }
    const bool carried = (__builtin_amdgcn_readfirstlane(word[uniform_i64(stream_id + c)]) & 1) != 0;
    int run = 0;
    for (long b0 = 0; b0 < n_own; b0 += 64) {
        const long b = b0 + lane;
        const bool in = b < n_own;
        const bool quiet = in && code[cb + b] == 0;
        const bool before = b == 0 ? carried : (in && code[cb + b - 1] == 0);
        const bool ev = quiet && before;
        const unsigned long long mask = __ballot(ev);
        const int below = __popcll(mask & ((1ull << lane) - 1ull));
        if (ev) events[cb + run + below] = (int)b;
        if (in) row[cb + b] = run + below + (ev ? 1 : 0);
        run += __popcll(mask);
    }
    if (lane == 0) ev_n[c] = run;
}

// ---- 3. the spectra of the estimation frames -------------------------------------------------------------------------
// spec[(e * n_mics + m) * 513 + k] = X_m[k] of the frame [block b - 1, block b], b = events[e], for every slot e of the
// concatenated axis that holds an event of its chunk (e - block_first[c] < ev_n[c]); a slot that holds none is skipped.
// Block -1 of a chunk is the stream's carried block.
__global__ __launch_bounds__(64) void mvnl_event_spectra_kernel(const short *__restrict__ pcm, long chan_stride, int n_mics,
                                                                const long long *__restrict__ stream_id,
                                                                const long long *__restrict__ sample_first,
                                                                const long long *__restrict__ block_first, long n_chunks,
                                                                long n_blocks, const int *__restrict__ events,
                                                                const int *__restrict__ ev_n,
                                                                const short *__restrict__ carried,
                                                                const float2 *__restrict__ table, float2 *__restrict__ spec)
{
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    __shared__ __attribute__((aligned(16))) unsigned int stage[256];
    const int lane = threadIdx.x;
    const long total = n_blocks * n_mics;
    WaveTwiddles tw;
    load_wave_twiddles(tw, table, lane);
    const float2 wsp[2] = {table[kStftSplit + 2 * lane], table[kStftSplit + 2 * lane + 1]};
    for (long w = blockIdx.x; w < total; w += gridDim.x) {
        const long e = w / n_mics;
        const int m = (int)(w % n_mics);
        const long c = ragged_find_utt(block_first, n_chunks, e);
        if (e - uniform_i64(block_first + c) >= __builtin_amdgcn_readfirstlane(ev_n[c])) continue;
        const long b = __builtin_amdgcn_readfirstlane(events[e]);
        const short *cur = pcm + (size_t)m * chan_stride + uniform_i64(sample_first + c) + b * 512;
        const short *before = b > 0 ? cur - 512 : carried + ((size_t)uniform_i64(stream_id + c) * 8 + m) * 512;
        unsigned int raw[8];
        relayout_half(stage, lane, reinterpret_cast<const u32x4_span *>(before)[lane], raw);
        relayout_half(stage, lane, reinterpret_cast<const u32x4_span *>(cur)[lane], raw + 4);
        mvn_event_spectrum(raw, lds, lane, tw, wsp, spec + (size_t)w * kMvnBins);
    }
}

// ---- 4. covariance and weights: (chunk, 8 bins), from the stream's matrix and back -----------------------------------
// The walk and its solve are mvdrn_update_kernel's, the same text (mvdrn_walk_body.h), with lead set: version e0 solves
// the matrix as it came in -- the weights of the chunk's blocks before its first event -- and every event adds a
// version, however many there are.  weights is the table from the chunk's own row base on (block_first[c] + c), so
// version v is its row v - e0.  cov is read and written through one pointer: this wave is its only user.
__global__ __launch_bounds__(64) void mvnl_update_kernel(const float2 *__restrict__ spec, int n_mics,
                                                         const long long *__restrict__ stream_id,
                                                         const long long *__restrict__ block_first,
                                                         const int *__restrict__ ev_n,
                                                         const int *__restrict__ word, double2 *cov,
                                                         const double2 *__restrict__ steer, double loading,
                                                         float2 *__restrict__ weight_table)
{
    const int lane = threadIdx.x, grp = lane >> 3, r = lane & 7;
    const long c = blockIdx.x;
    const long cb = uniform_i64(block_first + c);
    if (uniform_i64(block_first + c + 1) == cb) return;           // a chunk of 0 blocks touches nothing
    const long s = uniform_i64(stream_id + c);
    const int kb = blockIdx.y * 8 + grp;
    const int k = kb < kMvnBins ? kb : kMvnBins - 1;             // a group past the last bin repeats it and stores nothing
    double2 *mine = cov + ((size_t)s * kMvnBins + k) * 64 + 8 * r;
    cd R[8];
#pragma unroll
    for (int i = 0; i < 8; i++) R[i] = cd_of(mine[i]);
    constexpr int n_bins = kMvnBins;
    constexpr double inv_n = 1.0 / 1024.0;
    const int e0 = (int)cb, e1 = e0 + __builtin_amdgcn_readfirstlane(ev_n[c]);
    const bool lead = true;
    float2 *weights = weight_table + (size_t)c * 8 * kMvnBins;    // row v of it = row v + c of the table
#include "mvdrn_walk_body.h"
    if (kb < kMvnBins && e1 > e0) {
#pragma unroll
        for (int i = 0; i < 8; i++) mine[i] = d2_of(R[i]);
    }
    if (loading == 0.0) {                                         // singular by rank: no weights (the file's head)
        const int behind = __builtin_amdgcn_readfirstlane(word[s]) >> 1;     // estimation frames before this chunk
        const float nan = __builtin_nanf("");
        for (int v = e0; v <= e1 && behind + (v - e0) < n_mics; v++)
            if (r < n_mics && kb < kMvnBins) weights[((size_t)v * 8 + r) * kMvnBins + k] = make_float2(nan, nan);
    }
}

// ---- 5. apply: one wave per block of the concatenated axis -----------------------------------------------------------
// The frame body of mvdrn_apply_pairs_kernel, the same text (mvdrn_frame_body.h).  Block b >= 1 of a chunk reads the
// block before it from the span; block 0 reads the stream's carried block, and the first block a stream ever had has
// silence in front of it and emits nothing, so its wave leaves at once.  Time-aligned: every block writes at its own place.
struct MvnlSrc {
    const short *cur, *before;                                    // block b and the block before it of the next
    long chan_stride, before_stride;                              // microphone asked for (they come in order)
    __device__ __forceinline__ void load(int, int lane, u32x4 &prev, u32x4 &now)
    {
        prev = reinterpret_cast<const u32x4_span *>(before)[lane];
        now = reinterpret_cast<const u32x4_span *>(cur)[lane];
        cur += chan_stride;
        before += before_stride;
    }
    __device__ __forceinline__ void done(int, int) const {}
};

__global__ __launch_bounds__(64) void mvnl_apply_kernel(const short *__restrict__ pcm, long chan_stride, int n_mics,
                                                        const long long *__restrict__ stream_id,
                                                        const long long *__restrict__ sample_first,
                                                        const long long *__restrict__ block_first, long n_chunks,
                                                        long n_blocks, const int *__restrict__ row_of,
                                                        const short *__restrict__ carried,
                                                        const long long *__restrict__ seen,
                                                        const float2 *__restrict__ weights,
                                                        const float2 *__restrict__ table, short *__restrict__ out,
                                                        float *__restrict__ precast)
{
    const int lane = threadIdx.x;
    const long per_xcd = (gridDim.x + 7) >> 3;
    const long j = (long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (j >= n_blocks) return;
    const long c = ragged_find_utt(block_first, n_chunks, j);
    const long cb = uniform_i64(block_first + c);
    const long s = uniform_i64(stream_id + c);
    if (j == cb && uniform_i64(seen + s) == 0) return;
    const long at = uniform_i64(sample_first + c) + (j - cb) * 512;     // block j's first sample
    const long row = cb + c + __builtin_amdgcn_readfirstlane(row_of[j]);
    MvnlSrc src = {pcm + at, pcm + at - 512, chan_stride, chan_stride};
    if (j == cb) {
        src.before = carried + (size_t)s * 8 * 512;
        src.before_stride = 512;
    }
    const float2 *W = weights + (size_t)row * kMvnBins * 8;
#include "mvdrn_frame_body.h"
    mvn_emit_block<true>(y, lane, out ? out + at : nullptr, precast ? precast + at : nullptr);
}

// ---- 6. the state: one wave per chunk, behind every launch that read it ----------------------------------------------
__global__ __launch_bounds__(64) void mvnl_state_kernel(const short *__restrict__ pcm, long chan_stride, int n_mics,
                                                        const long long *__restrict__ stream_id,
                                                        const long long *__restrict__ sample_first,
                                                        const long long *__restrict__ block_first,
                                                        const unsigned char *__restrict__ code,
                                                        const int *__restrict__ ev_n, short *__restrict__ carried,
                                                        long long *__restrict__ seen, int *__restrict__ word)
{
    const int lane = threadIdx.x;
    const long c = blockIdx.x;
    const long cb = uniform_i64(block_first + c), n_own = uniform_i64(block_first + c + 1) - cb;
    if (n_own <= 0) return;
    const long s = uniform_i64(stream_id + c);
    const short *last = pcm + uniform_i64(sample_first + c) + (n_own - 1) * 512;
    for (int m = 0; m < n_mics; m++)
        reinterpret_cast<u32x4 *>(carried + ((size_t)s * 8 + m) * 512)[lane] =
            reinterpret_cast<const u32x4_span *>(last + (size_t)m * chan_stride)[lane];
    if (lane == 0) {
        seen[s] += n_own;
        const int events = (word[s] >> 1) + ev_n[c];
        word[s] = (code[cb + n_own - 1] == 0 ? 1 : 0) | ((events < 8 ? events : 8) << 1);
    }
}

// one workgroup per listed stream: fresh again
__global__ __launch_bounds__(256) void mvnl_reset_kernel(const long long *__restrict__ stream_id, MvnLive lv)
{
    const long long s = stream_id[blockIdx.x];
    const int tid = threadIdx.x;
    double2 *cov = lv.cov + (size_t)s * kMvnBins * 64;
    for (int i = tid; i < kMvnBins * 64; i += 256) cov[i] = make_double2(0.0, 0.0);
    unsigned int *prev = reinterpret_cast<unsigned int *>(lv.prev + (size_t)s * 8 * 512);
    for (int i = tid; i < 8 * 256; i += 256) prev[i] = 0u;
    if (tid == 0) {
        lv.seen[s] = 0;
        lv.word[s] = 0;
    }
}

int launch_mvdrn_live(hipStream_t s, const short *pcm, long chan_stride, int n_mics, const long long *stream_id,
                      const long long *sample_first, const long long *block_first, long n_chunks, long n_blocks,
                      const double *w_vad, const double2 *steer, double loading, const float2 *table, const MvnLive &lv,
                      unsigned char *flags, short *out, float *precast)
{
    if (n_chunks <= 0 || n_blocks <= 0) return 0;
    hipLaunchKernelGGL(mvnl_vad_kernel, dim3((unsigned)n_blocks), dim3(64), 0, s, pcm, sample_first, block_first, n_chunks,
                       n_blocks, w_vad, lv.code, flags);
    hipLaunchKernelGGL(mvnl_plan_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, stream_id, block_first, lv.code,
                       lv.word, lv.row, lv.events, lv.ev_n);
    const long g1 = n_blocks * n_mics < 4096 ? n_blocks * n_mics : 4096;
    hipLaunchKernelGGL(mvnl_event_spectra_kernel, dim3((unsigned)g1), dim3(64), 0, s, pcm, chan_stride, n_mics, stream_id,
                       sample_first, block_first, n_chunks, n_blocks, lv.events, lv.ev_n, lv.prev, table, lv.spec);
    hipLaunchKernelGGL(mvnl_update_kernel, dim3((unsigned)n_chunks, (kMvnBins + 7) / 8), dim3(64), 0, s, lv.spec, n_mics,
                       stream_id, block_first, lv.ev_n, lv.word, lv.cov, steer, loading, lv.weights);
    if (out || precast) {
        const long grid = (n_blocks + 7) / 8 * 8;
        hipLaunchKernelGGL(mvnl_apply_kernel, dim3((unsigned)grid), dim3(64), 0, s, pcm, chan_stride, n_mics, stream_id,
                           sample_first, block_first, n_chunks, n_blocks, lv.row, lv.prev, lv.seen, lv.weights, table, out,
                           precast);
    }
    hipLaunchKernelGGL(mvnl_state_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, pcm, chan_stride, n_mics, stream_id,
                       sample_first, block_first, lv.code, lv.ev_n, lv.prev, lv.seen, lv.word);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_mvdrn_live_reset(hipStream_t s, const long long *stream_id, long n_ids, const MvnLive &lv)
{
    if (n_ids <= 0) return 0;
    hipLaunchKernelGGL(mvnl_reset_kernel, dim3((unsigned)n_ids), dim3(256), 0, s, stream_id, lv);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
