// reverb_live_kernels.hip -- live reverberation streams (include/jdsp.h "live reverberation streams"): the batch's
// block (reverb_body.h, the text reverb_kernels.hip runs too) over chunks of streams whose history the handle carries
// as SPECTRA.
//   reverb_live_plan_kernel     block_first -> wave_first: ceil(B_c / 2) waves per chunk, prefixed (one workgroup)
//   reverb_live_analysis_kernel one half-spectrum row per NEW block into the call's workspace: the 1024-point frame
//                               [previous block | block]; in front of a chunk's first block stand the stream's carried
//                               512 samples, or zeros for a stream that has seen nothing
//   reverb_live_mac_kernel      a WAVE = two consecutive output blocks of one chunk; it walks the rows they need from the
//                               newest down -- rows of this chunk out of the workspace, older ones out of the stream's
//                               ring -- and stops at the stream's block 0; H straight from the bank (L2), no response in
//                               LDS, no workgroup barrier; Hermitian extension, pre-split, inverse wave FFT, scale, cast
//   reverb_live_commit_kernel   a workgroup per chunk: the chunk's last min(B_c, P - 1) rows into the ring (row of stream
//                               block i at slot i mod (P - 1)), its last 512 samples, blocks_seen += B_c
//   reverb_live_reset_kernel    the listed streams fresh
// The commit is a launch of its own because the analysis and the multiply-accumulate READ exactly what it WRITES (the
// carried samples, the ring, blocks_seen): stream order makes a delivery race-free, with nothing held twice and no
// parity word.
// Why the bytes are the batch's: per output block the operations are reverb_mac_kernel's, in its order, because they
// are the same functions -- the same rows (a row is a function of its two blocks of samples alone), the same H rows, p
// ascending in one accumulator chain from zero, the same finish.  Here: the carried samples as the lead, rows of the
// workspace and then of the ring, the response read from the bank, the commit and the reset.
#include "reverb_body.h"

namespace jdsp {

constexpr int kRlWaves = 4;                // waves per workgroup of the multiply-accumulate: independent of each other
constexpr int kRlCommitThreads = 256;

__global__ __launch_bounds__(kRvPlanThreads) void reverb_live_plan_kernel(const long long *__restrict__ block_first,
                                                                          long n_chunks, long long *__restrict__ wave_first)
{
    reverb_plan<kRvK>(block_first, n_chunks, wave_first);
}

// what stands in front of the first block of chunk c: the carried samples of its stream, zeros for a fresh one
__device__ __forceinline__ void rl_load_carried(const ReverbLive &lv, const long long *stream_id, long c, int lane,
                                                unsigned int (&h)[4])
{
    const long s = uniform_i64(stream_id + c);
    if (uniform_i64(lv.seen + s) > 0) rv_load_half(lv.last, s * kReverbBlock, lane, h);
    else {
#pragma unroll
        for (int q = 0; q < 4; q++) h[q] = 0u;
    }
}

__global__ __launch_bounds__(64) void reverb_live_analysis_kernel(const short *__restrict__ pcm,
                                                                  const long long *__restrict__ stream_id,
                                                                  const long long *__restrict__ sample_first,
                                                                  const long long *__restrict__ block_first, long n_chunks,
                                                                  long n_blocks, const float2 *__restrict__ table,
                                                                  ReverbLive lv)
{
    const int lane = threadIdx.x;
    reverb_analysis(pcm, sample_first, block_first, n_chunks, n_blocks, table, lv.X,
                    [&](long c, unsigned int (&h)[4]) { rl_load_carried(lv, stream_id, c, lane, h); });
}

struct ReverbLiveMacArgs {
    const float2 *bank;
    const long long *wave_first, *stream_id, *block_first, *sample_first;
    const int *ir;
    const float *gain;
    long n_chunks;
    int n_part, n_irs;
    short *out_i16;
    float *out_f32;
};

// Wave w of the plan belongs to the chunk c with wave_first[c] <= w < wave_first[c + 1] (the scalar binary search of
// ragged_batch.h) and owns its blocks k0 = 2 (w - wave_first[c]) and k0 + 1, stream blocks i0 + k0 and i0 + k0 + 1 with
// i0 = blocks_seen of the chunk's stream.  The walk reads the rows k0 + 1, k0, ... down to max(-i0, k0 + 1 - P) in the
// chunk's own numbering; row r >= 0 is row block_first[c] + r of the workspace, row r < 0 is stream block i0 + r in
// the ring.  Waves past wave_first[n_chunks] exit: the grid is the bound the host knows without reading the offsets.
__global__ __launch_bounds__(kRlWaves * 64) void reverb_live_mac_kernel(ReverbLiveMacArgs a, ReverbLive lv,
                                                                         const float2 *__restrict__ table)
{
    __shared__ __attribute__((aligned(16))) float2 smem[kRlWaves * kWaveLdsComplex];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float2 *lds = smem + wave * kWaveLdsComplex;                              // this wave's scratch: no wave reads another's
    const long w = (long)blockIdx.x * kRlWaves + wave;
    if (w >= uniform_i64(a.wave_first + a.n_chunks)) return;
    const long c = ragged_find_utt(a.wave_first, a.n_chunks, w);
    const long k0 = (w - uniform_i64(a.wave_first + c)) * kRvK;
    const long cb = uniform_i64(a.block_first + c);
    const long n_b = uniform_i64(a.block_first + c + 1) - cb;                 // > 0: the chunk has waves, and k0 < n_b
    const long s0 = uniform_i64(a.sample_first + c);
    const long s = uniform_i64(a.stream_id + c);
    const long i0 = uniform_i64(lv.seen + s);
    const int n_part = a.n_part;
    int irc = __builtin_amdgcn_readfirstlane(a.ir[c]);
    irc = irc < 0 ? 0 : (irc >= a.n_irs ? a.n_irs - 1 : irc);                 // never outside the bank
    const float g = a.gain ? a.gain[c] : 1.0f;
    const float scale = g * (1.0f / 1024.0f);                                 // the inverse's 1/1024 and the gain: one factor
    const float2 *H = a.bank + (size_t)irc * n_part * kRvPitch;

    const long r_top = k0 + (kRvK - 1);
    const int ring_n = n_part > 1 ? n_part - 1 : 1;
    const int m0 = (int)(i0 % ring_n);                                        // the slot stream block i0 will take
    const float2 *X = lv.X + cb * kRvPitch;                                   // the chunk's row 0
    const float2 *ring = lv.ring + (size_t)s * (n_part - 1) * kRvPitch;       // never read at P = 1
    auto row_of = [&](int q) {
        long r = r_top - q;
        if (r >= 0) return X + (r >= n_b ? n_b - 1 : r) * kRvPitch;           // clamped rows feed no written output
        r = r < -(long)ring_n ? -(long)ring_n : r;                            // -(P - 1) <= r: never taken (n_iter)
        const int slot = m0 + (int)r;                                         // (i0 + r) mod (P - 1)
        return ring + (slot < 0 ? slot + ring_n : slot) * kRvPitch;
    };
    // rows in front of the stream's first contribute nothing: the walk ends at stream block 0 (n_iter >= 2: the two
    // rows it starts with are rows of the chunk)
    const int n_full = n_part + kRvK - 1;
    const int n_iter = i0 + r_top + 1 < n_full ? (int)(i0 + r_top + 1) : n_full;
    float2 acc[kRvK][8], acc512[kRvK];
    reverb_mac_walk(row_of, H, n_iter, n_part, lane, acc, acc512);
    reverb_finish(acc, acc512, lds, lane, table, k0, n_b, s0, scale, a.out_i16, a.out_f32);
}

// ---- commit -----------------------------------------------------------------------------------------------------------
// Workgroup c: the chunk's last min(B_c, P - 1) rows from the workspace into the ring of its stream, its last 512 samples
// into the carried block, blocks_seen += B_c -- behind a barrier, after every thread has read the old count.
__global__ __launch_bounds__(kRlCommitThreads) void reverb_live_commit_kernel(const short *__restrict__ pcm,
                                                                              const long long *__restrict__ stream_id,
                                                                              const long long *__restrict__ sample_first,
                                                                              const long long *__restrict__ block_first,
                                                                              int n_part, ReverbLive lv)
{
    const long c = blockIdx.x;
    const long cb = block_first[c], n_b = block_first[c + 1] - cb;
    if (n_b <= 0) return;                                                     // the stream is not touched
    const long s = stream_id[c];
    const long i0 = lv.seen[s];
    const int ring_n = n_part - 1;
    const long n_rows = n_b < ring_n ? n_b : ring_n;
    float4 *ring = reinterpret_cast<float4 *>(lv.ring + (size_t)s * ring_n * kRvPitch);
    for (long k = n_b - n_rows; k < n_b; k++) {
        const float4 *src = reinterpret_cast<const float4 *>(lv.X + (cb + k) * kRvPitch);
        float4 *dst = ring + ((i0 + k) % ring_n) * (kRvPitch / 2);
        for (int i = threadIdx.x; i < kRvPitch / 2; i += kRlCommitThreads) dst[i] = src[i];
    }
    {
        const unsigned int *src = reinterpret_cast<const unsigned int *>(pcm + sample_first[c] + (n_b - 1) * kReverbBlock);
        unsigned int *dst = reinterpret_cast<unsigned int *>(lv.last + s * kReverbBlock);
        for (int i = threadIdx.x; i < kReverbBlock / 2; i += kRlCommitThreads) dst[i] = src[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) lv.seen[s] = i0 + n_b;
}

__global__ __launch_bounds__(kRlCommitThreads) void reverb_live_reset_kernel(const long long *__restrict__ stream_id,
                                                                             long n_streams, ReverbLive lv)
{
    const long s = stream_id[blockIdx.x];
    if (s < 0 || s >= n_streams) return;                                      // never outside the state
    unsigned int *dst = reinterpret_cast<unsigned int *>(lv.last + s * kReverbBlock);
    for (int i = threadIdx.x; i < kReverbBlock / 2; i += kRlCommitThreads) dst[i] = 0u;
    if (threadIdx.x == 0) lv.seen[s] = 0;
}

int launch_reverb_live(hipStream_t st, const ReverbLiveArgs &a, const float2 *bank, int n_part, int n_irs,
                       const float2 *rect_table, const ReverbLive &lv, long long *wave_first)
{
    if (a.n_chunks <= 0 || a.n_blocks_total <= 0) return 0;
    const long runs = (a.n_blocks_total + kRvRun - 1) / kRvRun;
    hipLaunchKernelGGL(reverb_live_analysis_kernel, dim3((unsigned)runs), dim3(64), 0, st, a.pcm, a.stream_id, a.sample_first,
                       a.block_first, a.n_chunks, a.n_blocks_total, rect_table, lv);
    if (a.out_i16 || a.out_f32) {                                             // with no output only the state advances
        hipLaunchKernelGGL(reverb_live_plan_kernel, dim3(1), dim3(kRvPlanThreads), 0, st, a.block_first, a.n_chunks, wave_first);
        // sum_c ceil(B_c / 2) <= (n_blocks_total + n_chunks) / 2
        const long waves = (a.n_blocks_total + a.n_chunks + 1) / 2;
        ReverbLiveMacArgs m = {bank, wave_first, a.stream_id, a.block_first, a.sample_first, a.ir, a.gain, a.n_chunks,
                               n_part, n_irs, a.out_i16, a.out_f32};
        hipLaunchKernelGGL(reverb_live_mac_kernel, dim3((unsigned)((waves + kRlWaves - 1) / kRlWaves)), dim3(kRlWaves * 64), 0,
                           st, m, lv, rect_table);
    }
    hipLaunchKernelGGL(reverb_live_commit_kernel, dim3((unsigned)a.n_chunks), dim3(kRlCommitThreads), 0, st, a.pcm,
                       a.stream_id, a.sample_first, a.block_first, n_part, lv);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_reverb_live_reset(hipStream_t st, const long long *stream_id, long n_ids, long n_streams, const ReverbLive &lv)
{
    if (n_ids <= 0) return 0;
    hipLaunchKernelGGL(reverb_live_reset_kernel, dim3((unsigned)n_ids), dim3(kRlCommitThreads), 0, st, stream_id, n_streams, lv);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
