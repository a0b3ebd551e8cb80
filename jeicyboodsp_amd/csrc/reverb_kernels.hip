// reverb_kernels.hip -- batched reverberation (include/jdsp.h "batched reverberation"): a batch of ragged utterances,
// each convolved with its own response out of a bank, as the uniformly partitioned overlap-save of fastconv_kernels.hip
// with the response chosen per utterance.
//   reverb_plan_kernel      block_first -> wg_first: ceil(B_u / G) workgroups per utterance, prefixed (one workgroup)
//   reverb_analysis_kernel  one half-spectrum row per block: the 1024-point frame [previous block | block], rectangular
//                           window, 512 zeros in front of an utterance's first block
//   reverb_mac_kernel       a workgroup = G = 32 output blocks of ONE utterance (16 waves x 2): H[ir[u]] in LDS once,
//                           each wave walks the rows its two blocks need from the newest down and stops at the
//                           utterance's first row; Hermitian extension, pre-split, inverse wave FFT, scale, cast
// The block itself -- plan, analysis, walk and finish -- is reverb_body.h, the text the live streams run too
// (reverb_live_kernels.hip).  Here: zeros as the lead, the response into LDS, the XCD remap, rows of the workspace alone.
#include "reverb_body.h"

namespace jdsp {

constexpr int kRvWaves = 16;
static_assert(kRvWaves * kRvK == kReverbGroup, "G sub-blocks per workgroup");

__global__ __launch_bounds__(kRvPlanThreads) void reverb_plan_kernel(const long long *__restrict__ block_first, long n_utts,
                                                                     long long *__restrict__ wg_first)
{
    reverb_plan<kReverbGroup>(block_first, n_utts, wg_first);
}

__global__ __launch_bounds__(64) void reverb_analysis_kernel(const short *__restrict__ pcm,
                                                             const long long *__restrict__ sample_first,
                                                             const long long *__restrict__ block_first, long n_utts,
                                                             long n_blocks, const float2 *__restrict__ table,
                                                             float2 *__restrict__ X)
{
    reverb_analysis(pcm, sample_first, block_first, n_utts, n_blocks, table, X, [](long, unsigned int (&h)[4]) {
#pragma unroll
        for (int q = 0; q < 4; q++) h[q] = 0u;                           // silence in front of the utterance
    });
}

struct ReverbMacArgs {
    const float2 *X, *bank;
    const long long *wg_first, *block_first, *sample_first;
    const int *ir;
    const float *gain;
    long n_utts;
    int n_part, n_irs;
    short *out_i16;
    float *out_f32;
};

// Workgroup w of the plan belongs to the utterance u with wg_first[u] <= w < wg_first[u + 1] (the scalar binary search of
// ragged_batch.h) and owns its blocks [G lw, G lw + G), lw = w - wg_first[u]; wave v the two blocks c0 = G lw + 2 v, c0 + 1.
// Output block c is sum_{p = 0}^{min(c, P - 1)} X[c - p] H_p, p ascending: the wave reads the rows c0 + 1, c0, ... down
// to max(0, c0 + 1 - P), two in flight, and every row feeds both blocks.  Workgroups past wg_first[n_utts] exit: the grid
// is the bound the host can know without reading the offsets.
__global__ __launch_bounds__(kRvWaves * 64) void reverb_mac_kernel(ReverbMacArgs a, const float2 *__restrict__ table)
{
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    float2 *Hs = smem;                                                        // [n_part][520]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_part = a.n_part;
    float2 *lds = smem + (size_t)n_part * kRvPitch + (size_t)wave * kWaveLdsComplex;   // this wave's scratch
    const long per_xcd = (gridDim.x + 7) >> 3;                                // neighbours share an XCD's L2: they
    const long w = (long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);      // read the same response and rows
    if (w >= uniform_i64(a.wg_first + a.n_utts)) return;
    const long u = ragged_find_utt(a.wg_first, a.n_utts, w);
    const long lw = w - uniform_i64(a.wg_first + u);
    const long ub = uniform_i64(a.block_first + u);
    const long n_b = uniform_i64(a.block_first + u + 1) - ub;                 // > 0: the utterance has workgroups
    const long s0 = uniform_i64(a.sample_first + u);
    int iru = __builtin_amdgcn_readfirstlane(a.ir[u]);
    iru = iru < 0 ? 0 : (iru >= a.n_irs ? a.n_irs - 1 : iru);                 // never outside the bank
    const float g = a.gain ? a.gain[u] : 1.0f;
    const float scale = g * (1.0f / 1024.0f);                                 // the inverse's 1/1024 and the gain: one factor
    {
        const float4 *src = reinterpret_cast<const float4 *>(a.bank + (size_t)iru * n_part * kRvPitch);
        float4 *dst = reinterpret_cast<float4 *>(Hs);
        for (int i = threadIdx.x; i < n_part * (kRvPitch / 2); i += kRvWaves * 64) dst[i] = src[i];
    }
    __syncthreads();
    const long c0 = (lw * kRvWaves + wave) * kRvK;
    if (c0 >= n_b) return;                                                    // no barrier follows

    const long r_top = c0 + (kRvK - 1);
    const float2 *X = a.X + ub * kRvPitch;                                    // the utterance's row 0
    auto row_of = [&](int q) {
        long r = r_top - q;
        r = r < 0 ? 0 : (r >= n_b ? n_b - 1 : r);                             // clamped rows feed no written output
        return X + r * kRvPitch;
    };
    // rows in front of the utterance's first contribute nothing: the walk ends at row 0
    const int n_full = n_part + kRvK - 1;
    const int n_iter = r_top + 1 < n_full ? (int)(r_top + 1) : n_full;
    float2 acc[kRvK][8], acc512[kRvK];
    reverb_mac_walk(row_of, Hs, n_iter, n_part, lane, acc, acc512);
    reverb_finish(acc, acc512, lds, lane, table, c0, n_b, s0, scale, a.out_i16, a.out_f32);
}

int launch_reverb_batch(hipStream_t st, const ReverbBatchArgs &a, const float2 *bank, int n_part, int n_irs,
                        const float2 *rect_table, float2 *X, long long *wg_first)
{
    if (a.n_utts <= 0 || a.n_blocks_total <= 0) return 0;
    hipLaunchKernelGGL(reverb_plan_kernel, dim3(1), dim3(kRvPlanThreads), 0, st, a.block_first, a.n_utts, wg_first);
    const long waves = (a.n_blocks_total + kRvRun - 1) / kRvRun;
    hipLaunchKernelGGL(reverb_analysis_kernel, dim3((unsigned)waves), dim3(64), 0, st, a.pcm, a.sample_first, a.block_first,
                       a.n_utts, a.n_blocks_total, rect_table, X);
    // sum_u ceil(B_u / G) <= n_blocks_total / G + n_utts, whole rounds of the eight XCDs
    const long grid = ((a.n_blocks_total + kReverbGroup - 1) / kReverbGroup + a.n_utts + 7) / 8 * 8;
    const size_t lds = ((size_t)n_part * kRvPitch + kRvWaves * (size_t)kWaveLdsComplex) * sizeof(float2);
    // more than 64 KB of dynamic LDS needs the attribute (a host-side flag: set on every launch, as launch_fastconv_upols)
    if (hipFuncSetAttribute((const void *)reverb_mac_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(((size_t)kReverbMaxPart * kRvPitch + kRvWaves * (size_t)kWaveLdsComplex) * sizeof(float2))) != hipSuccess)
        return -1;
    ReverbMacArgs m = {X, bank, wg_first, a.block_first, a.sample_first, a.ir, a.gain, a.n_utts, n_part, n_irs, a.out_i16, a.out_f32};
    hipLaunchKernelGGL(reverb_mac_kernel, dim3((unsigned)grid), dim3(kRvWaves * 64), lds, st, m, rect_table);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
