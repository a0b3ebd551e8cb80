// reverb_kernels.hip -- batched reverberation (include/jdsp.h "batched reverberation"): a batch of ragged utterances,
// each convolved with its own response out of a bank, as the uniformly partitioned overlap-save of fastconv_kernels.hip
// with the response chosen per utterance.
//   reverb_plan_kernel      block_first -> wg_first: ceil(B_u / G) workgroups per utterance, prefixed (one workgroup)
//   reverb_analysis_kernel  one half-spectrum row per block: the 1024-point frame [previous block | block], rectangular
//                           window, 512 zeros in front of an utterance's first block
//   reverb_mac_kernel       a workgroup = G = 32 output blocks of ONE utterance (16 waves x 2): H[ir[u]] in LDS once,
//                           each wave walks the rows its two blocks need from the newest down and stops at the
//                           utterance's first row; Hermitian extension, pre-split, inverse wave FFT, scale, cast
// The arithmetic is fastconv_upols4_kernel's, instruction for instruction (the complex helpers are inline assembly:
// wave_fft512.h), so what a block comes out as depends on its index in the utterance, the partition count, the samples
// and the response alone -- not on the wave, the workgroup or the utterance's place in the batch.  The pieces that
// live inside fastconv_kernels.hip and stft_kernels.hip (the pre-split of a pair, the even-row split store) are
// restated here: those modules compile to the same text as before (profiles/r29_reverb_batch_isa.txt).
#include "frame_io.h"
#include "reverb.h"
#include "ragged_batch.h"

namespace jdsp {

constexpr int kRvPitch = kUpolsRowPitch;
constexpr int kRvWaves = 16, kRvK = 2, kRvDepth = 2;
static_assert(kRvWaves * kRvK == kReverbGroup, "G sub-blocks per workgroup");
constexpr int kRvPlanThreads = 1024;

__device__ __forceinline__ long rv_wgs_of(const long long *block_first, long u)
{
    const long b = (long)(block_first[u + 1] - block_first[u]);
    return b > 0 ? (b + kReverbGroup - 1) / kReverbGroup : 0;
}

// wg_first[u] = sum over v < u of ceil(B_v / G), wg_first[n_utts] = the workgroups that have work.  One workgroup:
// thread t owns a run of consecutive utterances, the runs' sums are scanned in LDS.
__global__ __launch_bounds__(kRvPlanThreads) void reverb_plan_kernel(const long long *__restrict__ block_first, long n_utts,
                                                                     long long *__restrict__ wg_first)
{
    __shared__ long long part[kRvPlanThreads];
    const int t = threadIdx.x;
    const long per = (n_utts + kRvPlanThreads - 1) / kRvPlanThreads;
    const long a = t * per < n_utts ? t * per : n_utts, b = a + per < n_utts ? a + per : n_utts;
    long long sum = 0;
    for (long u = a; u < b; u++) sum += rv_wgs_of(block_first, u);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < kRvPlanThreads; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - sum;
    for (long u = a; u < b; u++) {
        wg_first[u] = run;
        run += rv_wgs_of(block_first, u);
    }
    if (t == kRvPlanThreads - 1) wg_first[n_utts] = part[t];
}

// ---- analysis -----------------------------------------------------------------------------------------------------
// stft_kernels.hip's even-row split store (split_store_half<false>): every row here is 16-byte aligned
template <int J>
__device__ __forceinline__ void rv_split_store_j(const float2 *lds, int lane, const float2 *w2, float2 *row)
{
    const int m = 128 * J + 2 * lane;
    const float4 zz = *reinterpret_cast<const float4 *>(&lds[m]);
    float2 zr0, zr1;
    load_mirror_pair(lds, m, zr0, zr1);
    float2 lo0, hi0, lo1, hi1;
    split_fwd<J>(make_float2(zz.x, zz.y), zr0, w2[0], lo0, hi0);
    split_fwd<J>(make_float2(zz.z, zz.w), zr1, w2[1], lo1, hi1);
    *reinterpret_cast<float4 *>(row + m) = make_float4(lo0.x, lo0.y, lo1.x, lo1.y);      // read again soon: not streamed
    if (J == 0 && lane == 0) row[512] = hi0;                                             // bin 512 = X[0 + 512]
}

constexpr int kRvRun = 4;      // consecutive blocks of the concatenated block axis per wave: every sample is read once
                               // inside a run, the previous block a second time at a run's start

__device__ __forceinline__ void rv_load_half(const short *pcm, long at, int lane, unsigned int (&h)[4])
{
    const unsigned int *p = reinterpret_cast<const unsigned int *>(pcm + at) + lane;     // at is even: sample_first is
#pragma unroll
    for (int q = 0; q < 4; q++) h[q] = p[64 * q];
}

__global__ __launch_bounds__(64) void reverb_analysis_kernel(const short *__restrict__ pcm,
                                                             const long long *__restrict__ sample_first,
                                                             const long long *__restrict__ block_first, long n_utts,
                                                             long n_blocks, const float2 *__restrict__ table,
                                                             float2 *__restrict__ X)
{
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    const int lane = threadIdx.x;
    const long j0 = (long)blockIdx.x * kRvRun;
    if (j0 >= n_blocks) return;
    const long j1 = j0 + kRvRun < n_blocks ? j0 + kRvRun : n_blocks;
    RaggedSpan<kReverbBlock> span(sample_first, block_first, n_utts);
    span.begin(j0);
    unsigned int prev[4], cur[4], nxt[4];
    if (j0 > span.ub) rv_load_half(pcm, span.at(j0 - 1), lane, prev);
    else {
#pragma unroll
        for (int q = 0; q < 4; q++) prev[q] = 0u;                        // silence in front of the utterance
    }
    rv_load_half(pcm, span.at(j0), lane, cur);
    FrameTables t;
    load_frame_tables(t, table, lane);
    for (long j = j0; j < j1; j++) {
        const bool last = span.last(j);
        const bool more = j + 1 < j1;
        if (more) {
            if (last) span.next();                                       // block j + 1 exists: a non-empty utterance follows
            rv_load_half(pcm, span.at(j + 1), lane, nxt);
        }
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float2 s0 = unpack_i16x2(prev[r]), s1 = unpack_i16x2(cur[r]);
            v[r] = make_float2(s0.x * t.win[r].x, s0.y * t.win[r].y);
            v[r + 4] = make_float2(s1.x * t.win[r + 4].x, s1.y * t.win[r + 4].y);
        }
        wave_fft512<false>(v, lds, lane, t.tw);
        store_natural_image(lds, lane, v);
        wave_lds_fence();
        float2 *row = X + j * kRvPitch;
        rv_split_store_j<0>(lds, lane, t.wsp, row);
        rv_split_store_j<1>(lds, lane, t.wsp, row);
        rv_split_store_j<2>(lds, lane, t.wsp, row);
        rv_split_store_j<3>(lds, lane, t.wsp, row);
        wave_lds_fence();
        if (more) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                prev[q] = last ? 0u : cur[q];                            // a new utterance starts from silence
                cur[q] = nxt[q];
            }
        }
    }
}

// ---- multiply-accumulate and inverse --------------------------------------------------------------------------------
template <int J>
__device__ __forceinline__ void rv_presplit_j(const float2 *img, float2 *zout, int lane, const float2 *wsp)
{
    const int m = 128 * J + 2 * lane;
    const float4 yy = *reinterpret_cast<const float4 *>(&img[m]);
    float2 zr0, zr1;
    load_mirror_pair(img, m, zr0, zr1);                              // Y[512 - m], Y[511 - m]
    // Y[m + 512] = conj(Y[512 - m]): the output is real
    zout[2 * J] = presplit_inv<J>(make_float2(yy.x, yy.y), make_float2(zr0.x, -zr0.y), wsp[0]);
    zout[2 * J + 1] = presplit_inv<J>(make_float2(yy.z, yy.w), make_float2(zr1.x, -zr1.y), wsp[1]);
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

    float2 acc[kRvK][8], acc512[kRvK];
#pragma unroll
    for (int k = 0; k < kRvK; k++) {
        acc512[k] = make_float2(0.f, 0.f);
#pragma unroll
        for (int q = 0; q < 8; q++) acc[k][q] = make_float2(0.f, 0.f);
    }
    const long r_top = c0 + (kRvK - 1);
    const float2 *X = a.X + ub * kRvPitch;                                    // the utterance's row 0
    auto row_of = [&](int q) {
        long r = r_top - q;
        r = r < 0 ? 0 : (r >= n_b ? n_b - 1 : r);                             // clamped rows feed no written output
        return X + r * kRvPitch;
    };
    float4 xb[kRvDepth][4];
    float2 xb512[kRvDepth];
#pragma unroll
    for (int d = 0; d < kRvDepth; d++) {
        const float2 *xr = row_of(d);
#pragma unroll
        for (int j = 0; j < 4; j++) xb[d][j] = *reinterpret_cast<const float4 *>(xr + 128 * j + 2 * lane);
        xb512[d] = xr[512];
    }
    // rows in front of the utterance's first contribute nothing: the walk ends at row 0
    const int n_full = n_part + kRvK - 1;
    const int n_iter = r_top + 1 < n_full ? (int)(r_top + 1) : n_full;
    for (int q0 = 0; q0 < n_iter; q0 += kRvDepth) {
#pragma unroll
        for (int d = 0; d < kRvDepth; d++) {
            const int q = q0 + d;
            if (q >= n_iter) break;                                          // wave-uniform
#pragma unroll
            for (int k = 0; k < kRvK; k++) {
                const int p = q - (kRvK - 1) + k;                            // wave-uniform
                if (p < 0 || p >= n_part) continue;
                const float2 *hr = Hs + p * kRvPitch;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float4 h = *reinterpret_cast<const float4 *>(hr + 128 * j + 2 * lane);
                    const float4 x = xb[d][j];
                    acc[k][2 * j] = cadd(acc[k][2 * j], cmul(make_float2(x.x, x.y), make_float2(h.x, h.y)));
                    acc[k][2 * j + 1] = cadd(acc[k][2 * j + 1], cmul(make_float2(x.z, x.w), make_float2(h.z, h.w)));
                }
                acc512[k] = cadd(acc512[k], cmul(xb512[d], hr[512]));
            }
            if (q + kRvDepth < n_iter) {                                     // refill this slot
                const float2 *xr = row_of(q + kRvDepth);
#pragma unroll
                for (int j = 0; j < 4; j++) xb[d][j] = *reinterpret_cast<const float4 *>(xr + 128 * j + 2 * lane);
                xb512[d] = xr[512];
            }
        }
    }
    WaveTwiddles tw;
    load_wave_twiddles(tw, table, lane);
    const float2 wsp[2] = {table[kStftSplit + 2 * lane], table[kStftSplit + 2 * lane + 1]};
#pragma unroll
    for (int k = 0; k < kRvK; k++) {
        const long c = c0 + k;
        if (c >= n_b) break;
#pragma unroll
        for (int j = 0; j < 4; j++)
            *reinterpret_cast<float4 *>(&lds[128 * j + 2 * lane]) =
                make_float4(acc[k][2 * j].x, acc[k][2 * j].y, acc[k][2 * j + 1].x, acc[k][2 * j + 1].y);
        if (lane == 0) lds[512] = acc512[k];
        wave_lds_fence();
        float2 z[8], y[8];
        rv_presplit_j<0>(lds, z, lane, wsp);
        rv_presplit_j<1>(lds, z, lane, wsp);
        rv_presplit_j<2>(lds, z, lane, wsp);
        rv_presplit_j<3>(lds, z, lane, wsp);
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < 4; j++)
            *reinterpret_cast<float4 *>(&lds[128 * j + 2 * lane]) = make_float4(z[2 * j].x, z[2 * j].y, z[2 * j + 1].x, z[2 * j + 1].y);
        wave_lds_fence();
#pragma unroll
        for (int r = 0; r < 8; r++) y[r] = lds[lane + 64 * r];
        wave_lds_fence();
        wave_fft512<true>(y, lds, lane, tw);
        wave_lds_fence();
        // samples 512..1023 of the frame are the valid ones: y[4..7] hold the pairs 2 lane + 128 d
        const long at = s0 + c * kReverbBlock;                               // even: dword and float2 stores are aligned
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const float2 v = make_float2(y[d + 4].x * scale, y[d + 4].y * scale);
            if (a.out_i16)
                __builtin_nontemporal_store(cast_i16x2_bits(v.x, v.y), reinterpret_cast<unsigned int *>(a.out_i16 + at) + lane + 64 * d);
            if (a.out_f32) *reinterpret_cast<float2 *>(a.out_f32 + at + 2 * lane + 128 * d) = v;
        }
    }
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
