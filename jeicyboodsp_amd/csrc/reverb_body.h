// reverb_body.h -- the one text of a reverberation block, under the batch kernels (reverb_kernels.hip) and the live ones
// (reverb_live_kernels.hip): the plan, the analysis of a run of blocks, the multiply-accumulate walk of a wave's two
// output blocks and their finish.  The arithmetic is fastconv_upols4_kernel's, instruction for instruction (the complex
// helpers are inline assembly: wave_fft512.h), so what a block comes out as depends on its index in its stream, the
// partition count, the samples and the response alone.  That a live stream's bytes are the batch's whatever the cuts
// follows from both sets of kernels being this text; they differ in what they hand it:
//   the lead     what stands in front of a span's first block: zeros (batch), the stream's carried 512 samples (live)
//   the rows     where row r_top - q of a wave's walk lies: the workspace (batch), the workspace, then the ring (live)
//   the response LDS (batch), the bank (live)
// Every piece is a function: the kernels keep their LDS, no scratch, their floating-point, conversion and memory opcode
// counts and their time (profiles/r31_reverb_one_body.txt).  The pre-split of a pair and the even-row split store
// also live inside fastconv_kernels.hip and stft_kernels.hip; those modules are not built on this header, since
// fastconv_upols4_kernel's code depends on what else its module holds (see there).
#pragma once
#include "frame_io.h"
#include "reverb.h"
#include "ragged_batch.h"

namespace jdsp {

constexpr int kRvPitch = kUpolsRowPitch;
constexpr int kRvK = 2, kRvDepth = 2;      // blocks per wave of the multiply-accumulate, rows in flight
constexpr int kRvRun = 4;                  // consecutive blocks of the concatenated block axis per analysis wave: every
                                           // sample is read once inside a run, the previous block again at a run's start
constexpr int kRvPlanThreads = 1024;

// ---- plan ---------------------------------------------------------------------------------------------------------
// first[u] = sum over v < u of ceil(B_v / PER), first[n] = the units (workgroups, waves) that have work.  One
// workgroup: thread t owns a run of consecutive spans, the runs' sums are scanned in LDS.
template <int PER> __device__ __forceinline__ long rv_units_of(const long long *block_first, long u)
{
    const long b = (long)(block_first[u + 1] - block_first[u]);
    return b > 0 ? (b + PER - 1) / PER : 0;
}

template <int PER>
__device__ __forceinline__ void reverb_plan(const long long *__restrict__ block_first, long n, long long *__restrict__ first)
{
    __shared__ long long part[kRvPlanThreads];
    const int t = threadIdx.x;
    const long per = (n + kRvPlanThreads - 1) / kRvPlanThreads;
    const long a = t * per < n ? t * per : n, b = a + per < n ? a + per : n;
    long long sum = 0;
    for (long u = a; u < b; u++) sum += rv_units_of<PER>(block_first, u);
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
        first[u] = run;
        run += rv_units_of<PER>(block_first, u);
    }
    if (t == kRvPlanThreads - 1) first[n] = part[t];
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

__device__ __forceinline__ void rv_load_half(const short *pcm, long at, int lane, unsigned int (&h)[4])
{
    const unsigned int *p = reinterpret_cast<const unsigned int *>(pcm + at) + lane;     // at is even: sample_first is
#pragma unroll
    for (int q = 0; q < 4; q++) h[q] = p[64 * q];
}

// One wave, the blocks [kRvRun blockIdx.x, + kRvRun) of the concatenated block axis: one half-spectrum row per block,
// the 1024-point frame [previous block | block], rectangular window.  lead(u, h) fills h with the 512 samples in front
// of span u's first block.
template <class Lead>
__device__ __forceinline__ void reverb_analysis(const short *pcm, const long long *sample_first, const long long *block_first,
                                                long n_spans, long n_blocks, const float2 *table, float2 *X, Lead lead)
{
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    const int lane = threadIdx.x;
    const long j0 = (long)blockIdx.x * kRvRun;
    if (j0 >= n_blocks) return;
    const long j1 = j0 + kRvRun < n_blocks ? j0 + kRvRun : n_blocks;
    RaggedSpan<kReverbBlock> span(sample_first, block_first, n_spans);
    span.begin(j0);
    unsigned int prev[4], cur[4], nxt[4];
    if (j0 > span.ub) rv_load_half(pcm, span.at(j0 - 1), lane, prev);
    else lead(span.u, prev);
    rv_load_half(pcm, span.at(j0), lane, cur);
    FrameTables t;
    load_frame_tables(t, table, lane);
    for (long j = j0; j < j1; j++) {
        const bool last = span.last(j);
        const bool more = j + 1 < j1;
        if (more) {
            if (last) span.next();                                       // block j + 1 exists: a non-empty span follows
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
            if (last) lead(span.u, prev);                                // the next span starts from its own lead
            else {
#pragma unroll
                for (int q = 0; q < 4; q++) prev[q] = cur[q];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) cur[q] = nxt[q];
        }
    }
}

// ---- multiply-accumulate and inverse --------------------------------------------------------------------------------
// A wave owns two consecutive output blocks c0, c0 + 1 of one span.  Output block c is sum_{p = 0}^{min(c, P - 1)}
// X[c - p] H_p, p ascending in one accumulator chain from zero: the wave reads the rows c0 + 1, c0, ... -- row_of(q) is
// where row c0 + 1 - q lies -- n_iter of them, two in flight, and every row feeds both blocks.  H: the response's
// n_part rows.
template <class RowOf>
__device__ __forceinline__ void reverb_mac_walk(RowOf row_of, const float2 *H, int n_iter, int n_part, int lane,
                                                float2 (&acc)[kRvK][8], float2 (&acc512)[kRvK])
{
#pragma unroll
    for (int k = 0; k < kRvK; k++) {
        acc512[k] = make_float2(0.f, 0.f);
#pragma unroll
        for (int q = 0; q < 8; q++) acc[k][q] = make_float2(0.f, 0.f);
    }
    float4 xb[kRvDepth][4];
    float2 xb512[kRvDepth];
#pragma unroll
    for (int d = 0; d < kRvDepth; d++) {
        const float2 *xr = row_of(d);
#pragma unroll
        for (int j = 0; j < 4; j++) xb[d][j] = *reinterpret_cast<const float4 *>(xr + 128 * j + 2 * lane);
        xb512[d] = xr[512];
    }
    for (int q0 = 0; q0 < n_iter; q0 += kRvDepth) {
#pragma unroll
        for (int d = 0; d < kRvDepth; d++) {
            const int q = q0 + d;
            if (q >= n_iter) break;                                          // wave-uniform
#pragma unroll
            for (int k = 0; k < kRvK; k++) {
                const int p = q - (kRvK - 1) + k;                            // wave-uniform
                if (p < 0 || p >= n_part) continue;
                const float2 *hr = H + p * kRvPitch;
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
}

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

// The walk's sums to samples: Hermitian extension, pre-split, inverse wave FFT, scale (the inverse's 1/1024 and the
// gain: one factor), cast.  Blocks c0 and c0 + 1 of a span of n_b blocks whose first sample is s0; lds: this wave's.
__device__ __forceinline__ void reverb_finish(const float2 (&acc)[kRvK][8], const float2 (&acc512)[kRvK], float2 *lds,
                                              int lane, const float2 *table, long c0, long n_b, long s0, float scale,
                                              short *out_i16, float *out_f32)
{
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
            if (out_i16)
                __builtin_nontemporal_store(cast_i16x2_bits(v.x, v.y), reinterpret_cast<unsigned int *>(out_i16 + at) + lane + 64 * d);
            if (out_f32) *reinterpret_cast<float2 *>(out_f32 + at + 2 * lane + 128 * d) = v;
        }
    }
}

}  // namespace jdsp
