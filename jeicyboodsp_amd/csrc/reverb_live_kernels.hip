// reverb_live_kernels.hip -- live reverberation streams (include/jdsp.h "live reverberation streams"): the batch's
// arithmetic (reverb_kernels.hip) over chunks of streams whose history the handle carries as SPECTRA.
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
// Why the bytes are the batch's: per output block the operations are reverb_mac_kernel's, in its order -- the same
// rows (a row is a function of its two blocks of samples alone), the same H rows, p ascending in one accumulator chain
// from zero, the same finish.  The pieces are restated here, as reverb_kernels.hip restates the convolver's: that
// module's kernels compile to the same text as before (profiles/r30_reverb_streams_isa.txt).
#include "frame_io.h"
#include "reverb.h"
#include "ragged_batch.h"

namespace jdsp {

constexpr int kRlPitch = kUpolsRowPitch;
constexpr int kRlWaves = 4;                // waves per workgroup of the multiply-accumulate: independent of each other
constexpr int kRlK = 2, kRlDepth = 2;      // blocks per wave, rows in flight
constexpr int kRlRun = 4;                  // consecutive blocks of the concatenated block axis per analysis wave
constexpr int kRlPlanThreads = 1024;
constexpr int kRlCommitThreads = 256;

__device__ __forceinline__ long rl_waves_of(const long long *block_first, long c)
{
    const long b = (long)(block_first[c + 1] - block_first[c]);
    return b > 0 ? (b + kRlK - 1) / kRlK : 0;
}

// wave_first[c] = sum over d < c of ceil(B_d / 2), wave_first[n_chunks] = the waves that have work
__global__ __launch_bounds__(kRlPlanThreads) void reverb_live_plan_kernel(const long long *__restrict__ block_first,
                                                                          long n_chunks, long long *__restrict__ wave_first)
{
    __shared__ long long part[kRlPlanThreads];
    const int t = threadIdx.x;
    const long per = (n_chunks + kRlPlanThreads - 1) / kRlPlanThreads;
    const long a = t * per < n_chunks ? t * per : n_chunks, b = a + per < n_chunks ? a + per : n_chunks;
    long long sum = 0;
    for (long c = a; c < b; c++) sum += rl_waves_of(block_first, c);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < kRlPlanThreads; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - sum;
    for (long c = a; c < b; c++) {
        wave_first[c] = run;
        run += rl_waves_of(block_first, c);
    }
    if (t == kRlPlanThreads - 1) wave_first[n_chunks] = part[t];
}

// ---- analysis -----------------------------------------------------------------------------------------------------
template <int J>
__device__ __forceinline__ void rl_split_store_j(const float2 *lds, int lane, const float2 *w2, float2 *row)
{
    const int m = 128 * J + 2 * lane;
    const float4 zz = *reinterpret_cast<const float4 *>(&lds[m]);
    float2 zr0, zr1;
    load_mirror_pair(lds, m, zr0, zr1);
    float2 lo0, hi0, lo1, hi1;
    split_fwd<J>(make_float2(zz.x, zz.y), zr0, w2[0], lo0, hi0);
    split_fwd<J>(make_float2(zz.z, zz.w), zr1, w2[1], lo1, hi1);
    *reinterpret_cast<float4 *>(row + m) = make_float4(lo0.x, lo0.y, lo1.x, lo1.y);
    if (J == 0 && lane == 0) row[512] = hi0;
}

__device__ __forceinline__ void rl_load_half(const short *pcm, long at, int lane, unsigned int (&h)[4])
{
    const unsigned int *p = reinterpret_cast<const unsigned int *>(pcm + at) + lane;     // at is even
#pragma unroll
    for (int q = 0; q < 4; q++) h[q] = p[64 * q];
}

// what stands in front of the first block of chunk c: the carried samples of its stream, zeros for a fresh one
__device__ __forceinline__ void rl_load_carried(const ReverbLive &lv, const long long *stream_id, long c, int lane,
                                                unsigned int (&h)[4])
{
    const long s = uniform_i64(stream_id + c);
    if (uniform_i64(lv.seen + s) > 0) rl_load_half(lv.last, s * kReverbBlock, lane, h);
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
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    const int lane = threadIdx.x;
    const long j0 = (long)blockIdx.x * kRlRun;
    if (j0 >= n_blocks) return;
    const long j1 = j0 + kRlRun < n_blocks ? j0 + kRlRun : n_blocks;
    RaggedSpan<kReverbBlock> span(sample_first, block_first, n_chunks);
    span.begin(j0);
    unsigned int prev[4], cur[4], nxt[4];
    if (j0 > span.ub) rl_load_half(pcm, span.at(j0 - 1), lane, prev);
    else rl_load_carried(lv, stream_id, span.u, lane, prev);
    rl_load_half(pcm, span.at(j0), lane, cur);
    FrameTables t;
    load_frame_tables(t, table, lane);
    for (long j = j0; j < j1; j++) {
        const bool last = span.last(j);
        const bool more = j + 1 < j1;
        if (more) {
            if (last) span.next();                                       // block j + 1 exists: a non-empty chunk follows
            rl_load_half(pcm, span.at(j + 1), lane, nxt);
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
        float2 *row = lv.X + j * kRlPitch;
        rl_split_store_j<0>(lds, lane, t.wsp, row);
        rl_split_store_j<1>(lds, lane, t.wsp, row);
        rl_split_store_j<2>(lds, lane, t.wsp, row);
        rl_split_store_j<3>(lds, lane, t.wsp, row);
        wave_lds_fence();
        if (more) {
            if (last) rl_load_carried(lv, stream_id, span.u, lane, prev);  // the next chunk starts from its own stream
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
template <int J>
__device__ __forceinline__ void rl_presplit_j(const float2 *img, float2 *zout, int lane, const float2 *wsp)
{
    const int m = 128 * J + 2 * lane;
    const float4 yy = *reinterpret_cast<const float4 *>(&img[m]);
    float2 zr0, zr1;
    load_mirror_pair(img, m, zr0, zr1);                              // Y[512 - m], Y[511 - m]
    zout[2 * J] = presplit_inv<J>(make_float2(yy.x, yy.y), make_float2(zr0.x, -zr0.y), wsp[0]);
    zout[2 * J + 1] = presplit_inv<J>(make_float2(yy.z, yy.w), make_float2(zr1.x, -zr1.y), wsp[1]);
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
// i0 = blocks_seen of the chunk's stream.  Output block i is sum_{p = 0}^{min(i, P - 1)} X[i - p] H_p, p ascending: the
// wave reads the rows k0 + 1, k0, ... down to max(-i0, k0 + 1 - P) in the chunk's own numbering, two in flight, every
// row feeding both blocks; row r >= 0 is row block_first[c] + r of the workspace, row r < 0 is stream block i0 + r in
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
    const long k0 = (w - uniform_i64(a.wave_first + c)) * kRlK;
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
    const float2 *H = a.bank + (size_t)irc * n_part * kRlPitch;

    float2 acc[kRlK][8], acc512[kRlK];
#pragma unroll
    for (int k = 0; k < kRlK; k++) {
        acc512[k] = make_float2(0.f, 0.f);
#pragma unroll
        for (int q = 0; q < 8; q++) acc[k][q] = make_float2(0.f, 0.f);
    }
    const long r_top = k0 + (kRlK - 1);
    const int ring_n = n_part > 1 ? n_part - 1 : 1;
    const int m0 = (int)(i0 % ring_n);                                        // the slot stream block i0 will take
    const float2 *X = lv.X + cb * kRlPitch;                                   // the chunk's row 0
    const float2 *ring = lv.ring + (size_t)s * (n_part - 1) * kRlPitch;       // never read at P = 1
    auto row_of = [&](int q) {
        long r = r_top - q;
        if (r >= 0) return X + (r >= n_b ? n_b - 1 : r) * kRlPitch;           // clamped rows feed no written output
        r = r < -(long)ring_n ? -(long)ring_n : r;                            // -(P - 1) <= r: never taken (n_iter)
        const int slot = m0 + (int)r;                                         // (i0 + r) mod (P - 1)
        return ring + (slot < 0 ? slot + ring_n : slot) * kRlPitch;
    };
    // rows in front of the stream's first contribute nothing: the walk ends at stream block 0
    const int n_full = n_part + kRlK - 1;
    const int n_iter = i0 + r_top + 1 < n_full ? (int)(i0 + r_top + 1) : n_full;
    float4 xb[kRlDepth][4];
    float2 xb512[kRlDepth];
#pragma unroll
    for (int d = 0; d < kRlDepth; d++) {
        const float2 *xr = row_of(d);                                         // n_iter >= 2: both are rows of the chunk
#pragma unroll
        for (int j = 0; j < 4; j++) xb[d][j] = *reinterpret_cast<const float4 *>(xr + 128 * j + 2 * lane);
        xb512[d] = xr[512];
    }
    for (int q0 = 0; q0 < n_iter; q0 += kRlDepth) {
#pragma unroll
        for (int d = 0; d < kRlDepth; d++) {
            const int q = q0 + d;
            if (q >= n_iter) break;                                          // wave-uniform
#pragma unroll
            for (int k = 0; k < kRlK; k++) {
                const int p = q - (kRlK - 1) + k;                            // wave-uniform
                if (p < 0 || p >= n_part) continue;
                const float2 *hr = H + p * kRlPitch;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float4 h = *reinterpret_cast<const float4 *>(hr + 128 * j + 2 * lane);
                    const float4 x = xb[d][j];
                    acc[k][2 * j] = cadd(acc[k][2 * j], cmul(make_float2(x.x, x.y), make_float2(h.x, h.y)));
                    acc[k][2 * j + 1] = cadd(acc[k][2 * j + 1], cmul(make_float2(x.z, x.w), make_float2(h.z, h.w)));
                }
                acc512[k] = cadd(acc512[k], cmul(xb512[d], hr[512]));
            }
            if (q + kRlDepth < n_iter) {                                     // refill this slot
                const float2 *xr = row_of(q + kRlDepth);
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
    for (int k = 0; k < kRlK; k++) {
        const long b = k0 + k;
        if (b >= n_b) break;
#pragma unroll
        for (int j = 0; j < 4; j++)
            *reinterpret_cast<float4 *>(&lds[128 * j + 2 * lane]) =
                make_float4(acc[k][2 * j].x, acc[k][2 * j].y, acc[k][2 * j + 1].x, acc[k][2 * j + 1].y);
        if (lane == 0) lds[512] = acc512[k];
        wave_lds_fence();
        float2 z[8], y[8];
        rl_presplit_j<0>(lds, z, lane, wsp);
        rl_presplit_j<1>(lds, z, lane, wsp);
        rl_presplit_j<2>(lds, z, lane, wsp);
        rl_presplit_j<3>(lds, z, lane, wsp);
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
        const long at = s0 + b * kReverbBlock;                               // even: dword and float2 stores are aligned
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const float2 v = make_float2(y[d + 4].x * scale, y[d + 4].y * scale);
            if (a.out_i16)
                __builtin_nontemporal_store(cast_i16x2_bits(v.x, v.y), reinterpret_cast<unsigned int *>(a.out_i16 + at) + lane + 64 * d);
            if (a.out_f32) *reinterpret_cast<float2 *>(a.out_f32 + at + 2 * lane + 128 * d) = v;
        }
    }
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
    float4 *ring = reinterpret_cast<float4 *>(lv.ring + (size_t)s * ring_n * kRlPitch);
    for (long k = n_b - n_rows; k < n_b; k++) {
        const float4 *src = reinterpret_cast<const float4 *>(lv.X + (cb + k) * kRlPitch);
        float4 *dst = ring + ((i0 + k) % ring_n) * (kRlPitch / 2);
        for (int i = threadIdx.x; i < kRlPitch / 2; i += kRlCommitThreads) dst[i] = src[i];
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
    const long runs = (a.n_blocks_total + kRlRun - 1) / kRlRun;
    hipLaunchKernelGGL(reverb_live_analysis_kernel, dim3((unsigned)runs), dim3(64), 0, st, a.pcm, a.stream_id, a.sample_first,
                       a.block_first, a.n_chunks, a.n_blocks_total, rect_table, lv);
    if (a.out_i16 || a.out_f32) {                                             // with no output only the state advances
        hipLaunchKernelGGL(reverb_live_plan_kernel, dim3(1), dim3(kRlPlanThreads), 0, st, a.block_first, a.n_chunks, wave_first);
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
