// binaural_kernels.hip -- live binaural rendering on gfx950 (include/jdsp.h, "binaural rendering"): every output
// block of a mix is the sum over the mix's sources of overlap-save convolutions (Fast_Convolution_Based_3DAudio_Impl.cpp
// :102-177, 1024-point transforms, 512-sample blocks) with the HRIR pair of each source's direction, summed IN THE
// SPECTRUM: S forward transforms and two inverse ones per block (four while a source fades), not S + 2 S.
//
//   binaural_render_kernel   one wavefront per output block over the concatenated block axis
//   binaural_commit_kernel   parity[stream] ^= 1 for the chunks of mixes that got blocks
//   binaural_reset_kernel    the listed streams fresh again
//   binaural_bank_kernel     FP64 spectra of the taps -> the FP32 bank in the layout the render kernel reads
//
// The arithmetic of one block of mix m, fixed here and relied on by the tests (cuts, independence):
//   - per chunk, in LIST ORDER: the segment [previous 512 samples | the block's 512] goes through wave_fft512 as 512
//     packed complex values, unscaled; the pair-owned split (frame_io.h) gives the lane X[k], X[k + 512] for its five
//     k = lane + 64 d; THE GAIN ENTERS HERE: the ten split values are multiplied by the chunk's gain in FP32; each
//     product is then multiplied by the two ears' bank values of the chunk's direction and added to the ear's
//     accumulator, acc <- acc + (g X) H as two packed FMAs (cmac).  The bank carries the transform's 1/1024 and the
//     split's 1/2 (powers of two, exact).
//   - the PLAIN form: one accumulated spectrum per ear, presplit_inv_pair and the staggered two-ear inverse transform,
//     samples 512..1023 kept.  A block takes it exactly when none of its chunks fades, i.e. for b >= 1 always and for
//     b = 0 when every chunk's carried (dir, gain) equals the delivered one (gains compared as bit patterns; a fresh
//     stream carries nothing and never fades).
//   - the FADED form: a second pair of accumulators, "old", takes (g0 X) H[d0] of every chunk -- for the chunks that
//     do not fade the same bits as "new" -- and goes through a second two-ear inverse; the kept samples are
//     fma(r, new, (1 - r) old) in FP32 with r = i / 512 (exact, and so is 1 - r).
// The instructions of the plain form do not depend on b, on the place of the mix or on stream ids: where the samples
// come from (the carried history or the chunk) is a pair of wave-uniform base pointers, nothing else.  That is what
// makes a stream cut into deliveries give the same bits.
//
// The bank holds, per direction and ear, only the 640 values the pair scheme reads (bins k and k + 512 for the 320
// values k = lane + 64 d, d < 5; the spectrum of real taps is Hermitian, the rest is redundant), in the order the
// lanes read them: row[(h 5 + d) 64 + lane] = H[lane + 64 d + 512 h].  5,120 bytes per ear, 10 KB per direction,
// every load a 512-byte line-aligned run.
#include "frame_io.h"
#include "jdsp_internal.h"
#include "ragged_batch.h"

namespace jdsp {

// acc + a * w: (acc.x + a.x w.x - a.y w.y, acc.y + a.x w.y + a.y w.x)
__device__ __forceinline__ float2 cmac(float2 acc, float2 a, float2 w)
{
    cfv t, r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(t) : "v"(tv(a)), "v"(tv(w)), "v"(tv(acc)));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(tv(a)), "v"(tv(w)), "v"(t));
    return fv(r);
}

__device__ __forceinline__ int uniform_i32(const int *p) { return __builtin_amdgcn_readfirstlane(*p); }
__device__ __forceinline__ long clamp_idx(long v, long n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// What a wave knows of one chunk before it touches its samples: all wave-uniform.
struct BinChunk {
    const short *lo, *hi;      // the segment's samples 0..511 and 512..1023
    const float2 *h_new;       // bank rows of the delivered direction: [2 ears][640]
    const float2 *h_old;       // ... of the carried one (== h_new when the chunk does not fade)
    float g_new, g_old;
    long at_out;               // where the stream's next state goes: (parity ^ 1) n_streams + stream
    int d_new;
};

__global__ __launch_bounds__(64, 2) void binaural_render_kernel(
    const short *__restrict__ pcm, const long long *__restrict__ stream_id, const long long *__restrict__ sample_first,
    const int *__restrict__ dir, const float *__restrict__ gain, const long long *__restrict__ chunk_first,
    const long long *__restrict__ block_first, long n_mixes, const float2 *__restrict__ bank, int n_dirs,
    const float2 *__restrict__ table, const int *__restrict__ parity, BinauralStreams st, short *__restrict__ out_i16,
    float *__restrict__ out_f32, long plane)
{
    __shared__ __attribute__((aligned(16))) float2 lds[2 * kWaveLdsComplex];
    float2 *lds_b = lds + kWaveLdsComplex;
    const int lane = threadIdx.x;
    const long j = blockIdx.x;
    const long m = ragged_find_utt(block_first, n_mixes, j);
    const long b = j - uniform_i64(block_first + m);
    const bool first = b == 0, last = j + 1 == uniform_i64(block_first + m + 1);
    const long c0 = uniform_i64(chunk_first + m), c1 = uniform_i64(chunk_first + m + 1);

    // Does any chunk of this block fade?  Only a mix's block 0 can; a lane per chunk looks.
    bool faded = false;
    if (first) {
        int f = 0;
        for (long c = c0 + lane; c < c1; c += 64) {
            const long s = clamp_idx(stream_id[c], st.n_streams);
            const long at = (long)(parity[s] & 1) * st.n_streams + s;
            if (st.started[at])
                f |= (st.dir[at] != (int)clamp_idx(dir[c], n_dirs)) |
                     (__float_as_int(st.gain[at]) != __float_as_int(gain[c]));
        }
        faded = __builtin_amdgcn_ballot_w64(f != 0) != 0;
    }

    const auto chunk_of = [&](long c) {
        BinChunk k;
        const long sf = uniform_i64(sample_first + c);
        k.d_new = (int)clamp_idx(uniform_i32(dir + c), n_dirs);
        k.g_new = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gain[c])));
        k.h_new = bank + (size_t)k.d_new * 1280;
        k.h_old = k.h_new, k.g_old = k.g_new, k.at_out = 0;
        if (first || last) {
            const long s = clamp_idx(uniform_i64(stream_id + c), st.n_streams);
            const int p = uniform_i32(parity + s) & 1;
            const long at = (long)p * st.n_streams + s;
            k.at_out = (long)(p ^ 1) * st.n_streams + s;
            if (first) {
                k.lo = st.hist + at * 512;             // zeros for a fresh stream: silence lies before its first sample
                k.hi = pcm + sf;
                if (uniform_i32(st.started + at)) {
                    k.h_old = bank + (size_t)uniform_i32(st.dir + at) * 1280;
                    k.g_old = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(st.gain[at])));
                }
                return k;
            }
        }
        k.lo = pcm + sf + 512 * (b - 1);
        k.hi = k.lo + 512;
        return k;
    };

    WaveTwiddles tw;
    load_wave_twiddles(tw, table, lane);
    PairTwiddles pw;
    load_pair_twiddles(pw, table, lane);

    float2 acc_n[2][10], acc_o[2][10];
#pragma unroll
    for (int e = 0; e < 2; e++)
#pragma unroll
        for (int q = 0; q < 10; q++) acc_n[e][q] = acc_o[e][q] = make_float2(0.f, 0.f);

    // The next chunk's samples are requested before this chunk's arithmetic starts (the pairs kernel of
    // fastconv_kernels.hip says what that is worth: a wave with nothing in flight spent 61 % of its time waiting).
    // The chunk's own bank rows are requested in front of its forward transform and used behind it: the transform
    // covers their way from L2, and held one chunk ahead they would cost forty more registers (scratch at two waves
    // per SIMD).
    unsigned int nxt[8];
    BinChunk kn;
    const auto request = [&](const BinChunk &k) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            nxt[r] = reinterpret_cast<const unsigned int *>(k.lo)[lane + 64 * r];
            nxt[r + 4] = reinterpret_cast<const unsigned int *>(k.hi)[lane + 64 * r];
        }
    };
    if (c0 < c1) {
        kn = chunk_of(c0);
        request(kn);
    }
    for (long c = c0; c < c1; c++) {
        const BinChunk k = kn;
        unsigned int cur[8];
        float2 h[2][10];
#pragma unroll
        for (int r = 0; r < 8; r++) cur[r] = nxt[r];
#pragma unroll
        for (int e = 0; e < 2; e++)
#pragma unroll
            for (int q = 0; q < 10; q++) h[e][q] = k.h_new[e * 640 + q * 64 + lane];
        if (c + 1 < c1) {
            kn = chunk_of(c + 1);
            request(kn);
        }
        float2 ho[2][10];
        if (faded) {
            // requested in front of the forward transform, used behind it
#pragma unroll
            for (int e = 0; e < 2; e++)
#pragma unroll
                for (int q = 0; q < 10; q++) ho[e][q] = k.h_old[e * 640 + q * 64 + lane];
        }
        if (last) {
            // the state the stream's next delivery starts from, into the copy no wave of this launch reads
            unsigned int *hw = reinterpret_cast<unsigned int *>(st.hist + k.at_out * 512);
#pragma unroll
            for (int r = 0; r < 4; r++) hw[lane + 64 * r] = cur[r + 4];
            if (lane == 0) {
                st.dir[k.at_out] = k.d_new;
                st.gain[k.at_out] = k.g_new;
                st.started[k.at_out] = 1;
            }
        }
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; r++) v[r] = unpack_i16x2(cur[r]);
        wave_fft512<false>(v, lds, lane, tw);
        float2 zr[5];
        wave_lds_fence();
        pair_fetch_lds(v, lds, lane, zr);
#pragma unroll
        for (int d = 0; d < 5; d++) {
            const float2 ev = cadd_conj(v[d], zr[d]);
            const float2 od = csub_conj_mj(v[d], zr[d]);
            const float2 p = cmul(pw.w[d], od);
            const float2 xl = cadd(ev, p), xh = csub(ev, p);
            const float2 gl = make_float2(k.g_new * xl.x, k.g_new * xl.y), gh = make_float2(k.g_new * xh.x, k.g_new * xh.y);
#pragma unroll
            for (int e = 0; e < 2; e++) {
                acc_n[e][d] = cmac(acc_n[e][d], gl, h[e][d]);
                acc_n[e][5 + d] = cmac(acc_n[e][5 + d], gh, h[e][5 + d]);
            }
            if (faded) {
                const float2 ol = make_float2(k.g_old * xl.x, k.g_old * xl.y), oh = make_float2(k.g_old * xh.x, k.g_old * xh.y);
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    acc_o[e][d] = cmac(acc_o[e][d], ol, ho[e][d]);
                    acc_o[e][5 + d] = cmac(acc_o[e][5 + d], oh, ho[e][5 + d]);
                }
            }
        }
    }

    // both ears' accumulated spectra -> the 1024 samples of the segment, lane l holding the pairs (2 l + 128 d, +1)
    const auto inverse = [&](const float2 (&acc)[2][10], float2 (&ya)[8], float2 (&yb)[8]) {
        float2 ret[2][4];
#pragma unroll
        for (int d = 0; d < 5; d++) {
            if (d < 4) {
                presplit_inv_pair(acc[0][d], acc[0][5 + d], pw.w[d], ya[d], ret[0][d]);
                presplit_inv_pair(acc[1][d], acc[1][5 + d], pw.w[d], yb[d], ret[1][d]);
            } else {
                ya[d] = presplit_inv_reg(acc[0][d], acc[0][5 + d], pw.w[d]);
                yb[d] = presplit_inv_reg(acc[1][d], acc[1][5 + d], pw.w[d]);
            }
        }
        wave_lds_fence();
#pragma unroll
        for (int d = 0; d < 4; d++) { xchg_st(lds, 512 - lane - 64 * d, ret[0][d]); xchg_st(lds_b, 512 - lane - 64 * d, ret[1][d]); }
        wave_lds_fence();
#pragma unroll
        for (int d = 5; d < 8; d++) { ya[d] = xchg_ld(lds, lane + 64 * d); yb[d] = xchg_ld(lds_b, lane + 64 * d); }
        wave_lds_fence();
        wave_fft512_x2_staggered<true>(ya, yb, lds, lds_b, lane, tw);
    };
    float2 y[2][8];
    inverse(acc_n, y[0], y[1]);
    if (faded) {
        float2 o[2][8];
        inverse(acc_o, o[0], o[1]);
#pragma unroll
        for (int e = 0; e < 2; e++)
#pragma unroll
            for (int d = 4; d < 8; d++) {
                const float r0 = (float)(2 * lane + 128 * (d - 4)) * (1.0f / 512.0f), r1 = r0 + (1.0f / 512.0f);
                y[e][d].x = fmaf(r0, y[e][d].x, (1.0f - r0) * o[e][d].x);
                y[e][d].y = fmaf(r1, y[e][d].y, (1.0f - r1) * o[e][d].y);
            }
    }
    // samples 512..1023 leave from the registers: blocks are 512 long, plane and the bases even, so every pair is a dword
#pragma unroll
    for (int e = 0; e < 2; e++) {
        if (out_i16) {
            unsigned int *o32 = reinterpret_cast<unsigned int *>(out_i16 + (size_t)e * plane + 512 * j) + lane;
#pragma unroll
            for (int d = 4; d < 8; d++) __builtin_nontemporal_store(cast_i16x2_bits(y[e][d].x, y[e][d].y), o32 + 64 * (d - 4));
        }
        if (out_f32) {
            float2 *of = reinterpret_cast<float2 *>(out_f32 + (size_t)e * plane + 512 * j) + lane;
#pragma unroll
            for (int d = 4; d < 8; d++) of[64 * (d - 4)] = y[e][d];
        }
    }
}

// One thread per chunk: the chunk's mix is the last m with chunk_first[m] <= c; a mix without blocks changes nothing.
__global__ void binaural_commit_kernel(const long long *__restrict__ stream_id, const long long *__restrict__ chunk_first,
                                       const long long *__restrict__ block_first, long n_mixes, long n_chunks,
                                       long n_streams, int *__restrict__ parity)
{
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    long m = 0, hi = n_mixes;
    while (hi - m > 1) {
        const long mid = (m + hi) >> 1;
        if (chunk_first[mid] <= c) m = mid;
        else hi = mid;
    }
    if (block_first[m + 1] > block_first[m]) parity[clamp_idx(stream_id[c], n_streams)] ^= 1;
}

// One workgroup per listed stream: both copies of its history silent, nothing carried, not started.
__global__ void binaural_reset_kernel(const long long *__restrict__ stream_id, BinauralStreams st)
{
    const long s = clamp_idx(stream_id[blockIdx.x], st.n_streams);
    for (int p = 0; p < 2; p++) {
        const long at = (long)p * st.n_streams + s;
        unsigned int *h = reinterpret_cast<unsigned int *>(st.hist + at * 512);
        for (int i = threadIdx.x; i < 256; i += blockDim.x) h[i] = 0u;
        if (threadIdx.x == 0) st.dir[at] = 0, st.gain[at] = 0.f, st.started[at] = 0;
    }
}

__global__ void binaural_bank_kernel(const double2 *__restrict__ spec, float2 *__restrict__ bank, long rows)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * 640) return;
    const long row = i / 640;
    const int q = (int)(i % 640) >> 6, l = (int)(i & 63);
    const double2 v = spec[row * 1024 + l + 64 * (q % 5) + 512 * (q / 5)];
    // the render kernel's forward transform is unscaled: the split's 1/2 and the inverse's 1/1024 live here (exact)
    bank[i] = make_float2((float)v.x * (1.0f / 2048.0f), (float)v.y * (1.0f / 2048.0f));
}

// ---------------------------------------------------------------------------------------------------------------
int launch_binaural_bank(hipStream_t s, const double2 *spec, float2 *bank, long rows)
{
    const long n = rows * 640;
    hipLaunchKernelGGL(binaural_bank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, spec, bank, rows);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_binaural_render(hipStream_t s, const short *pcm, const long long *stream_id, const long long *sample_first,
                           const int *dir, const float *gain, const long long *chunk_first, const long long *block_first,
                           long n_mixes, long n_chunks, long n_blocks_total, const float2 *bank, int n_dirs,
                           const float2 *table, const BinauralStreams &st, int *parity, short *out_i16, float *out_f32,
                           long plane)
{
    hipLaunchKernelGGL(binaural_render_kernel, dim3((unsigned)n_blocks_total), dim3(64), 0, s, pcm, stream_id, sample_first,
                       dir, gain, chunk_first, block_first, n_mixes, bank, n_dirs, table, parity, st, out_i16, out_f32, plane);
    if (n_chunks > 0)
        hipLaunchKernelGGL(binaural_commit_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, s, stream_id,
                           chunk_first, block_first, n_mixes, n_chunks, st.n_streams, parity);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_binaural_reset(hipStream_t s, const long long *stream_id, long n_ids, const BinauralStreams &st)
{
    if (n_ids > 0) hipLaunchKernelGGL(binaural_reset_kernel, dim3((unsigned)n_ids), dim3(256), 0, s, stream_id, st);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
