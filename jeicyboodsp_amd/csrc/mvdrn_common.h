// mvdrn_common.h -- the device code the n-microphone MVDR kernels of a stream (mvdrn_kernels.hip), of a batch of
// ragged utterances (mvdrn_batch_kernels.hip) and of live streams (mvdrn_live_kernels.hip) share as functions: the 513-bin spectrum of a frame and its store, complex
// FP64 on (re, im) pairs, the covariance row update and its sum over an event range, and the emit of a beamformed block.
// Each is called once per kernel, with what differs between a stream and a batch (addresses, chunk lookup) left to the
// caller.  The two long bodies, the walk with its solve and the beamformed frame, are shared as text:
// mvdrn_walk_body.h, mvdrn_frame_body.h (profiles/r25_mvdrn_one_walk.txt).
#pragma once
#include "frame_io.h"

namespace jdsp {

constexpr int kMvnBins = 513;

__device__ __forceinline__ void mvn_spectrum(float2 (&v)[8], float2 *lds, int lane, const WaveTwiddles &tw,
                                             const float2 *wsp, float2 (&lo)[8], float2 (&hi)[8])
{
    wave_fft512<false>(v, lds, lane, tw);
    store_natural_image(lds, lane, v);
    wave_lds_fence();
#define JDSP_SPLIT(J)                                                                          \
    {                                                                                          \
        const int m = 128 * J + 2 * lane;                                                      \
        const float4 zz = *reinterpret_cast<const float4 *>(&lds[m]);                          \
        float2 zr0, zr1; load_mirror_pair(lds, m, zr0, zr1);                           \
        split_fwd<J>(make_float2(zz.x, zz.y), zr0, wsp[0], lo[2 * J], hi[2 * J]);             \
        split_fwd<J>(make_float2(zz.z, zz.w), zr1, wsp[1], lo[2 * J + 1], hi[2 * J + 1]);     \
    }
    JDSP_SPLIT(0) JDSP_SPLIT(1) JDSP_SPLIT(2) JDSP_SPLIT(3)
#undef JDSP_SPLIT
    wave_lds_fence();
}

// ---- complex FP64 helpers on (re, im) pairs
struct cd { double x, y; };
__device__ __forceinline__ cd cd_mul(cd a, cd b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cd cd_sub(cd a, cd b) { return {a.x - b.x, a.y - b.y}; }

__device__ __forceinline__ cd cd_of(double2 a) { return {a.x, a.y}; }
__device__ __forceinline__ double2 d2_of(cd a) { return make_double2(a.x, a.y); }
// 1 / a with one reciprocal: hardware estimate + two Newton steps (relative error ~1e-16: the weights are stored as FP32)
__device__ __forceinline__ cd cd_inv_fast(cd a)
{
    const double d = a.x * a.x + a.y * a.y;
    double y = __builtin_amdgcn_rcp(d);
    y = y * (2.0 - d * y);
    y = y * (2.0 - d * y);
    return {a.x * y, -a.y * y};
}

// this lane's spectrum value to its group, the group's eight back: row[c] += X_r conj(X_c) / N   (N a power of two: exact)
__device__ __forceinline__ void mvn_row_add(cd (&row)[8], float2 xr, float2 *xs, int r, double inv_n)
{
    wave_lds_fence();
    xs[r] = xr;
    wave_lds_fence();
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 two = *reinterpret_cast<const float4 *>(&xs[2 * q]);
        row[2 * q].x += ((double)xr.x * two.x + (double)xr.y * two.y) * inv_n;
        row[2 * q].y += ((double)xr.y * two.x - (double)xr.x * two.y) * inv_n;
        row[2 * q + 1].x += ((double)xr.x * two.z + (double)xr.y * two.w) * inv_n;
        row[2 * q + 1].y += ((double)xr.y * two.z - (double)xr.x * two.w) * inv_n;
    }
}

// S = the sum of X X^H / N over the events [e0, e1) (this lane's row of it), event e + 1 requested while e is added.
// grp, r: lane >> 3, lane & 7, from the caller, who addresses its store with them (worked out again from the lane here,
// mvdrn_chunk_sums_kernel came out a VGPR granule smaller than it was)
__device__ __forceinline__ void mvn_range_sum(cd (&S)[8], int grp, int r, const float2 *__restrict__ spec, int e0, int e1,
                                              int n_mics, int n_bins, int k, double inv_n)
{
    __shared__ __attribute__((aligned(16))) float2 sx[8][8];
#pragma unroll
    for (int c = 0; c < 8; c++) S[c] = {0.0, 0.0};
    float2 xr = make_float2(0.f, 0.f);
    if (r < n_mics && e0 < e1) xr = spec[((size_t)e0 * n_mics + r) * n_bins + k];
    for (int e = e0; e < e1; e++) {
        const float2 x = xr;
        if (r < n_mics && e + 1 < e1) xr = spec[((size_t)(e + 1) * n_mics + r) * n_bins + k];
        mvn_row_add(S, x, sx[grp], r, inv_n);
    }
}

// The estimation frame's spectrum from its sample pairs (relayout_half's layout) and its store: dst[k] = X[k], k = 0..512
__device__ __forceinline__ void mvn_event_spectrum(const unsigned int (&raw)[8], float2 *lds, int lane, const WaveTwiddles &tw,
                                                   const float2 *wsp, float2 *__restrict__ dst)
{
    float2 v[8], lo[8], hi[8];
#pragma unroll
    for (int r = 0; r < 8; r++) { const float2 s = unpack_i16x2(raw[r]); v[r] = make_float2(0.5f * s.x, 0.5f * s.y); }
    mvn_spectrum(v, lds, lane, tw, wsp, lo, hi);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        dst[128 * q + 2 * lane] = lo[2 * q];
        dst[128 * q + 2 * lane + 1] = lo[2 * q + 1];
    }
    if (lane == 0) dst[512] = hi[0];
}

// Samples 511..1022 of the frame, scaled, as int16 at o[0..511] and before the cast at pc[0..511] (pc may be null; o only
// where the entry lets it: OUT_OPTIONAL)
template <bool OUT_OPTIONAL>
__device__ __forceinline__ void mvn_emit_block(const float2 (&y)[8], int lane, short *__restrict__ o, float *__restrict__ pc)
{
#pragma unroll
    for (int dd = 0; dd < 8; dd++) {
        const int i0 = 2 * lane + 128 * dd - 511;
        const float s0 = y[dd].x * (1.0f / 1024.0f), s1 = y[dd].y * (1.0f / 1024.0f);
        if (i0 >= 0 && i0 < 512) { if (!OUT_OPTIONAL || o) o[i0] = (short)cast_i16_bits(s0); if (pc) pc[i0] = s0; }
        if (i0 + 1 >= 0 && i0 + 1 < 512) { if (!OUT_OPTIONAL || o) o[i0 + 1] = (short)cast_i16_bits(s1); if (pc) pc[i0 + 1] = s1; }
    }
}

}  // namespace jdsp
