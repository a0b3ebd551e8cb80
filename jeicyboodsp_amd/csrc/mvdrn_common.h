// mvdrn_common.h -- the device helpers the n-microphone MVDR kernels of a stream (mvdrn_kernels.hip) and of a batch of
// ragged utterances (mvdrn_batch_kernels.hip) share: the 513-bin spectrum of a frame, complex FP64 on (re, im) pairs,
// and the covariance row update.  Moved here from mvdrn_kernels.hip as they stood; the kernels of that file compile to
// what they did (profiles/r21_mvdrn_batch_isa.txt).
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

}  // namespace jdsp
