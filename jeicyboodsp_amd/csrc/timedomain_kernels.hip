// timedomain_kernels.hip -- the reference's time-domain analysis programs on gfx950, one frame per wavefront:
//   PitchEstimation_method2.cpp:69-101  CalcPitch, AMDF             sum |x[i] - x[i+k]| / (1024 - k), arg min
//   PitchEstimation_method3.cpp:69-101  CalcPitch, autocorrelation  sum  x[i] * x[i+k]  / (1024 - k), arg max
//   LPCEstimation.cpp:87-137            Hamming window, 13 autocorrelation lags, Toeplitz solve
// Frame b = [block b-1, block b]; block -1 is prev_block (NULL: zeros, the reference's initial keep buffer).
//
// Both pitch sums are integers that the reference holds in a double without ever rounding (|x - y| sums stay below
// 2^26, products below 2^40), so ANY order of summation gives the reference's bits: the AMDF sum is kept in a u32
// (v_sad_u16 on pairs of samples biased by 0x8000), the autocorrelation in FP64 FMAs.  One IEEE division by
// (double)(1024 - k) follows, as the reference's `/=` does.
#include "jdsp_internal.h"

namespace jdsp {

// ---- pitch: lane l owns the eight consecutive lags base + 8 l .. + 7 ---------------------------------------------
// The frame lies in LDS followed by zeros up to sample 1536: the sum over i < 1024 - k runs to a bound common to the
// wave (1024, or 928 when only the lags from 96 up are wanted), and x[i + k] past the frame is a zero.  For the
// autocorrelation those terms vanish; for the AMDF they add |x[i]| for 1024 - k <= i < bound, a difference of two
// suffix sums of |x|: taken off at the end from a table of them (tail[]).
// Template flag CURVE: all 512 lags (base 0, i < 1024); otherwise lags 96 .. 511 on lanes 0 .. 51 (i < 928).
constexpr int kTdLags = 8;

__device__ __forceinline__ void td_unpack8(const uint4 r, int (&s)[8])
{
    const unsigned int w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        s[2 * q] = (int)(short)(w[q] & 0xffffu);
        s[2 * q + 1] = (int)w[q] >> 16;
    }
}

// this lane's eight samples of block b-1 (prev_block, or zeros, before the first) and of block b
__device__ __forceinline__ void td_load_frame(const short *pcm, const short *prev_block, long b, int lane, uint4 &r0, uint4 &r1)
{
    const uint4 *p0 = b > 0 ? reinterpret_cast<const uint4 *>(pcm + (b - 1) * 512) : reinterpret_cast<const uint4 *>(prev_block);
    const uint4 *p1 = reinterpret_cast<const uint4 *>(pcm + b * 512);
    r0 = p0 ? p0[lane] : make_uint4(0u, 0u, 0u, 0u);
    r1 = p1[lane];
}

// dAutoCorrelation[k] = sum / (1024 - k) (:83) for this lane's lags, then the scan :87-95 from lag 511 down to 101 with
// <= (>=): the smallest (largest) value wins and ties go to the SMALLEST lag.  key = the value, negated for the arg
// max (exact).
template <bool CURVE, bool ARGMAX>
__device__ __forceinline__ void td_finish(const double (&sum)[kTdLags], int k0, int lane, long b, int *arg, double *value, double *curve)
{
    double best = INFINITY, c[kTdLags];
    int at = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < kTdLags; j++) {
        const int k = k0 + j;
        c[j] = sum[j] / (double)(1024 - k);
        const double key = ARGMAX ? -c[j] : c[j];
        const bool t = (k > 100) & (k < 512) & ((key < best) | ((key == best) & (k < at)));
        best = t ? key : best;
        at = t ? k : at;
    }
    if (CURVE) {
        double2 *row = reinterpret_cast<double2 *>(curve + b * 512 + k0);
#pragma unroll
        for (int q = 0; q < 4; q++) row[q] = make_double2(c[2 * q], c[2 * q + 1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(at, o);
        const bool t = (ob < best) | ((ob == best) & (oa < at));
        best = t ? ob : best;
        at = t ? oa : at;
    }
    if (lane == 0) {
        if (arg) arg[b] = at;
        if (value) value[b] = ARGMAX ? -best : best;
    }
}

// Autocorrelation: FP64 FMAs.  The image holds doubles in groups of eight padded to 80 B: lane l reads group g0 + l
// with ds_read_b128, and that stride puts the sixteen lanes of every b128 lane group on sixteen different 16-B slots
// of the 256-B bank row.  A step takes eight values of i (a[c] = x[i0 + c], the same address in every lane) against the
// sixteen samples x[i0 + k0 ..] (lo, hi): 64 FMAs on 8 + 8 loaded doubles, the window's other half kept from the step
// before.
constexpr int kAcfStride = 10, kAcfGroups = 192;       // 1536 samples: the longest reach is 1008 + 504 + 23 = 912 + 600 + 23

__device__ __forceinline__ void acf_load8(const double *g, double (&v)[8])
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const double2 t = *reinterpret_cast<const double2 *>(g + 2 * q);
        v[2 * q] = t.x;
        v[2 * q + 1] = t.y;
    }
}

__device__ __forceinline__ void acf_step(double (&acc)[kTdLags], const double (&a)[8], const double (&lo)[8], const double (&hi)[8])
{
#pragma unroll
    for (int c = 0; c < 8; c++)
#pragma unroll
        for (int j = 0; j < kTdLags; j++) acc[j] = __builtin_fma(a[c], c + j < 8 ? lo[c + j] : hi[c + j - 8], acc[j]);
}

template <bool CURVE>
__global__ __launch_bounds__(64) void pitch_acf_kernel(const short *__restrict__ pcm, long n_blocks,
                                                       const short *__restrict__ prev_block, int *__restrict__ arg,
                                                       double *__restrict__ value, double *__restrict__ curve)
{
    constexpr int S = kAcfStride, kBase = CURVE ? 0 : 96, kEnd = 1024 - kBase;
    __shared__ __attribute__((aligned(16))) double x[kAcfGroups * S];
    const int lane = threadIdx.x;
    const long per_xcd = (gridDim.x + 7) >> 3;                // XCD-aware block order (speed only)
    const long b = (long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (b >= n_blocks) return;
    uint4 r0, r1;
    td_load_frame(pcm, prev_block, b, lane, r0, r1);
    int s0[8], s1[8];
    td_unpack8(r0, s0);
    td_unpack8(r1, s1);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        x[lane * S + q] = (double)s0[q];
        x[(64 + lane) * S + q] = (double)s1[q];
        x[(128 + lane) * S + q] = 0.0;
    }
    __syncthreads();

    const int k0 = kBase + kTdLags * lane;
    double acc[kTdLags];
#pragma unroll
    for (int j = 0; j < kTdLags; j++) acc[j] = 0.0;
    const double *xa = x, *xw = x + (k0 >> 3) * S;
    double a[8], h0[8], h1[8];
    acf_load8(xw, h0);
    for (int i0 = 0; i0 < kEnd; i0 += 16) {
        acf_load8(xw + S, h1);
        acf_load8(xa, a);
        acf_step(acc, a, h0, h1);
        acf_load8(xw + 2 * S, h0);
        acf_load8(xa + S, a);
        acf_step(acc, a, h1, h0);
        xa += 2 * S;
        xw += 2 * S;
    }
    td_finish<CURVE, true>(acc, k0, lane, b, arg, value, curve);
}

// AMDF: v_sad_u16 on pairs of samples biased by 0x8000, two terms per instruction into a u32.  p0[m] = (x[2m], x[2m+1]),
// p1[m] = (x[2m+1], x[2m+2]): the pair (x[i], x[i+1]), i even, meets (x[i+k], x[i+k+1]) out of p0 for an even lag and
// out of p1 for an odd one.  A step takes sixteen values of i (eight pairs, the same address in every lane) against
// twelve dwords of each image; lane l reads them at 16 l bytes from the wave's base, consecutive 16-B slots.
constexpr int kAmdfPairs = 768;                        // 1536 samples: the longest reach is (1008 + 504) / 2 + 11

template <bool CURVE>
__global__ __launch_bounds__(64) void pitch_amdf_kernel(const short *__restrict__ pcm, long n_blocks,
                                                        const short *__restrict__ prev_block, int *__restrict__ arg,
                                                        double *__restrict__ value, double *__restrict__ curve)
{
    constexpr int kBase = CURVE ? 0 : 96, kEnd = 1024 - kBase;
    constexpr unsigned int kBias = 0x80008000u;
    __shared__ __attribute__((aligned(16))) unsigned int p0[kAmdfPairs + 4], p1[kAmdfPairs];
    __shared__ unsigned int tail[513];
    const int lane = threadIdx.x;
    const long per_xcd = (gridDim.x + 7) >> 3;                // XCD-aware block order (speed only)
    const long b = (long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (b >= n_blocks) return;
    uint4 r0, r1;
    td_load_frame(pcm, prev_block, b, lane, r0, r1);
    reinterpret_cast<uint4 *>(p0)[lane] = make_uint4(r0.x ^ kBias, r0.y ^ kBias, r0.z ^ kBias, r0.w ^ kBias);
    reinterpret_cast<uint4 *>(p0)[64 + lane] = make_uint4(r1.x ^ kBias, r1.y ^ kBias, r1.z ^ kBias, r1.w ^ kBias);
    reinterpret_cast<uint4 *>(p0)[128 + lane] = make_uint4(kBias, kBias, kBias, kBias);
    if (lane == 0) reinterpret_cast<uint4 *>(p0)[192] = make_uint4(kBias, kBias, kBias, kBias);
    {
        // tail[t] = sum of |x| over the last t samples of the frame, t <= 512: this lane's eight, then a suffix scan
        int s1[8];
        td_unpack8(r1, s1);
        unsigned int ab[8], run = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            ab[q] = (unsigned int)(s1[q] < 0 ? -s1[q] : s1[q]);
            run += ab[q];
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int up = __shfl_down(run, o);
            run += lane + o < 64 ? up : 0u;
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
            tail[512 - 8 * lane - q] = run;
            run -= ab[q];
        }
        if (lane == 0) tail[0] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 3; h++) {
        const int m = 256 * h + 4 * lane;
        const uint4 u = *reinterpret_cast<const uint4 *>(p0 + m);
        const unsigned int nx = p0[m + 4];
        *reinterpret_cast<uint4 *>(p1 + m) = make_uint4((u.x >> 16) | (u.y << 16), (u.y >> 16) | (u.z << 16),
                                                        (u.z >> 16) | (u.w << 16), (u.w >> 16) | (nx << 16));
    }
    __syncthreads();

    const int k0 = kBase + kTdLags * lane;
    unsigned int acc[kTdLags];
#pragma unroll
    for (int j = 0; j < kTdLags; j++) acc[j] = 0u;
    const uint4 *pa = reinterpret_cast<const uint4 *>(p0);
    const uint4 *w0 = reinterpret_cast<const uint4 *>(p0 + (k0 >> 1)), *w1 = reinterpret_cast<const uint4 *>(p1 + (k0 >> 1));
#pragma unroll 2
    for (int i0 = 0; i0 < kEnd; i0 += 16) {
        const uint4 a0 = pa[0], a1 = pa[1], e0 = w0[0], e1 = w0[1], e2 = w0[2], o0 = w1[0], o1 = w1[1], o2 = w1[2];
        const unsigned int a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const unsigned int ev[12] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w, e2.x, e2.y, e2.z, e2.w};
        const unsigned int od[12] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w, o2.x, o2.y, o2.z, o2.w};
#pragma unroll
        for (int c = 0; c < 8; c++)
#pragma unroll
            for (int j = 0; j < kTdLags; j++)
                acc[j] = __builtin_amdgcn_sad_u16(a[c], (j & 1) ? od[c + (j >> 1)] : ev[c + (j >> 1)], acc[j]);
        pa += 2;
        w0 += 2;
        w1 += 2;
    }
    double sum[kTdLags];
#pragma unroll
    for (int j = 0; j < kTdLags; j++) {
        const int k = k0 + j;
        // the terms kEnd > i >= 1024 - k met a zero: |x[i]| over the last k samples but the last kBase
        sum[j] = (double)(acc[j] - (tail[k < 512 ? k : 0] - tail[kBase]));
    }
    td_finish<CURVE, false>(sum, k0, lane, b, arg, value, curve);
}

int launch_pitch_lag(hipStream_t s, int method, const short *pcm, long n_blocks, const short *prev_block, int *arg,
                     double *value, double *curve)
{
    if (n_blocks <= 0) return 0;
    const dim3 grid((unsigned)((n_blocks + 7) / 8 * 8)), block(64);
    if (method == 2 && curve) hipLaunchKernelGGL((pitch_amdf_kernel<true>), grid, block, 0, s, pcm, n_blocks, prev_block, arg, value, curve);
    else if (method == 2) hipLaunchKernelGGL((pitch_amdf_kernel<false>), grid, block, 0, s, pcm, n_blocks, prev_block, arg, value, curve);
    else if (curve) hipLaunchKernelGGL((pitch_acf_kernel<true>), grid, block, 0, s, pcm, n_blocks, prev_block, arg, value, curve);
    else hipLaunchKernelGGL((pitch_acf_kernel<false>), grid, block, 0, s, pcm, n_blocks, prev_block, arg, value, curve);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- LPC ---------------------------------------------------------------------------------------------------------
// Lane l windows the N / 64 consecutive samples it loaded and sums, for every lag i <= 16, its own products
// y[j] y[j + i] in j order (zeros follow the frame in LDS: no ragged end); a fixed butterfly adds the 64 partial sums.
// The order of summation is a function of the frame alone, so a frame's output does not depend on its batch.
// The solve is Gaussian elimination with partial pivoting (rows stay in place: lane r < order holds row r of [T | v]
// in registers, the pivot row is read with v_readlane) and a back substitution, all in FP64.
__device__ __forceinline__ double td_bcast(double v, int uniform_lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), uniform_lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), uniform_lane);
    return __hiloint2double(hi, lo);
}

constexpr int kLpcMax = 16;

template <int N>
__global__ __launch_bounds__(64) void lpc_kernel(const short *__restrict__ pcm, long n_blocks, int order,
                                                 const short *__restrict__ prev_block, const double *__restrict__ win,
                                                 double *__restrict__ autocorr, double *__restrict__ lpc)
{
    constexpr int B = N / 2, PER = N / 64;
    __shared__ __attribute__((aligned(16))) double y[N + PER + kLpcMax];
    __shared__ double rs[kLpcMax + 1];
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    if (b >= n_blocks) return;
    const short *blk = lane < 32 ? (b > 0 ? pcm + (b - 1) * B : prev_block) : pcm + b * B;   // :100-101
    const uint4 *src = blk ? reinterpret_cast<const uint4 *>(blk + (lane & 31) * PER) : nullptr;
#pragma unroll
    for (int h = 0; h < PER / 8; h++) {
        int sv[8];
        td_unpack8(src ? src[h] : make_uint4(0u, 0u, 0u, 0u), sv);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int j = lane * PER + 8 * h + q;
            y[j] = (double)sv[q] * win[j];                                                    // :104-106
        }
    }
    if (lane < PER + kLpcMax) y[N + lane] = 0.0;
    __syncthreads();

    double yw[PER + kLpcMax], r[kLpcMax + 1];
#pragma unroll
    for (int q = 0; q < PER + kLpcMax; q++) yw[q] = y[lane * PER + q];
#pragma unroll
    for (int i = 0; i <= kLpcMax; i++) {                                                      // :108-113
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < PER; q++) s = __builtin_fma(yw[q], yw[q + i], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        r[i] = s / (double)(N - i);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i <= kLpcMax; i++) rs[i] = r[i];
    }
    if (autocorr && lane <= order) {
        double mine = r[0];
#pragma unroll
        for (int i = 1; i <= kLpcMax; i++) mine = lane == i ? r[i] : mine;
        autocorr[b * (order + 1) + lane] = mine;
    }
    __syncthreads();

    // row `lane` of the Toeplitz system (:115-123); columns past the order are zeros, rows past it take no part
    const bool row = lane < order;
    double m[kLpcMax], rhs = row ? -rs[lane + 1] : 0.0;
#pragma unroll
    for (int cidx = 0; cidx < kLpcMax; cidx++) {
        const int d = lane > cidx ? lane - cidx : cidx - lane;
        m[cidx] = (row && cidx < order) ? rs[d <= kLpcMax ? d : 0] : 0.0;
    }
    bool used = !row, bad = false;
    int piv_of[kLpcMax];
#pragma unroll
    for (int k = 0; k < kLpcMax; k++) {
        piv_of[k] = 0;
        if (k < order) {
            double cand = used ? -1.0 : __builtin_fabs(m[k]);
            int who = lane;
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                const double oc = __shfl_xor(cand, o);
                const int ow = __shfl_xor(who, o);
                const bool t = (oc > cand) | ((oc == cand) & (ow < who));
                cand = t ? oc : cand;
                who = t ? ow : who;
            }
            const int piv = __builtin_amdgcn_readfirstlane(who);
            piv_of[k] = piv;
            const double pv = td_bcast(m[k], piv);
            bad = bad | !(__builtin_isfinite(pv) && pv != 0.0);
            const double prhs = td_bcast(rhs, piv);
            if (lane == piv) used = true;
            const double f = used ? 0.0 : m[k] / pv;
#pragma unroll
            for (int cidx = k + 1; cidx < kLpcMax; cidx++) {
                const double pc = td_bcast(m[cidx], piv);
                m[cidx] = __builtin_fma(-f, pc, m[cidx]);
            }
            rhs = __builtin_fma(-f, prhs, rhs);
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int k = kLpcMax - 1; k >= 0; k--) {
        if (k < order) {
            const double xk = td_bcast((rhs - acc) / m[k], piv_of[k]);
            acc = __builtin_fma(m[k], xk, acc);
            if (lane == 0) lpc[b * order + k] = bad ? __builtin_nan("") : xk;
        }
    }
}

int launch_lpc(hipStream_t s, const short *pcm, long n_blocks, int block_len, int order, const short *prev_block,
               const double *win, double *autocorr, double *lpc)
{
    if (n_blocks <= 0) return 0;
    const dim3 grid((unsigned)n_blocks), block(64);
    if (block_len == 256) hipLaunchKernelGGL((lpc_kernel<512>), grid, block, 0, s, pcm, n_blocks, order, prev_block, win, autocorr, lpc);
    else hipLaunchKernelGGL((lpc_kernel<1024>), grid, block, 0, s, pcm, n_blocks, order, prev_block, win, autocorr, lpc);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
