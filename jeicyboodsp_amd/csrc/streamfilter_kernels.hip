// streamfilter_kernels.hip -- the reference's two sample-serial filters on gfx950, batched over independent streams:
//   7Band_GEQ.cpp:259-332   ApplyIirGEQ, a cascade of biquads whose every section output is cast to short
//   NormalLMS.cpp:96-136    LMSFilter, a normalised LMS step per sample
// Both are serial in time within a stream and FP64.  Every product and every sum below is rounded on its own, as the
// reference's x86-64 build rounds it: contraction into v_fma_f64 is switched off for the whole file, here and not in
// build_flags.txt, so every way of building this file agrees.
#pragma clang fp contract(off)
#include "jdsp_internal.h"

namespace jdsp {

// (short)double as the reference's build does it, for values inside int32: truncate, keep the low 16 bits.
__device__ __forceinline__ int sf_cast_i16(double v)
{
    return (int)(short)(__double2int_rz(v) & 0xffff);
}

template <int CTRL>
__device__ __forceinline__ int sf_dpp(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}

template <int CTRL>
__device__ __forceinline__ double sf_dpp_f64(double v)
{
    return __hiloint2double(sf_dpp<CTRL>(__double2hiint(v)), sf_dpp<CTRL>(__double2loint(v)));
}

// ---- equaliser -----------------------------------------------------------------------------------------------------
// A stream owns G adjacent lanes of one DPP row (G = 2, 4, 8 or 16, the smallest that holds the sections); lane k of the
// group is section k and at step s computes sample t = s - k, so a call of n samples takes n + n_sections - 1 steps.
// The accumulation is the reference's (:280-283 with the coefficient index running down):
//   d = 0; d += b2 in[t-2]; d -= a2 out[t-2]; d += b1 in[t-1]; d -= a1 out[t-1]; d += b0 in[t];   out[t] = (short)d
// (its sixth term a0 out[t] is 0.0 * 0).  Walking samples outside and sections inside gives the same values as the
// reference's sections-outside order because a section reads nothing but its own history and the section before it.
// A section's freshly cast output reaches the next lane with one row_shr:1 DPP move at the top of the next step.
// state: [n_streams][n_sections + 1][2] int16, {older, newer}; row 0 the input's last two samples, row k + 1 the last
// two outputs of section k (= the input keep of section k + 1, 7Band_GEQ.cpp:288-300).

// the head of a section's sum, the three terms that are known a step early: ((0 + b2 in[t-2]) - a2 out[t-2]) + b1 in[t-1]
__device__ __forceinline__ double geq_part(double b2, double a2, double b1, int in2, int out2, int in1)
{
    double d = 0.0;
    d += b2 * (double)in2;
    d -= a2 * (double)out2;
    d += b1 * (double)in1;
    return d;
}

template <int G>
__global__ __launch_bounds__(64) void geq_cascade_kernel(const short *__restrict__ pcm, long n_streams, long n, long pitch,
                                                         const double *__restrict__ coeff, int n_sections,
                                                         short *__restrict__ state, short *__restrict__ out,
                                                         double *__restrict__ precast)
{
    const int lane = threadIdx.x, k = lane & (G - 1);
    const long stream = (long)blockIdx.x * (64 / G) + lane / G;
    const bool live = stream < n_streams && k < n_sections;
    const long n_mine = live ? n : 0;                        // a lane without a section never becomes active
    const bool first = k == 0, last = k == n_sections - 1;

    double b0 = 0, b1 = 0, b2 = 0, a1 = 0, a2 = 0;
    int in1 = 0, in2 = 0, out1 = 0, out2 = 0;
    short *st = nullptr;
    if (live) {
        const double *c = coeff + k * 6;                     // [section][b | a][3]
        b0 = c[0], b1 = c[1], b2 = c[2], a1 = c[4], a2 = c[5];
        st = state + (stream * (n_sections + 1) + k) * 2;
        in2 = st[0], in1 = st[1], out2 = st[2], out1 = st[3];
    }
    const short *src = pcm + stream * pitch;
    short *dst = out + stream * pitch;
    double *pdst = precast ? precast + stream * pitch : nullptr;

    // eight raw samples of lane 0, loaded one chunk ahead of their use; a chunk that crosses n is loaded by element
    auto load8 = [&](long t0) -> uint4 {
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if (!(live && first) || t0 >= n) return r;
        if (t0 + 8 <= n) return *reinterpret_cast<const uint4 *>(src + t0);
        unsigned int w[4] = {0u, 0u, 0u, 0u};
        for (int q = 0; q < 8 && t0 + q < n; q++) w[q >> 1] |= (unsigned int)(unsigned short)src[t0 + q] << (16 * (q & 1));
        return make_uint4(w[0], w[1], w[2], w[3]);
    };

    const long steps = n + n_sections - 1;
    double part = geq_part(b2, a2, b1, in2, out2, in1);
    uint4 cur = load8(0);
    unsigned int g0 = 0, g1 = 0, g2 = 0, g3 = 0;             // the last eight outputs, oldest in the low half of g0
    int fresh = 0;                                           // this lane's output of the step before
    for (long s0 = 0; s0 < steps; s0 += 8) {
        const uint4 nxt = load8(s0 + 8);
        const unsigned int raw[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const long t = s0 + j - k;
            const int mine = (int)(short)(raw[j >> 1] >> (16 * (j & 1)));
            const int from_prev = sf_dpp<0x111>(fresh);      // row_shr:1
            const int x = first ? mine : from_prev;
            const bool active = t >= 0 && t < n_mine;
            // only the a1 and b0 terms wait for the step before; `part` was formed ahead of them (same order of additions)
            double d = part;
            d -= a1 * (double)out1;
            d += b0 * (double)x;
            const int y = sf_cast_i16(d);
            // an inactive lane keeps its state (selects, no branch: the next step's `part` overlaps this step's chain)
            in2 = active ? in1 : in2, in1 = active ? x : in1, out2 = active ? out1 : out2, out1 = active ? y : out1;
            fresh = active ? y : fresh;
            g0 = active ? (g0 >> 16) | (g1 << 16) : g0, g1 = active ? (g1 >> 16) | (g2 << 16) : g1;
            g2 = active ? (g2 >> 16) | (g3 << 16) : g2, g3 = active ? (g3 >> 16) | ((unsigned int)y << 16) : g3;
            part = geq_part(b2, a2, b1, in2, out2, in1);
            if (active && last) {
                if (pdst) pdst[t] = d;
                if ((t & 7) == 7) *reinterpret_cast<uint4 *>(dst + (t - 7)) = make_uint4(g0, g1, g2, g3);
            }
        }
        cur = nxt;
    }
    if (live && last && (n & 7)) {                           // the store tail: the n % 8 newest of the gathered eight
        const int r = (int)(n & 7);
        const unsigned int g[4] = {g0, g1, g2, g3};
        for (int q = 8 - r; q < 8; q++) dst[n - 8 + q] = (short)(g[q >> 1] >> (16 * (q & 1)));
    }
    if (live && n > 0) {
        if (first) st[0] = (short)in2, st[1] = (short)in1;
        st[2] = (short)out2, st[3] = (short)out1;
    }
}

int launch_geq(hipStream_t s, const short *pcm, long n_streams, long n_samples, long pitch, const double *coeff,
               int n_sections, short *state, short *out, double *precast)
{
    if (n_streams <= 0 || n_samples <= 0) return 0;
    const int g = n_sections <= 2 ? 2 : n_sections <= 4 ? 4 : n_sections <= 8 ? 8 : 16;
    const long per_wave = 64 / g;
    const dim3 grid((unsigned)((n_streams + per_wave - 1) / per_wave)), block(64);
#define JDSP_GEQ_LAUNCH(G) \
    hipLaunchKernelGGL((geq_cascade_kernel<G>), grid, block, 0, s, pcm, n_streams, n_samples, pitch, coeff, n_sections, state, out, precast)
    if (g == 2) JDSP_GEQ_LAUNCH(2);
    else if (g == 4) JDSP_GEQ_LAUNCH(4);
    else if (g == 8) JDSP_GEQ_LAUNCH(8);
    else JDSP_GEQ_LAUNCH(16);
#undef JDSP_GEQ_LAUNCH
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- NLMS ----------------------------------------------------------------------------------------------------------
// One wavefront per stream, L = 64 T taps.  With x the kept L - 1 samples followed by the call's, sample i is
//   sum  = sum over j < L of c[L-1-j] x[i+j]                                             (:112-114)
//   est  = (short)sum,  e = ref[i] - est (int),  err = (short)e                           (:115-116)
//   c[m] += ((2.0 x[i+m]) MU) (double)e / (norm_i + COMPENSATION),  norm_i = sum x[i+j]^2 (:118-126)
// The dot product is the one sum whose order is ours to fix; it is a function of L alone:
//   lane l adds the products j = T l .. T l + T - 1 in ascending j, then six pairwise stages join lanes at distance
//   1, 2, 4, 8 (DPP inside the row), 16 and 32 (v_permlane16_swap, v_permlane32_swap).
// IEEE addition commutes, so both partners of a pair, and in the end all 64 lanes, hold the same bits.  The sum reaches
// the rest of the step only through its cast to short; norm_i is an integer below 2^53, exact in any order (taken from
// 64-bit prefix sums of x^2); the tap update is elementwise with a correctly rounded division.
// Lane l keeps the T coefficients its products use, c[L-1-j]; their update reads x[i + L-1-j].
// A call is walked in chunks of kNlmsChunk samples staged in LDS; nothing about the arithmetic depends on the chunk.
constexpr int kNlmsChunk = 256;

// own + the partner's value at lane distance 16 / 32: the swap leaves {own, partner} in one order in half of the lanes
// and in the other order in the other half, and the sum does not care
__device__ __forceinline__ double sf_add_swap16(double v)
{
    const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(v), __double2loint(v), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(v), __double2hiint(v), false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ double sf_add_swap32(double v)
{
    const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(v), __double2loint(v), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(v), __double2hiint(v), false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}

template <int T>
__global__ __launch_bounds__(64) void nlms_kernel(const short *__restrict__ input, const short *__restrict__ refsig,
                                                  long n, long pitch, double mu, double compensation,
                                                  double *__restrict__ coef, short *__restrict__ keep,
                                                  short *__restrict__ est, short *__restrict__ err,
                                                  double *__restrict__ precast)
{
    constexpr int L = 64 * T, K = L - 1, C = kNlmsChunk, W = K + C;      // W staged samples per chunk
    constexpr int PER = (W + 63) / 64;
    __shared__ short xs[W + T + 1];
    __shared__ short rs[C], es[C], ers[C];
    __shared__ double nc[C];
    __shared__ unsigned long long pre[64 * PER + 1];         // prefix sums of x^2; then the chunk's pre-cast sums
    const int lane = threadIdx.x;
    const long stream = blockIdx.x;
    const short *xin = input + stream * pitch, *rin = refsig + stream * pitch;
    short *kp = keep + stream * K;
    double *cf = coef + stream * L;

    double c[T];
#pragma unroll
    for (int q = 0; q < T; q++) c[q] = cf[L - 1 - (T * lane + q)];
    if (lane <= T) xs[W + lane] = 0;

    for (long c0 = 0; c0 < n; c0 += C) {
        const int cn = (int)(n - c0 < C ? n - c0 : C);
        // stage: xs[p] = sample c0 - K + p of the call (negative positions: the keep), zero past the chunk
        unsigned long long part = 0;
#pragma unroll
        for (int r = 0; r < PER; r++) {
            const int p = lane * PER + r;
            int v = 0;
            if (p < K + cn) {
                const long pos = c0 - K + p;
                v = pos < 0 ? kp[K + pos] : xin[pos];
            }
            if (p < W) xs[p] = (short)v;
            part += (unsigned long long)((long long)v * v);
        }
        for (int p = lane; p < C; p += 64) rs[p] = p < cn ? rin[c0 + p] : (short)0;
        unsigned long long incl = part;                      // inclusive scan of the lanes' sums
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(incl, o);
            incl += lane >= o ? up : 0ull;
        }
        __syncthreads();
        {
            unsigned long long run = incl - part;            // sum of x^2 over xs[0 .. lane PER)
#pragma unroll
            for (int r = 0; r < PER; r++) {
                const int p = lane * PER + r;
                pre[p] = run;
                const int v = p < W ? xs[p] : 0;
                run += (unsigned long long)((long long)v * v);
            }
            if (lane == 63) pre[64 * PER] = run;
        }
        __syncthreads();
        for (int p = lane; p < C; p += 64) nc[p] = (double)(pre[p + L] - pre[p]) + compensation;   // :118-121, :125
        __syncthreads();
        double *pc = reinterpret_cast<double *>(pre);

        // the serial loop; the windows of step i + 1 are read while step i computes
        int xd[T], xu[T];
#pragma unroll
        for (int q = 0; q < T; q++) xd[q] = xs[T * lane + q], xu[q] = xs[L - 1 - T * lane - q];
        for (int i = 0; i < cn; i++) {
            int nd[T], nu[T];
#pragma unroll
            for (int q = 0; q < T; q++) nd[q] = xs[i + 1 + T * lane + q], nu[q] = xs[i + 1 + L - 1 - T * lane - q];
            const double nrm = nc[i];
            const int rv = rs[i];
            double g[T];
#pragma unroll
            for (int q = 0; q < T; q++) g[q] = (2.0 * (double)xu[q]) * mu;
            double sum = c[0] * (double)xd[0];
#pragma unroll
            for (int q = 1; q < T; q++) sum += c[q] * (double)xd[q];
            sum += sf_dpp_f64<0xB1>(sum);                    // quad_perm [1,0,3,2]: distance 1
            sum += sf_dpp_f64<0x4E>(sum);                    // quad_perm [2,3,0,1]: distance 2
            sum += sf_dpp_f64<0x141>(sum);                   // row_half_mirror: the other quad of the eight (all four equal)
            sum += sf_dpp_f64<0x140>(sum);                   // row_mirror: the other eight of the row
            sum = sf_add_swap16(sum);
            sum = sf_add_swap32(sum);
            const int e_hat = sf_cast_i16(sum);
            const int e = rv - e_hat;
            const double ed = (double)e;
#pragma unroll
            for (int q = 0; q < T; q++) c[q] += (g[q] * ed) / nrm;
            if (lane == 0) {
                es[i] = (short)e_hat;
                ers[i] = (short)e;
                pc[i] = sum;
            }
#pragma unroll
            for (int q = 0; q < T; q++) xd[q] = nd[q], xu[q] = nu[q];
        }
        __syncthreads();
        for (int p = lane; p < cn; p += 64) {
            est[stream * pitch + c0 + p] = es[p];
            err[stream * pitch + c0 + p] = ers[p];
            if (precast) precast[stream * pitch + c0 + p] = pc[p];
        }
        __syncthreads();
    }

#pragma unroll
    for (int q = 0; q < T; q++) cf[L - 1 - (T * lane + q)] = c[q];
    // the new keep: the last K samples of (keep, call); read all of it before any of it is written
    short nk[T];
#pragma unroll
    for (int r = 0; r < T; r++) {
        const int p = lane + 64 * r;
        const long pos = n - K + p;
        nk[r] = p < K ? (pos < 0 ? kp[K + pos] : xin[pos]) : (short)0;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < T; r++) {
        const int p = lane + 64 * r;
        if (p < K) kp[p] = nk[r];
    }
}

int launch_nlms(hipStream_t s, const short *input, const short *refsig, long n_streams, long n_samples, long pitch,
                int filter_len, double mu, double compensation, double *coef, short *keep, short *est, short *err,
                double *precast)
{
    if (n_streams <= 0 || n_samples <= 0) return 0;
    const dim3 grid((unsigned)n_streams), block(64);
#define JDSP_NLMS_LAUNCH(T) \
    hipLaunchKernelGGL((nlms_kernel<T>), grid, block, 0, s, input, refsig, n_samples, pitch, mu, compensation, coef, keep, est, err, precast)
    if (filter_len == 64) JDSP_NLMS_LAUNCH(1);
    else if (filter_len == 128) JDSP_NLMS_LAUNCH(2);
    else JDSP_NLMS_LAUNCH(4);
#undef JDSP_NLMS_LAUNCH
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
