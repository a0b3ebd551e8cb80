// stftmask_kernels.hip -- fused STFT masking (gfx950): PCM -> analysis window -> forward transform -> per-bin mask ->
// inverse transform -> synthesis window -> overlap-add -> (short), one streaming pass (include/jdsp.h, jdsp_stftmask_*).
// The spectrum never leaves the wave: what the unfused route (jdsp_stft_* -> multiply -> jdsp_istft_*) writes to HBM,
// multiplies there and reads back stays in registers and the wave's LDS scratch.
//
// The kernel joins two that exist.  The frame is denoise_frame_pairs' (denoise_kernels.hip): one 512-point complex
// transform of the packed real frame, the split with every mirror pair of bins owned by one lane (frame_io.h,
// PairTwiddles), the per-bin stage, the inverse pre-split and one inverse transform -- with a mask value streamed from
// HBM where the denoiser evaluates a gain from a noise estimate.  Everything after the frame is the stream of
// ola_stream.h, which istft_run_kernel feeds too: lane l holds the frame's samples 2 l + 128 d, +1 in register d.  The
// halo frames of a wave (their PCM and mask rows are read again) go through the one loop, without the stores: the raw
// PCM registers shift from frame to frame, so the halo cannot stand apart as it does in istft_run_kernel.
//
// Mask.  Lane l owns the bins m and m + 512 of m = l + 64 d, d < 5.  Bin m <= 319 takes M[m]; bin m + 512 lies above
// n/2, where the caller gives no value: Y[1024 - k] = conj(Y[k]) (the output is real), so it takes M[512 - m],
// conjugated for a complex mask.  Lane 0's d = 0 item holds bins 0 and 512, whose imaginary mask parts are ignored.
// The items of d = 3 and 4 cover the bins 193..319 from both sides (frame_io.h); both sides use the same M[k].  A lane
// reads M[l + 64 d] and M[512 - l - 64 d]: ten coalesced loads per frame, bins 193..319 twice (the second from L2).
// The 1/1024 of the inverse transform is folded into the mask value (a power of two: exact).
//
// PCM.  Frame j + 1 starts one hop after frame j, and a hop is HR registers of the frame's layout, so the raw sample
// pairs shift down like the overlap-add does: a wave reads every sample of its run once (HR dwords per lane and frame)
// plus the R - 1 halo frames.
//
// Accuracy.  The forward transform rounds every bin by about 2^-23 sqrt(E), E the frame's energy, wherever the energy
// sits, and the mask passes that rounding like anything else in a bin: under a mask that removes something loud and
// keeps something faint it can exceed the project's bar of 1e-5 of the output.  stftmask_frame therefore forms
// rho^2 = 2^-46 E mean|M|^2 / sum y^2 (y: the frame before the synthesis window; tests/stftmask_fp32_ref.py) and a
// frame with rho > JDSP_STFTMASK_RHO is computed again by the same wave in FP64 (stftmask_frame_f64) before it enters
// the overlap-add.  The decision and both results are functions of the frame's samples and mask row alone, so the
// stream stays bit-identical across call cuts, launch geometries, shards and the batch.
#include "jdsp_internal.h"
#include "ola_stream.h"
#include "ragged_batch.h"

namespace jdsp {

#ifndef JDSP_STFTMASK_RESIDENT
// Waves per SIMD the launch plans for and __launch_bounds__ asks for.  A wave holds two mask rows (the frame's and
// the prefetched one: 20 registers REAL, 40 COMPLEX), both windows, the gain, the overlap-add sums, the raw PCM and
// the transform's twiddles, and the FP64 pass below needs some forty more while it runs: 208-214 registers with a real
// mask, 240-248 with a complex one, nothing in scratch (profiles/r13_stftmask_suppress.txt; 162-164 and 196 before that
// pass, profiles/r08_stftmask_isa.txt).  That is past the 128 of four waves per SIMD and past the 168 of three; two
// (256 registers) hold every instantiation, and two is what istft_run_kernel measured fastest for the same
// overlap-add and store pattern (profiles/r04_istft_launch_ab.txt).
#define JDSP_STFTMASK_RESIDENT 2
#endif

#ifndef JDSP_STFTMASK_RHO
// Half the bar with a margin of two: tests/stftmask_fp32_ref.py (RHO) derives it from a plain-FP32 restatement, and
// tests/test_stftmask_fp32_ref_cpu.py holds it there.  White input under a mask of order one has rho = 1.2e-7.
#define JDSP_STFTMASK_RHO 8.0e-7f
#endif

namespace {

// one mask row as a lane holds it: lo[d] for bin l + 64 d, hi[d] for bin l + 64 d + 512 (the value of bin 512 - l - 64 d)
template <int CPX> struct MaskRow;
template <> struct MaskRow<0> { float lo[5], hi[5]; };
template <> struct MaskRow<1> { float2 lo[5], hi[5]; };

// nontemporal: a mask row is read once
__device__ __forceinline__ void mask_load(MaskRow<0> &m, const void *row, int lane)
{
    const float *r = static_cast<const float *>(row);
#pragma unroll
    for (int d = 0; d < 5; d++) {
        m.lo[d] = __builtin_nontemporal_load(r + lane + 64 * d);
        m.hi[d] = __builtin_nontemporal_load(r + 512 - lane - 64 * d);
    }
}
__device__ __forceinline__ void mask_load(MaskRow<1> &m, const void *row, int lane)
{
    const f32x2 *r = static_cast<const f32x2 *>(row);
#pragma unroll
    for (int d = 0; d < 5; d++) {
        const f32x2 a = __builtin_nontemporal_load(r + lane + 64 * d);
        const f32x2 b = __builtin_nontemporal_load(r + 512 - lane - 64 * d);
        m.lo[d] = make_float2(a.x, a.y);
        m.hi[d] = make_float2(b.x, b.y);
    }
}

// raw row -> the factors the frame multiplies by: M / 1024, the upper bins' conjugated, no imaginary part at DC and n/2
__device__ __forceinline__ void mask_prepare(MaskRow<0> &m, const MaskRow<0> &raw, int)
{
#pragma unroll
    for (int d = 0; d < 5; d++) {
        m.lo[d] = raw.lo[d] * (1.0f / 1024.0f);
        m.hi[d] = raw.hi[d] * (1.0f / 1024.0f);
    }
}
__device__ __forceinline__ void mask_prepare(MaskRow<1> &m, const MaskRow<1> &raw, int lane)
{
    const float c = 1.0f / 1024.0f;
#pragma unroll
    for (int d = 0; d < 5; d++) {
        const bool real = d == 0 && lane == 0;
        m.lo[d] = make_float2(raw.lo[d].x * c, real ? 0.0f : raw.lo[d].y * c);
        m.hi[d] = make_float2(raw.hi[d].x * c, real ? 0.0f : -(raw.hi[d].y * c));
    }
}

__device__ __forceinline__ float2 mask_mul(float2 x, float m) { return make_float2(x.x * m, x.y * m); }
__device__ __forceinline__ float2 mask_mul(float2 x, float2 m)
{
    // spelled with fmaf: the same operations in every instantiation
    return make_float2(__builtin_fmaf(-x.y, m.y, x.x * m.x), __builtin_fmaf(x.y, m.x, x.x * m.y));
}

__device__ __forceinline__ float mask_abs2(float m) { return m * m; }
__device__ __forceinline__ float mask_abs2(float2 m) { return __builtin_fmaf(m.x, m.x, m.y * m.y); }

// A lane's share of sum |M / 1024|^2 over all 1024 bins of the Hermitian-extended row.  A lane's items hold the bins
// k = lane + 64 d and k + 512; the mirror images of both are some other item's for k >= 193 and their own for k = 0,
// and nobody's otherwise (those count twice).
template <int CPX> __device__ __forceinline__ float mask_energy(const MaskRow<CPX> &m, int lane)
{
    float s = 0.0f;
#pragma unroll
    for (int d = 0; d < 5; d++) {
        const int k = lane + 64 * d;
        s = __builtin_fmaf(k == 0 || k >= 193 ? 1.0f : 2.0f, mask_abs2(m.lo[d]) + mask_abs2(m.hi[d]), s);
    }
    return s;
}

// rho^2 > RHO^2 in the kernel's own units: e_in = sum (w_a x / 2)^2 = E / 4, m_sq = sum mask_energy = mean|M|^2 / 1024,
// so 2^-46 E mean|M|^2 = 2^-34 e_in m_sq.  False for NaN, for an all-zero mask and for silence (both exact).
constexpr float kUnsafeK = 5.8207660913467407e-11f / (JDSP_STFTMASK_RHO * JDSP_STFTMASK_RHO);
__device__ __forceinline__ bool stftmask_unsafe(float e_in, float m_sq, float e_out) { return e_in * m_sq * kUnsafeK > e_out; }

// One frame: y[d] = w_s * IDFT(M * DFT(w_a * frame)) at the samples (2 lane + 128 d, +1).  wa = w_a / 2 (the forward
// split's 1/2, frame_io.h), m as mask_prepare left it (so the 1/1024 is in), m_sq the lane's mask_energy of it,
// ws = w_s.  Returns stftmask_unsafe (wave-uniform): FP32 cannot hold this frame.  The criterion's three sums are
// reduced over the wave side by side at the end, where their dependent DPP chains interleave.
template <int CPX>
__device__ __forceinline__ bool stftmask_frame(const unsigned int (&raw)[8], const float2 (&wa)[8], const WaveTwiddles &tw,
                                               const PairTwiddles &pw, float2 *lds, int lane, const MaskRow<CPX> &m,
                                               float m_sq, const float2 (&ws)[8], float2 (&y)[8])
{
    float2 v[8];
    float e_in = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const float2 s = unpack_i16x2(raw[r]);
        v[r] = make_float2(s.x * wa[r].x, s.y * wa[r].y);
        e_in = __builtin_fmaf(v[r].x, v[r].x, __builtin_fmaf(v[r].y, v[r].y, e_in));
    }
    wave_fft512<false>(v, lds, lane, tw);
    float2 zr[5], ret[4];
    wave_lds_fence();                                            // the transform's last exchange reads are done
    pair_fetch_lds(v, lds, lane, zr);
#pragma unroll
    for (int d = 0; d < 5; d++) {
        const float2 e = cadd_conj(v[d], zr[d]);
        const float2 o = csub_conj_mj(v[d], zr[d]);
        const float2 p = cmul(pw.w[d], o);
        const float2 lo = mask_mul(cadd(e, p), m.lo[d]);         // Y[m] / 1024
        const float2 hi = mask_mul(csub(e, p), m.hi[d]);         // Y[m + 512] / 1024
        if (d < 4) presplit_inv_pair(lo, hi, pw.w[d], y[d], ret[d]);
        else y[d] = presplit_inv_reg(lo, hi, pw.w[d]);
    }
    pair_return_lds(ret, lds, lane, y);
    wave_fft512<true>(y, lds, lane, tw);
    wave_lds_fence();                                            // the scratch is free for the next frame
    float e_out = 0.0f;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        e_out = __builtin_fmaf(y[d].x, y[d].x, __builtin_fmaf(y[d].y, y[d].y, e_out));
        y[d] = make_float2(y[d].x * ws[d].x, y[d].y * ws[d].y);
    }
    return stftmask_unsafe(wave_sum_f32(e_in), wave_sum_f32(m_sq), wave_sum_f32(e_out));
}

// ---- the same frame in FP64 ----------------------------------------------------------------------------------------
// What the handle keeps for it (stftmask_api.hip): the windows as OlaStream::window_at gives them, unrounded, the
// twiddles tw[t] = exp(-2 pi i t / 1024), t < 512, and the count of recomputed frames: two words, of which the call
// number `epoch` (from the host) adds to count[epoch & 1] -- one atomic per wave, at the end of its run -- and zeroes
// the other for the next call.  Calls on a stream follow each other, so a call finds its word zero without anything
// being enqueued ahead of the launch.
struct StftMaskF64 {
    const double *wa, *ws;    // [1024] each
    const double2 *tw;        // [512]
    unsigned int *count;      // [2]
    unsigned int epoch;
};

__device__ __forceinline__ void stftmask_count_begin(const StftMaskF64 &q, int lane)
{
    if (blockIdx.x == 0 && lane == 0) q.count[(q.epoch + 1) & 1] = 0;
}
__device__ __forceinline__ void stftmask_count_end(const StftMaskF64 &q, int n, int lane)
{
    if (n && lane == 0) atomicAdd(q.count + (q.epoch & 1), (unsigned int)n);
}

__device__ __forceinline__ double2 cmul64(double2 a, double2 b)
{
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// One wave, a plain 1024-point complex radix-2 in LDS (buf: 1024 double2): decimation in frequency forward (natural
// order in, bit-reversed out), the mask applied where the bins lie, decimation in time back (bit-reversed in, natural
// out) -- no reordering pass.  The inverse runs as the forward transform of conj(Y): the output is real, so its real
// part is the frame.  row: the frame's mask row as the caller gave it.  Loops over registers are unrolled, the passes
// are not: the branch is rare and must not grow the kernel's registers.
template <int CPX>
__device__ __forceinline__ void stftmask_frame_f64(const unsigned int (&raw)[8], const StftMaskF64 &q, const void *row,
                                                   double2 *buf, int lane, float2 (&y)[8])
{
    // opaque from here on: what this rare pass derives from the lane (sixteen window addresses and more) must not be
    // hoisted out of the frame loop into registers the FP32 frames then carry
    asm volatile("" : "+v"(lane));
    wave_lds_fence();
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int i = 2 * lane + 128 * d;
        const float2 s = unpack_i16x2(raw[d]);
        buf[i] = make_double2((double)s.x * q.wa[i], 0.0);
        buf[i + 1] = make_double2((double)s.y * q.wa[i + 1], 0.0);
        asm volatile("" ::: "memory");                           // one register's loads in flight, not eight
    }
#pragma unroll 1
    for (int half = 512; half >= 1; half >>= 1) {
        wave_lds_fence();
        const int step = 512 / half;
#pragma unroll 1
        for (int t = lane; t < 512; t += 64) {
            const int j = t & (half - 1), i = ((t - j) << 1) + j;
            const double2 a = buf[i], b = buf[i + half];
            buf[i] = make_double2(a.x + b.x, a.y + b.y);
            buf[i + half] = cmul64(make_double2(a.x - b.x, a.y - b.y), q.tw[j * step]);
        }
    }
    wave_lds_fence();
    // bin k <= 512 sits at brev(k); conj(Y[k]) goes back there and conj(Y[1024 - k]) = Y[k] to brev(1024 - k), which
    // no lane reads in this pass
#pragma unroll 1
    for (int k = lane; k <= 512; k += 64) {
        const int at = (int)(__brev((unsigned int)k) >> 22);
        const double2 x = buf[at];
        double2 m;
        if (CPX) {
            const float2 mv = static_cast<const float2 *>(row)[k];
            m = make_double2((double)mv.x, (double)mv.y);
        } else {
            m = make_double2((double)static_cast<const float *>(row)[k], 0.0);
        }
        const bool real_bin = k == 0 || k == 512;                // Im M ignored, the bin is real
        const double2 yk = real_bin ? make_double2(m.x * x.x, 0.0) : cmul64(x, m);
        buf[at] = make_double2(yk.x, -yk.y);
        if (!real_bin) buf[(int)(__brev((unsigned int)(1024 - k)) >> 22)] = yk;
    }
#pragma unroll 1
    for (int half = 1; half <= 512; half <<= 1) {
        wave_lds_fence();
        const int step = 512 / half;
#pragma unroll 1
        for (int t = lane; t < 512; t += 64) {
            const int j = t & (half - 1), i = ((t - j) << 1) + j;
            const double2 a = buf[i], b = cmul64(buf[i + half], q.tw[j * step]);
            buf[i] = make_double2(a.x + b.x, a.y + b.y);
            buf[i + half] = make_double2(a.x - b.x, a.y - b.y);
        }
    }
    wave_lds_fence();
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int i = 2 * lane + 128 * d;
        y[d] = make_float2((float)(buf[i].x * (1.0 / 1024.0) * q.ws[i]), (float)(buf[i + 1].x * (1.0 / 1024.0) * q.ws[i + 1]));
        asm volatile("" ::: "memory");
    }
    wave_lds_fence();                                            // the scratch is free for the next frame
}

}  // namespace

struct StftMaskArgs {
    const short *pcm;         // hop (n_frames - 1) + 1024 samples
    const void *mask;         // rows of float (REAL) or float2 (COMPLEX), bins 0..512
    long pitch, n_frames;     // pitch in elements; 0: one row for every frame
    const float *wa;          // [1024] w_a[i] / 2
    const float *ws;          // [1024] w_s[i]
    const float *g;           // [hop]  emission gain
    const float *tail_in;     // [1024 - hop] partial sums of the samples after the last emitted one
    float *tail_out;
    short *out;               // may be NULL
    float *out_f32;           // may be NULL
    int run;
    StftMaskF64 f64;
};

// the FP32 transform's scratch and the FP64 pass's 1024 complex doubles share one LDS array (16 KiB a wave: eight
// workgroups of one wave a CU at JDSP_STFTMASK_RESIDENT 2, 128 of the CU's 160 KiB)
#define JDSP_STFTMASK_LDS                                           \
    __shared__ __attribute__((aligned(16))) double2 lds64[1024];    \
    static_assert(sizeof(double2) * 1024 >= sizeof(float2) * kWaveLdsComplex, "the FP32 scratch fits"); \
    float2 *lds = reinterpret_cast<float2 *>(lds64)

template <int R, int CPX>
__global__ __launch_bounds__(64, JDSP_STFTMASK_RESIDENT) void stftmask_run_kernel(StftMaskArgs a,
                                                                                  const float2 *__restrict__ table)
{
    constexpr int HR = 8 / R;                                   // registers per hop
    constexpr int HOP = 1024 / R;
    constexpr size_t kElem = CPX ? sizeof(float2) : sizeof(float);
    JDSP_STFTMASK_LDS;
    const int lane = threadIdx.x;
    stftmask_count_begin(a.f64, lane);
    int n_redo = 0;                                              // emitted frames of this run computed again in FP64
    long j0, j1;
    if (!ola_run_range(a.run, a.n_frames, j0, j1)) return;
    // the halo: frames j0 - R + 1 .. j0 - 1 are transformed and added, not emitted (all >= 0: the launch keeps
    // run >= R - 1)
    const long js = j0 == 0 ? 0 : j0 - (R - 1);

    WaveTwiddles tw;
    load_wave_twiddles(tw, table, lane);
    PairTwiddles pw;
    load_pair_twiddles(pw, table, lane);
    float2 wa[8], ws[8];
    {
        const float2 *wa_t = reinterpret_cast<const float2 *>(a.wa);
        const float2 *ws_t = reinterpret_cast<const float2 *>(a.ws);
#pragma unroll
        for (int d = 0; d < 8; d++) { wa[d] = wa_t[lane + 64 * d]; ws[d] = ws_t[lane + 64 * d]; }
    }
    OlaAcc<float2, HR> ola;
    ola.init(a.g, lane);
    if (j0 == 0) ola.load_tail(a.tail_in, lane);
    float2 y[8], o[HR];

    const char *mask = static_cast<const char *>(a.mask);
    const size_t row_bytes = (size_t)a.pitch * kElem;
    unsigned int raw[8], nraw[HR];
    MaskRow<CPX> m, nm;
    {
        const unsigned int *p = reinterpret_cast<const unsigned int *>(a.pcm + js * HOP) + lane;
#pragma unroll
        for (int r = 0; r < 8; r++) raw[r] = p[64 * r];
        mask_load(nm, mask + (size_t)js * row_bytes, lane);
        mask_prepare(m, nm, lane);
    }
    float m_sq = mask_energy(m, lane);
    for (long j = js; j < j1; j++) {
        // frame j + 1's new hop of PCM and its mask row, needed one iteration from now: unguarded loads at a clamped
        // frame (past the wave's run they are never used), raw until they are staged below
        const long jn = j + 1 < a.n_frames ? j + 1 : a.n_frames - 1;
        {
            const unsigned int *p = reinterpret_cast<const unsigned int *>(a.pcm + jn * HOP) + 64 * (8 - HR) + lane;
#pragma unroll
            for (int r = 0; r < HR; r++) nraw[r] = p[64 * r];
        }
        if (a.pitch) mask_load(nm, mask + (size_t)jn * row_bytes, lane);     // pitch 0: the row stays in registers
        if (stftmask_frame<CPX>(raw, wa, tw, pw, lds, lane, m, m_sq, ws, y)) {
            // a frame FP32 cannot hold: again, in FP64; counted by the wave that emits it
            stftmask_frame_f64<CPX>(raw, a.f64, mask + (size_t)(a.pitch ? j : 0) * row_bytes, lds64, lane, y);
            n_redo += j >= j0;
        }
        ola.add(y, o);
        // stage the prefetched values before this frame's stores: vmcnt counts loads and stores in issue order, and a
        // wait for them at the top of the next iteration would also wait for these stores (istft_run_kernel)
#pragma unroll
        for (int r = 0; r < 8 - HR; r++) raw[r] = raw[r + HR];
#pragma unroll
        for (int r = 0; r < HR; r++) raw[8 - HR + r] = nraw[r];
        if (a.pitch) {
            mask_prepare(m, nm, lane);
            m_sq = mask_energy(m, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (j >= j0) ola.emit(o, a.out, a.out_f32, j * HOP, lane);
        ola.shift(j == a.n_frames - 1, a.tail_out, lane);
    }
    stftmask_count_end(a.f64, n_redo, lane);
}

template <int R>
static void launch_kind(hipStream_t s, int cpx, long grid, const StftMaskArgs &a, const float2 *table)
{
    if (cpx) hipLaunchKernelGGL((stftmask_run_kernel<R, 1>), dim3((unsigned)grid), dim3(64), 0, s, a, table);
    else hipLaunchKernelGGL((stftmask_run_kernel<R, 0>), dim3((unsigned)grid), dim3(64), 0, s, a, table);
}

int launch_stftmask(hipStream_t s, int n_cu, int hop, int complex_mask, const short *pcm, const void *mask, long pitch,
                    long n_frames, const float *wa, const float *ws, const float *g, const float *tail_in,
                    float *tail_out, short *out, float *out_f32, const float2 *table, int run_opt, const double *f64,
                    unsigned int *count, unsigned int epoch)
{
    if (n_frames <= 0) return 0;
    const int r = 1024 / hop;
    const OlaRunPlan p = plan_ola_run(n_cu, JDSP_STFTMASK_RESIDENT, r, n_frames, run_opt);
    StftMaskArgs a = {pcm, mask, pitch, n_frames, wa, ws, g, tail_in, tail_out, out, out_f32, (int)p.run,
                      {f64, f64 + 1024, reinterpret_cast<const double2 *>(f64 + 2048), count, epoch}};
    if (r == 1) launch_kind<1>(s, complex_mask, p.grid, a, table);
    else if (r == 2) launch_kind<2>(s, complex_mask, p.grid, a, table);
    else launch_kind<4>(s, complex_mask, p.grid, a, table);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- a batch of independent streams (utterances), or the chunks of live streams, in one launch ---------------------
// (jdsp_stftmask_batch_*, jdsp_stftmask_streams_*)
// The waves are planned over the CONCATENATED frame axis: wave w owns the global frames [w run, (w + 1) run) whatever
// the utterances' lengths are, so the plan is plan_ola_run's host arithmetic on the total alone.  Global frame j is
// mask row j; it belongs to utterance u with frame_first[u] <= j < frame_first[u + 1] and starts at the sample
// sample_first[u] + hop (j - frame_first[u]) of pcm and out.  A wave finds the utterance of its first frame by a
// binary search and then walks: its halo stops at the utterance's first frame; after an utterance's last frame it
// writes the tail from its registers (OlaAcc::emit_tail: no flush launch, no tail in memory), zeroes the sums and
// reads all eight raw registers at the next non-empty utterance's first sample.  That walk is RaggedSpan
// (ragged_batch.h) and the raw registers are PcmHops (frame_io.h), both shared with the analysis and synthesis batch
// kernels.  The stream kernel above keeps its own loop, statement for statement: every restatement of it tried -- the
// merged loop under either args layout or with two args structs, the hop pipeline alone -- moved its instruction
// schedule, and with it two to four benchmark legs by 0.2-0.9 % past the parent's spread
// (profiles/r17_one_frame_walk.txt).
struct StftMaskBatchArgs {
    const short *pcm;
    const void *mask;
    long pitch, n_frames;     // n_frames: of all utterances, frame_first[n_utts]
    const float *wa, *ws, *g; // as StftMaskArgs
    long n_utts;
    short *out;               // may be NULL
    float *out_f32;           // may be NULL
    int run;
    StftMaskF64 f64;
};

// The frame loop of stftmask_batch_kernel and stftmask_live_kernel, over RaggedSpan and LiveSpan (ragged_batch.h).
// They differ where a span starts and ends: a live chunk starts from its stream's carried tail wherever the first frame
// a wave computes is the chunk's first -- at the start of the walk and after every span.next() -- where an utterance
// starts from zero; and after a chunk's last frame the new tail goes to the stream's other tail buffer (OlaAcc::shift)
// where an utterance's is emitted behind it and the sums restart.  A chunk writes its hop F_c samples and nothing
// behind them.  The frames, the rho criterion and the FP64 pass are functions of a frame's samples and mask row alone.
// The arguments come by value: with a reference to the kernel's the compiler scheduled both kernels' loops otherwise
// than it does a loop written into the kernel itself; by value both come out as they do from a loop of their own,
// up to the operand order of commutative instructions (profiles/r19_ragged_call_layer.txt).
template <int R, int CPX, class Span>
__device__ __forceinline__ void stftmask_ragged(StftMaskBatchArgs a, const float2 *__restrict__ table, Span span)
{
    constexpr int HR = 8 / R;
    constexpr size_t kElem = CPX ? sizeof(float2) : sizeof(float);
    JDSP_STFTMASK_LDS;
    const int lane = threadIdx.x;
    stftmask_count_begin(a.f64, lane);
    int n_redo = 0;                                              // emitted frames of this run computed again in FP64
    long j0, j1;
    if (!ola_run_range(a.run, a.n_frames, j0, j1)) return;
    span.begin(j0);
    const long js = span.first(j0, R);                           // the halo, never into the span before

    WaveTwiddles tw;
    load_wave_twiddles(tw, table, lane);
    PairTwiddles pw;
    load_pair_twiddles(pw, table, lane);
    float2 wa[8], ws[8];
    {
        const float2 *wa_t = reinterpret_cast<const float2 *>(a.wa);
        const float2 *ws_t = reinterpret_cast<const float2 *>(a.ws);
#pragma unroll
        for (int d = 0; d < 8; d++) { wa[d] = wa_t[lane + 64 * d]; ws[d] = ws_t[lane + 64 * d]; }
    }
    OlaAcc<float2, HR> ola;
    ola.init(a.g, lane);
    if constexpr (Span::kLive) {
        if (span.starts_span(js)) ola.load_tail(span.tail_in(), lane);
    }
    float2 y[8], o[HR];

    const char *mask = static_cast<const char *>(a.mask);
    const size_t row_bytes = (size_t)a.pitch * kElem;
    PcmHops<HR> pcm;
    MaskRow<CPX> m, nm;
    pcm.load(a.pcm, span.at(js), lane);
    mask_load(nm, mask + (size_t)js * row_bytes, lane);
    mask_prepare(m, nm, lane);
    float m_sq = mask_energy(m, lane);
    for (long j = js; j < j1; j++) {
        // the PCM's prefetch clamps inside the span: after its last frame the next frame's samples are another
        // span's, read whole below.  The mask rows run on across spans.
        const bool last = span.last(j);
        const long jm = j + 1 < a.n_frames ? j + 1 : a.n_frames - 1;
        pcm.prefetch(a.pcm, span.at(span.next_inside(j)), lane);
        if (a.pitch) mask_load(nm, mask + (size_t)jm * row_bytes, lane);
        if (stftmask_frame<CPX>(pcm.raw, wa, tw, pw, lds, lane, m, m_sq, ws, y)) {
            stftmask_frame_f64<CPX>(pcm.raw, a.f64, mask + (size_t)(a.pitch ? j : 0) * row_bytes, lds64, lane, y);
            n_redo += j >= j0;
        }
        ola.add(y, o);
        pcm.advance();                                           // staged before this frame's stores (frame_io.h)
        if (a.pitch) {
            mask_prepare(m, nm, lane);
            m_sq = mask_energy(m, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (j >= j0) ola.emit(o, a.out, a.out_f32, span.at(j), lane);
        // a halo frame is never a span's last (j0 lies in the halo's span), so the wave that emits the last frame
        // emits or writes the tail
        if constexpr (Span::kLive) {
            ola.shift(last, span.tail_out(), lane);
            if (last && j + 1 < j1) {
                span.next();                                     // frame j + 1 exists, so a non-empty chunk follows
                ola.load_tail(span.tail_in(), lane);
                pcm.load(a.pcm, span.at(j + 1), lane);
            }
        } else {
            ola.shift(false, nullptr, lane);
            if (last) {
                ola.emit_tail(a.out, a.out_f32, span.at(j + 1), lane);
                ola.restart();
                if (j + 1 < j1) {
                    span.next();                                 // frame j + 1 exists, so a non-empty utterance follows
                    pcm.load(a.pcm, span.at(j + 1), lane);
                }
            }
        }
    }
    stftmask_count_end(a.f64, n_redo, lane);
}

template <int R, int CPX>
__global__ __launch_bounds__(64, JDSP_STFTMASK_RESIDENT) void stftmask_batch_kernel(
    StftMaskBatchArgs a, const float2 *__restrict__ table, const long long *__restrict__ sample_first,
    const long long *__restrict__ frame_first)
{
    stftmask_ragged<R, CPX>(a, table, RaggedSpan<1024 / R>(sample_first, frame_first, a.n_utts));
}

// the chunks of live streams (jdsp_stftmask_streams_*): the chunk's stream and parity are loaded next to its offsets,
// into scalar registers (LiveStreams, jdsp_internal.h)
template <int R, int CPX>
__global__ __launch_bounds__(64, JDSP_STFTMASK_RESIDENT) void stftmask_live_kernel(
    StftMaskBatchArgs a, const float2 *__restrict__ table, const long long *__restrict__ sample_first,
    const long long *__restrict__ frame_first, const long long *__restrict__ stream_id, const int *__restrict__ parity,
    LiveStreams live)
{
    stftmask_ragged<R, CPX>(a, table, LiveSpan<1024 / R>(sample_first, frame_first, a.n_utts, stream_id, parity, live));
}

// live != NULL: the chunks of live streams
template <int R, int CPX>
static void launch_ragged_one(hipStream_t s, long grid, const StftMaskBatchArgs &a, const float2 *table,
                              const long long *sample_first, const long long *frame_first, const LiveStreams *live)
{
    if (live)
        hipLaunchKernelGGL((stftmask_live_kernel<R, CPX>), dim3((unsigned)grid), dim3(64), 0, s, a, table, sample_first,
                           frame_first, live->stream_id, live->parity, *live);
    else
        hipLaunchKernelGGL((stftmask_batch_kernel<R, CPX>), dim3((unsigned)grid), dim3(64), 0, s, a, table, sample_first,
                           frame_first);
}

template <int R>
static void launch_ragged_kind(hipStream_t s, int cpx, long grid, const StftMaskBatchArgs &a, const float2 *table,
                               const long long *sample_first, const long long *frame_first, const LiveStreams *live)
{
    if (cpx) launch_ragged_one<R, 1>(s, grid, a, table, sample_first, frame_first, live);
    else launch_ragged_one<R, 0>(s, grid, a, table, sample_first, frame_first, live);
}

int launch_stftmask_ragged(hipStream_t s, int n_cu, int hop, int complex_mask, const short *pcm, const void *mask,
                           long pitch, long n_frames_total, const long long *sample_first, const long long *frame_first,
                           long n_spans, const LiveStreams *live, const float *wa, const float *ws, const float *g,
                           short *out, float *out_f32, const float2 *table, int run_opt, const double *f64,
                           unsigned int *count, unsigned int epoch)
{
    if (n_frames_total <= 0 || n_spans <= 0) return 0;
    const int r = 1024 / hop;
    const OlaRunPlan p = plan_ola_run(n_cu, JDSP_STFTMASK_RESIDENT, r, n_frames_total, run_opt);
    StftMaskBatchArgs a = {pcm, mask, pitch, n_frames_total, wa, ws, g, n_spans, out, out_f32, (int)p.run,
                           {f64, f64 + 1024, reinterpret_cast<const double2 *>(f64 + 2048), count, epoch}};
    if (r == 1) launch_ragged_kind<1>(s, complex_mask, p.grid, a, table, sample_first, frame_first, live);
    else if (r == 2) launch_ragged_kind<2>(s, complex_mask, p.grid, a, table, sample_first, frame_first, live);
    else launch_ragged_kind<4>(s, complex_mask, p.grid, a, table, sample_first, frame_first, live);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
