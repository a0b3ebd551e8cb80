// denoise_kernels.hip -- SpectralSubtraction_final.cpp / WienerFilter_final.cpp on gfx950.
//
// The reference runs one 512-sample block at a time through a chain of functions with
// static state (SS:92-113).  Here a whole batch of blocks goes through five launches:
//
//   vad_kernel          A11  VoiceActivityDetection per block (SS:121-156): integer/FP64, bit-exact
//   plan_kernel         A13  main()'s run-length counter (SS:98-109) as prefix scans over 64-block
//                            bit masks: the list of blocks that call EstimateNoiseSpectrum (run
//                            length >= 2) and, per block, which latched estimate (run length == 10,
//                            SS:189-193) is current
//   noise_accum_kernel  A12  |FFT(window * [previous block, block])| of the listed blocks (SS:168-183) folded into one
//                            affine map of the running average (SS:182-187) per chunk of events, in registers
//   noise_combine_kernel A12 the chunk maps composed: the average entering every chunk, the latched rows, the state
//   denoise_run_kernel  A8/A9/A10  window -> FFT -> gain -> IFFT -> overlap-add -> (short), fused; one wavefront
//                            walks a run of consecutive output blocks (one round of resident waves, or the handle's
//                            "blocks_per_wave") and recomputes one halo frame, in the same loop body as every other
// (512-point frames: vad_*<4>, noise_accum512_kernel, denoise512_run_kernel; sharded runs use the same kernels on a
// rank's range of events.)
// (A batch of ragged utterances, each a fresh stream: vad_flags_batch_kernel, noise_batch_kernel, denoise_batch_kernel,
// denoise_redo_f64_batch_kernel, further down.)
//
// All of the reference's statics live in DenoiseState (ping-ponged between calls so a launch
// never reads state it is also writing), which makes batches of any size -- down to the
// reference's one block per call -- produce the same stream.
#include "frame_io.h"
#include "jdsp_internal.h"
#include "ragged_batch.h"

namespace jdsp {

// ---------------------------------------------------------------------------------------
// A11.  frame = [zeros(512), block] because the keep buffer is never updated (SS:154 is
// unreachable); s = (short)(x * w) truncates; E = sum s^2 / 1024; Z counts s[i]*x[i+1] < 0
// (the next sample is not windowed yet, SS:139).  E > 700 <=> sum s^2 > 716800 exactly.
#ifndef JDSP_VAD_BLOCKS_PER_WAVE
#define JDSP_VAD_BLOCKS_PER_WAVE 4
#endif
// blocks per wave: the FP64 window slice (64 B per lane) is loaded once per wave.  4: 66 registers, seven waves per SIMD,
// 13.0 us per 65,536 blocks; 8: 86 registers, 15.0 us; 2: 13.4; 1: 18.9; 16: 278 registers, 28.8 (profiles/r02_denoise_ab.txt)
constexpr int kVadBlocksPerWave = JDSP_VAD_BLOCKS_PER_WAVE;

// SPL = samples per lane = BLOCK_LEN / 64: 8 for the reference's 512-sample blocks (SS:54), 4 for 256-sample blocks
// (FFT_PROCESSING_SIZE 512, BASELINE config 3 as worded).  dEnergy = sum / (2 BLOCK_LEN) > 700 (SS:143,147,48).
template <int SPL>
__global__ __launch_bounds__(64) void vad_kernel(const short *__restrict__ pcm, long n_blocks,
                                                 const double *__restrict__ w_hi, int use_zcr,
                                                 unsigned char *__restrict__ flags,
                                                 long long *__restrict__ dbg_energy, int *__restrict__ dbg_zcr)
{
    static_assert(SPL == 8 || SPL == 4, "block of 512 or 256 samples");
    const int lane = threadIdx.x;
    const long b0 = (long)blockIdx.x * kVadBlocksPerWave;
    if (b0 >= n_blocks) return;
    double w[SPL];
#pragma unroll
    for (int k = 0; k < SPL; k++) w[k] = w_hi[SPL * lane + k];
    u32x4 img[kVadBlocksPerWave];
#pragma unroll
    for (int i = 0; i < kVadBlocksPerWave; i++) {
        const long b = b0 + i < n_blocks ? b0 + i : n_blocks - 1;
        if (SPL == 8) {
            img[i] = reinterpret_cast<const u32x4 *>(pcm + b * 512)[lane];
        } else {
            const uint2 h = reinterpret_cast<const uint2 *>(pcm + b * 256)[lane];
            img[i].x = h.x; img[i].y = h.y; img[i].z = 0u; img[i].w = 0u;
        }
    }
#pragma unroll
    for (int i = 0; i < kVadBlocksPerWave; i++) {
        const long b = b0 + i;
        if (b >= n_blocks) break;
        int x[9];
        x[0] = (short)(img[i].x & 0xffffu); x[1] = (int)img[i].x >> 16;
        x[2] = (short)(img[i].y & 0xffffu); x[3] = (int)img[i].y >> 16;
        x[4] = (short)(img[i].z & 0xffffu); x[5] = (int)img[i].z >> 16;
        x[6] = (short)(img[i].w & 0xffffu); x[7] = (int)img[i].w >> 16;
        x[SPL] = __shfl_down(x[0], 1);                 // first sample of the next lane
        if (lane == 63) x[SPL] = 0;                    // the sample past the block does not exist: frame[N], defined 0
        // s and x are 16-bit quantities: 24-bit multiplies (full rate; the 32-bit v_mul_lo is quarter rate) are
        // exact, and four squares (< 2^30 each) fit an unsigned 32-bit partial sum
        long long e = 0;
        unsigned int q4 = 0;
        int z = 0;
#pragma unroll
        for (int k = 0; k < SPL; k++) {
            const int s = (int)((double)x[k] * w[k]);  // (short)(short * double), in range
            q4 += (unsigned int)__mul24(s, s);
            if ((k & 3) == 3) { e += (long long)q4; q4 = 0; }
            z += (__mul24(s, x[k + 1]) < 0) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            e += __shfl_xor(e, o);
            z += __shfl_xor(z, o);
        }
        if (lane == 0) {
            // SS:147 with THRESHOLD_OF_ENERGY 700, _ZCR 200; BeamForming_MVDR_ver1.cpp:233 tests the energy only
            flags[b] = (e > 700LL * 128 * SPL || (use_zcr && z < 200)) ? 1 : 0;
            if (dbg_energy) dbg_energy[b] = e;
            if (dbg_zcr) dbg_zcr[b] = z;
        }
    }
}

// The same decision without the trace (dbg_energy / dbg_zcr are NULL in every batched chain): what costs in the
// kernel above is not the arithmetic but the two wave reductions -- __shfl_xor is a ds_bpermute, 8.9 issue slots
// each on this chip (tools/valu_rate.hip), eighteen of them per block.  Only the FLAG is needed here, so
//   * the zero-crossing count never exists per lane: every sample position's comparison goes to an SGPR pair and
//     the scalar unit counts its bits (s_bcnt1), beside the vector pipe;
//   * a lane's energy is clamped to 2^20 per four samples before the wave sum: the sum then fits 32 bits, and it
//     exceeds 700 * n exactly when the true sum does (a clamped lane alone is already above the threshold);
//   * the one 32-bit wave sum is five DPP adds (quad swaps, row mirrors, row broadcasts) and a v_readlane
//     (wave_sum_u32, frame_io.h).
// Flags are bit-identical to the traced kernel's (tests/test_denoise_gpu.py checks both against the CPU restatement).
template <int SPL>
__global__ __launch_bounds__(64) void vad_flags_kernel(const short *__restrict__ pcm, long n_blocks,
                                                       const double *__restrict__ w_hi, int use_zcr,
                                                       unsigned char *__restrict__ flags)
{
    static_assert(SPL == 8 || SPL == 4, "block of 512 or 256 samples");
    const int lane = threadIdx.x;
    const long b0 = (long)blockIdx.x * kVadBlocksPerWave;
    if (b0 >= n_blocks) return;
    double w[SPL];
#pragma unroll
    for (int k = 0; k < SPL; k++) w[k] = w_hi[SPL * lane + k];
    u32x4 img[kVadBlocksPerWave];
#pragma unroll
    for (int i = 0; i < kVadBlocksPerWave; i++) {
        const long b = b0 + i < n_blocks ? b0 + i : n_blocks - 1;
        if (SPL == 8) {
            img[i] = reinterpret_cast<const u32x4 *>(pcm + b * 512)[lane];
        } else {
            const uint2 h = reinterpret_cast<const uint2 *>(pcm + b * 256)[lane];
            img[i].x = h.x; img[i].y = h.y; img[i].z = 0u; img[i].w = 0u;
        }
    }
    unsigned int voice_bits = 0;                                   // wave-uniform
#pragma unroll
    for (int i = 0; i < kVadBlocksPerWave; i++) {
        int x[9];
        x[0] = (short)(img[i].x & 0xffffu); x[1] = (int)img[i].x >> 16;
        x[2] = (short)(img[i].y & 0xffffu); x[3] = (int)img[i].y >> 16;
        x[4] = (short)(img[i].z & 0xffffu); x[5] = (int)img[i].z >> 16;
        x[6] = (short)(img[i].w & 0xffffu); x[7] = (int)img[i].w >> 16;
        x[SPL] = __builtin_amdgcn_update_dpp(0, x[0], 0x130, 0xf, 0xf, true);    // wave_shl:1 -- lane i takes lane i+1; lane 63 gets 0
        unsigned int qa = 0, qb = 0;
        int z = 0;                                                  // wave-uniform: counted on the scalar unit
#pragma unroll
        for (int k = 0; k < SPL; k++) {
            const int sv = (int)((double)x[k] * w[k]);              // (short)(short * double), in range
            if (k < 4) qa += (unsigned int)__mul24(sv, sv); else qb += (unsigned int)__mul24(sv, sv);
            z += __popcll(__ballot(__mul24(sv, x[k + 1]) < 0));
        }
        const unsigned int cap = 1u << 20;
        const unsigned int e = wave_sum_u32((qa < cap ? qa : cap) + (qb < cap ? qb : cap));
        if (e > 700u * 128u * SPL || (use_zcr && z < 200)) voice_bits |= 1u << i;
    }
    if (lane < kVadBlocksPerWave && b0 + lane < n_blocks) flags[b0 + lane] = (voice_bits >> lane) & 1u;
}

// The same flags over the CONCATENATED block axis of a batch of ragged utterances (ragged_batch.h; the layout
// include/jdsp.h gives for jdsp_denoise_batch_dev): global block j of utterance u is the 512 samples at
// sample_first[u] + 512 (j - block_first[u]).  The VAD has no state (the frame is [zeros, block]), so only the block's
// address is new; sample_first is even, so a lane's 16 bytes are 4-byte aligned and no more.
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));
// vad_flags_kernel's decision for the blocks of a wave: bit i = block i (its image in img[i]) is voice.  The arithmetic
// is that kernel's, statement for statement; it is restated and not shared because calling a common function from
// vad_flags_kernel changes that kernel's own instruction selection (profiles/r14_denoise_batch_isa.txt).
template <int SPL>
__device__ __forceinline__ unsigned int vad_voice_bits(const u32x4 (&img)[kVadBlocksPerWave], const double (&w)[SPL],
                                                       int use_zcr)
{
    unsigned int voice_bits = 0;
#pragma unroll
    for (int i = 0; i < kVadBlocksPerWave; i++) {
        int x[9];
        x[0] = (short)(img[i].x & 0xffffu); x[1] = (int)img[i].x >> 16;
        x[2] = (short)(img[i].y & 0xffffu); x[3] = (int)img[i].y >> 16;
        x[4] = (short)(img[i].z & 0xffffu); x[5] = (int)img[i].z >> 16;
        x[6] = (short)(img[i].w & 0xffffu); x[7] = (int)img[i].w >> 16;
        x[SPL] = __builtin_amdgcn_update_dpp(0, x[0], 0x130, 0xf, 0xf, true);    // wave_shl:1 -- lane i takes lane i+1; lane 63 gets 0
        unsigned int qa = 0, qb = 0;
        int z = 0;                                                  // wave-uniform: counted on the scalar unit
#pragma unroll
        for (int k = 0; k < SPL; k++) {
            const int sv = (int)((double)x[k] * w[k]);              // (short)(short * double), in range
            if (k < 4) qa += (unsigned int)__mul24(sv, sv); else qb += (unsigned int)__mul24(sv, sv);
            z += __popcll(__ballot(__mul24(sv, x[k + 1]) < 0));
        }
        const unsigned int cap = 1u << 20;
        const unsigned int e = wave_sum_u32((qa < cap ? qa : cap) + (qb < cap ? qb : cap));
        if (e > 700u * 128u * SPL || (use_zcr && z < 200)) voice_bits |= 1u << i;
    }
    return voice_bits;
}

__global__ __launch_bounds__(64) void vad_flags_batch_kernel(const short *__restrict__ pcm,
                                                             const long long *__restrict__ sample_first,
                                                             const long long *__restrict__ block_first, long n_utts,
                                                             long n_blocks, const double *__restrict__ w_hi,
                                                             unsigned char *__restrict__ flags)
{
    const int lane = threadIdx.x;
    const long b0 = (long)blockIdx.x * kVadBlocksPerWave;
    if (b0 >= n_blocks) return;
    double w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = w_hi[8 * lane + k];
    long u = ragged_find_utt(block_first, n_utts, b0);
    long ue = uniform_i64(block_first + u + 1);
    long base = uniform_i64(sample_first + u) - uniform_i64(block_first + u) * 512;   // global block j starts at base + 512 j
    u32x4 img[kVadBlocksPerWave];
#pragma unroll
    for (int i = 0; i < kVadBlocksPerWave; i++) {
        const long b = b0 + i < n_blocks ? b0 + i : n_blocks - 1;
        if (b >= ue) {                                          // block b exists, so a non-empty utterance follows
            const long nb = ue;
            ragged_next_utt(block_first, n_utts, u, ue);
            base = uniform_i64(sample_first + u) - nb * 512;
        }
        img[i] = reinterpret_cast<const u32x4_a4 *>(pcm + base + b * 512)[lane];
    }
    const unsigned int voice_bits = vad_voice_bits<8>(img, w, 1);              // wave-uniform
    if (lane < kVadBlocksPerWave && b0 + lane < n_blocks) flags[b0 + lane] = (voice_bits >> lane) & 1u;
}

// ---------------------------------------------------------------------------------------
// A13 bookkeeping.  One workgroup of 1024 threads; each thread owns 64 consecutive blocks,
// whose voice flags it packs into one 64-bit mask, so every pass after the single load runs
// in registers.  Batches longer than 65,536 blocks are walked tile by tile with the carries
// (run length, event and latch counts) kept in LDS.
//
// Outputs: events[e] / ev_n[e] = block index and run length of the e-th EstimateNoiseSpectrum
// call (run length >= 2, SS:103-105); per 64-block slice s, ver_base[s] = number of latches
// (run length == 10, SS:189) before the slice and snap_mask[s] = which of its blocks latch, so
//     version(j) = ver_base[j >> 6] + popcount(snap_mask[j >> 6] & bits 0..(j & 63))
// (the estimate latched AT block j already applies to block j: main() estimates first).
struct RunSummary { int has_voice, trailing; };

__device__ __forceinline__ RunSummary combine(RunSummary a, RunSummary b)
{
    RunSummary r;
    r.has_voice = a.has_voice | b.has_voice;
    r.trailing = b.has_voice ? b.trailing : a.trailing + b.trailing;
    return r;
}

__global__ __launch_bounds__(1024) void plan_kernel(const unsigned char *__restrict__ flags, long n_blocks,
                                                    const int *__restrict__ run_len_in_p, DenoiseState *st_out,
                                                    int *__restrict__ ver_base,
                                                    unsigned long long *__restrict__ snap_mask,
                                                    int *__restrict__ events, int *__restrict__ ev_n,
                                                    DenoisePlan *plan, int latch_run, int *run_len_out)
{
    // latch_run > 0: the estimate changes when the run length equals it (SS:189: 10);
    // latch_run == 0: it changes at every event (BeamForming_MVDR_ver1.cpp:201 accumulates each time)
    __shared__ RunSummary sum[1024];
    __shared__ int cnt_ev[1024], cnt_sn[1024];
    __shared__ int carry_run, carry_ev, carry_sn;
    __shared__ RunSummary wave_sum[16];
    __shared__ int wave_ev[16], wave_sn[16];
    const int t = threadIdx.x;
    const int run_len_in = *run_len_in_p;
    if (t == 0) { carry_run = run_len_in; carry_ev = 0; carry_sn = 0; }
    __syncthreads();

    for (long tile0 = 0; tile0 < n_blocks; tile0 += 65536) {
        const long a = tile0 + (long)t * 64;
        long left = n_blocks - a;
        const int cnt = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        unsigned long long V = 0;                               // bit i: block a+i is voice
        if (cnt == 64 && (((uintptr_t)(flags + a)) & 15u) == 0) {
            const uint4 *p = reinterpret_cast<const uint4 *>(flags + a);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 w = p[q];
                const unsigned int d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    // the four 0/1 bytes of d[k] -> 4 adjacent bits
                    const unsigned int nib = ((d[k] & 0x01010101u) * 0x01020408u) >> 24;
                    V |= (unsigned long long)(nib & 15u) << (16 * q + 4 * k);
                }
            }
        } else {
            for (int i = 0; i < cnt; i++) V |= (unsigned long long)(flags[a + i] != 0) << i;
        }
        RunSummary mine;
        mine.has_voice = V != 0;
        mine.trailing = V ? (cnt - 1) - (63 - __clzll(V)) : cnt;
        // inclusive scan of the run summaries over the 1024 threads: shuffles inside each wave, one pass over the
        // 16 wave totals, two barriers (a Hillis-Steele scan through LDS took twenty)
        {
            const int lane = t & 63, wv = t >> 6;
            RunSummary v = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                RunSummary u;
                u.has_voice = __shfl_up(v.has_voice, o, 64);
                u.trailing = __shfl_up(v.trailing, o, 64);
                if (lane >= o) v = combine(u, v);
            }
            if (lane == 63) wave_sum[wv] = v;
            __syncthreads();
            if (wv > 0) {
                RunSummary pre = wave_sum[0];
                for (int q = 1; q < wv; q++) pre = combine(pre, wave_sum[q]);
                v = combine(pre, v);
            }
            sum[t] = v;
            __syncthreads();
        }
        const int run_in = carry_run;
        int r = run_in;                                          // run length entering my slice
        if (t > 0) r = sum[t - 1].has_voice ? sum[t - 1].trailing : run_in + sum[t - 1].trailing;
        const int r_start = r;
        // event / latch masks of my slice, bit-parallel.  N = noise bits.  An event (run length >= 2) is a noise
        // bit whose predecessor is noise too -- bit 0's predecessor is the incoming run.  A latch (run length ==
        // latch_run) is the last of latch_run noise bits that follow a voice bit inside the slice, or bit
        // latch_run - r_start - 1 when everything up to it is noise (the run came in from before the slice).
        const unsigned long long full = cnt == 64 ? ~0ull : ((1ull << cnt) - 1ull);
        const unsigned long long N = ~V & full;
        const unsigned long long E = N & ((N << 1) | (r_start >= 1 ? 1ull : 0ull));
        unsigned long long S = E;                                // latch_run == 0: every event changes the estimate
        if (latch_run > 0) {
            unsigned long long A = N;
            for (int k = 1; k < latch_run && k < 64; k++) A &= N << k;
            S = latch_run < 64 ? (A & (V << latch_run)) : 0ull;
            const int ic = latch_run - r_start - 1;
            if (ic >= 0 && ic < cnt) {
                const unsigned long long upto = (2ull << ic) - 1ull;        // bits 0..ic (all ones for ic = 63)
                if ((N & upto) == upto) S |= 1ull << ic;
            }
        }
        const int ne = __popcll(E), ns = __popcll(S);
        {
            const int lane = t & 63, wv = t >> 6;
            int ve = ne, vs = ns;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int ue = __shfl_up(ve, o, 64), us = __shfl_up(vs, o, 64);
                if (lane >= o) { ve += ue; vs += us; }
            }
            if (lane == 63) { wave_ev[wv] = ve; wave_sn[wv] = vs; }
            __syncthreads();
            for (int q = 0; q < wv; q++) { ve += wave_ev[q]; vs += wave_sn[q]; }
            cnt_ev[t] = ve;
            cnt_sn[t] = vs;
            __syncthreads();
        }
        if (cnt > 0) {
            ver_base[a >> 6] = carry_sn + cnt_sn[t] - ns;
            snap_mask[a >> 6] = S;
        }
        {
            // The event list, written by the wave together: for each of its 64 slices in turn, lane i takes bit i of the
            // slice's event mask.  (Every thread walking its own slice's bits wrote up to 64 scattered 4-byte stores
            // per lane and instruction: 68 us of this kernel on an all-quiet 65,536-block call, now a handful of
            // contiguous stores per slice.)
            const int eo_mine = carry_ev + cnt_ev[t] - ne;
            const int lane = t & 63;
            const long a_wave = tile0 + (long)(t - lane) * 64;
            unsigned long long todo = __ballot(E != 0ull);                  // slices of this wave that hold events
            for (; todo; todo &= todo - 1ull) {
                const int sl = __ffsll((long long)todo) - 1;                   // wave-uniform
                const unsigned int e_lo = __builtin_amdgcn_readlane((int)(unsigned int)E, sl);
                const unsigned int e_hi = __builtin_amdgcn_readlane((int)(unsigned int)(E >> 32), sl);
                const unsigned long long Es = ((unsigned long long)e_hi << 32) | e_lo;
                const unsigned int v_lo = __builtin_amdgcn_readlane((int)(unsigned int)V, sl);
                const unsigned int v_hi = __builtin_amdgcn_readlane((int)(unsigned int)(V >> 32), sl);
                const unsigned long long Vs = ((unsigned long long)v_hi << 32) | v_lo;
                const int rs = __builtin_amdgcn_readlane(r_start, sl), eos = __builtin_amdgcn_readlane(eo_mine, sl);
                if ((Es >> lane) & 1ull) {
                    const unsigned long long lower = (1ull << lane) - 1ull;
                    const int idx = eos + __popcll(Es & lower);
                    const unsigned long long below = Vs & lower;            // voice bits before this one (this bit is noise)
                    events[idx] = (int)(a_wave + (long)sl * 64 + lane);
                    ev_n[idx] = below ? lane - (63 - __clzll((long long)below)) : rs + lane + 1;
                }
            }
        }
        __syncthreads();
        if (t == 0) {
            carry_run = sum[1023].has_voice ? sum[1023].trailing : run_in + sum[1023].trailing;
            carry_ev += cnt_ev[1023];
            carry_sn += cnt_sn[1023];
        }
        __syncthreads();
    }
    if (t == 0) {
        if (st_out) st_out->run_len = carry_run;
        if (run_len_out) *run_len_out = carry_run;
        plan->n_events = carry_ev;
        plan->n_snap = carry_sn;
    }
}

// ---------------------------------------------------------------------------------------
// The same block in the transform's own layout: q[r] = the sample pair (2 lane + 128 r, +1), four coalesced
// dword loads, nothing to re-lay out.
__device__ __forceinline__ void load_block_pairs(const short *__restrict__ pcm, long n_blocks,
                                                 const DenoiseState *__restrict__ st_in, long j, int lane,
                                                 unsigned int (&q)[4])
{
    const unsigned int *src = nullptr;
    if (j >= 0 && j < n_blocks) src = reinterpret_cast<const unsigned int *>(pcm + j * 512);
    else if (j == -1) src = reinterpret_cast<const unsigned int *>(st_in->prev);
#pragma unroll
    for (int r = 0; r < 4; r++) q[r] = src ? src[lane + 64 * r] : 0u;
}

// ---------------------------------------------------------------------------------------
// A12 (SS:165-193), the noise average: at every EstimateNoiseSpectrum event  A += |X|;  from run length 3 on  A /= 2;  at
// run length 10 the average is latched as the estimate.  Over the events of a call that is a chain of affine maps
// A <- h (A + |X|), h in {1, 1/2}: sequential by definition, and speech is 40-60 % pauses -- a 65,536-block call can hold
// tens of thousands of events.  (Walked one event after the other, one thread per bin, that chain took 0.26 us per event:
// 8.9 ms per 65,536 blocks of a stream that is half pauses, against 0.1 ms for everything else;
// tools/denoise_events_probe.py.)  So the chain is cut into chunks:
//   noise_accum_kernel    one wave per chunk of C consecutive events (C = 1 up to kNoiseChunks events, else
//                         ceil(events / grid)): transforms each event's frame, keeps the chunk's map
//                         A -> alpha A + beta[bin] in registers (alpha a power of two), and writes it once; at a latch it
//                         writes the map so far into the latched row.  No magnitude ever goes to memory.
//   noise_combine_kernel  16 bins per workgroup, 64 groups of chunks per bin: composes each group's maps, walks the 64
//                         group maps from the carried-in average, expands to the average entering every chunk, and
//                         completes the latched rows:  row = alpha_so_far * A_entering_chunk + beta_so_far.
// Multiplying by a power of two commutes with rounding, so with one event per chunk and one chunk per group -- up to 64
// events per call, e.g. any per-block or small-batch streaming use -- the result is bit-identical to the sequential
// walk; beyond that the additions associate differently (1e-7 relative, the same size as FP32 against the reference's FP64).
struct ChunkGeom { int per_chunk, n_chunks; };
__device__ __forceinline__ ChunkGeom chunk_geom(int n_events, int grid)
{
    ChunkGeom g;
    g.per_chunk = n_events > grid ? (n_events + grid - 1) / grid : 1;
    g.n_chunks = (n_events + g.per_chunk - 1) / g.per_chunk;
    return g;
}

__global__ __launch_bounds__(64) void noise_accum_kernel(const short *__restrict__ pcm, long n_blocks,
                                                         const DenoiseState *__restrict__ st_in,
                                                         const int *__restrict__ events, const int *__restrict__ ev_n,
                                                         const DenoisePlan *__restrict__ plan,
                                                         const int *__restrict__ ver_base,
                                                         const unsigned long long *__restrict__ snap_mask,
                                                         const float2 *__restrict__ table, NoiseAccum acc,
                                                         float *__restrict__ noise_rows, int latch_run,
                                                         const int *__restrict__ range, long ext0)
{
    // range (device, or NULL: every event of the plan) = {first event, one past the last, latches before the first} of a
    // sharded run; ext0 = global index of the first block `pcm` holds (sharded runs; st_in is then NULL and never needed)
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    const int lane = threadIdx.x;
    const int e_base = range ? range[0] : 0, row_off = range ? range[2] : 0;
    const int n_events = range ? range[1] - range[0] : plan->n_events;
    const ChunkGeom cg = chunk_geom(n_events, (int)gridDim.x);
    const int chunk = blockIdx.x;
    if (chunk >= cg.n_chunks) return;
    const int e0 = chunk * cg.per_chunk;
    const int e1 = e0 + cg.per_chunk < n_events ? e0 + cg.per_chunk : n_events;
    FrameTables t;
    load_frame_tables(t, table, lane);
    // Pair-owned bins (frame_io.h): |X| of the bins m, m + 512 of m = lane + 64 d, d < 5; the bins 1024 - m and 512 - m
    // are their mirrors (a real frame), so ten magnitudes per lane and event instead of sixteen.  A row is stored as the
    // ten own values plus the mirrors of m = 1..192 (the items of d = 3, 4 mirror each other: those bins are stored by
    // their owners only).
    PairTwiddles pw;
    load_pair_twiddles(pw, table, lane);
    constexpr int ND = 5;
    float blo[ND], bhi[ND], alpha = 1.0f;                        // beta[lane + 64 d], beta[lane + 64 d + 512]
    auto store_row = [&](float *row) {
#pragma unroll
        for (int d = 0; d < ND; d++) { row[lane + 64 * d] = blo[d]; row[lane + 64 * d + 512] = bhi[d]; }
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int m = lane + 64 * d;
            if (m >= 1 && m <= 192) { row[1024 - m] = blo[d]; row[512 - m] = bhi[d]; }
        }
    };
#pragma unroll
    for (int d = 0; d < ND; d++) blo[d] = bhi[d] = 0.0f;
    for (int e = e0; e < e1; e++) {
        const long jg = events[e_base + e], j = jg - ext0;
        const int n = ev_n[e_base + e];
        unsigned int prev[4], cur[4];
        load_block_pairs(pcm, n_blocks, st_in, j - 1, lane, prev);   // rgssKeepBuffer (SS:165-170)
        load_block_pairs(pcm, n_blocks, st_in, j, lane, cur);
        float2 v[8], zr[ND], lo[ND], hi[ND];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float2 s0 = unpack_i16x2(prev[r]), s1 = unpack_i16x2(cur[r]);
            v[r] = make_float2(s0.x * t.win[r].x, s0.y * t.win[r].y);
            v[r + 4] = make_float2(s1.x * t.win[r + 4].x, s1.y * t.win[r + 4].y);
        }
        wave_fft512<false>(v, lds, lane, t.tw);
        wave_lds_fence();
        pair_fetch_lds(v, lds, lane, zr);
#pragma unroll
        for (int d = 0; d < ND; d++) {
            const float2 ev = cadd_conj(v[d], zr[d]), od = csub_conj_mj(v[d], zr[d]);
            const float2 tw = cmul(pw.w[d], od);
            lo[d] = cadd(ev, tw);
            hi[d] = csub(ev, tw);
        }
        const float h = n >= 3 ? 0.5f : 1.0f;                    // SS:182-187
#pragma unroll
        for (int d = 0; d < ND; d++) {
            // hardware square root (1 ulp; sqrtf() expands to ~12 instructions of scaling and fix-up per value, a third
            // of this loop)
            blo[d] = (blo[d] + __builtin_amdgcn_sqrtf(lo[d].x * lo[d].x + lo[d].y * lo[d].y)) * h;
            bhi[d] = (bhi[d] + __builtin_amdgcn_sqrtf(hi[d].x * hi[d].x + hi[d].y * hi[d].y)) * h;
        }
        alpha *= h;
        if (n == latch_run) {                                    // SS:189-193
            const int row = version_of(ver_base, snap_mask, jg) - row_off;
            store_row(noise_rows + (size_t)row * 1024);
            if (lane == 0) { acc.lat_alpha[row] = alpha; acc.lat_chunk[row] = chunk; }
        }
    }
    store_row(acc.chunk_beta + (size_t)chunk * 1024);
    if (lane == 0) acc.chunk_alpha[chunk] = alpha;
}

// grid: n_bins / kCombineBins workgroups of 1024 threads = kCombineBins bins x kCombineGroups chunk groups;
// accum_grid = noise_accum's grid size
#ifndef JDSP_COMBINE_BINS
#define JDSP_COMBINE_BINS 16
#endif
constexpr int kCombineBins = JDSP_COMBINE_BINS, kCombineGroups = 1024 / JDSP_COMBINE_BINS;
// Sharded runs (range != NULL: {first event, one past the last, latches before, latches inside} of this rank): the
// average starts from a_in (NULL: zero), summary (or NULL) receives the rank's composed map {alpha, beta[1024]}, last
// (or NULL) {number of latches, the last latched row}; complete_rows = 0 leaves the latched rows' partial maps alone
// (the first of a rank's two passes: its a_in is not known yet).
__global__ __launch_bounds__(1024) void noise_combine_kernel(const DenoisePlan *__restrict__ plan,
                                                             const DenoiseState *__restrict__ st_in, DenoiseState *st_out,
                                                             NoiseAccum acc, float *__restrict__ noise_rows, int accum_grid,
                                                             const int *__restrict__ range, const float *__restrict__ a_in,
                                                             float *__restrict__ summary, float *__restrict__ last,
                                                             int complete_rows)
{
    __shared__ float ga[kCombineGroups][kCombineBins], gb[kCombineGroups][kCombineBins];
    const int bl = threadIdx.x % kCombineBins, g = threadIdx.x / kCombineBins;
    const int bin = blockIdx.x * kCombineBins + bl;
    const int n_snap = range ? range[3] : plan->n_snap;
    const ChunkGeom cg = chunk_geom(range ? range[1] - range[0] : plan->n_events, accum_grid);
    const int per_group = (cg.n_chunks + kCombineGroups - 1) / kCombineGroups;
    const int c0 = g * per_group < cg.n_chunks ? g * per_group : cg.n_chunks;
    const int c1 = c0 + per_group < cg.n_chunks ? c0 + per_group : cg.n_chunks;
    // The two walks over the group's chunks are chains of one FMA per chunk -- but of one LOAD per chunk too, and a
    // load at a time is a memory latency per chunk (49 us for 4,096 chunks: profiles/r02_denoise_events.txt).  The
    // loads do not depend on the chain: sixteen chunks' values are requested together, then applied in order.
    constexpr int kBatch = 16;
    {
        float a = 1.0f, b = 0.0f;                                 // this group's chunks composed
        for (int cb = c0; cb < c1; cb += kBatch) {
            float al[kBatch], be[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; u++) {
                const int c = cb + u < c1 ? cb + u : c1 - 1;
                al[u] = acc.chunk_alpha[c];
                be[u] = acc.chunk_beta[(size_t)c * 1024 + bin];
            }
#pragma unroll
            for (int u = 0; u < kBatch; u++)
                if (cb + u < c1) { b = al[u] * b + be[u]; a *= al[u]; }
        }
        ga[g][bl] = a;
        gb[g][bl] = b;
    }
    __syncthreads();
    if (summary && blockIdx.x == 0 && threadIdx.x == 0) {
        float p = 1.0f;
        for (int q = 0; q < kCombineGroups; q++) p *= ga[q][0];
        summary[0] = p;                                          // alpha = 2^-(number of halvings)
    }
    float A = a_in ? a_in[bin] : (st_in ? st_in->avg[bin] : 0.0f);
    for (int q = 0; q < g; q++) A = ga[q][bl] * A + gb[q][bl];   // the average entering this group
    for (int cb = c0; cb < c1; cb += kBatch) {
        float al[kBatch], be[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
            const int c = cb + u < c1 ? cb + u : c1 - 1;
            al[u] = acc.chunk_alpha[c];
            be[u] = acc.chunk_beta[(size_t)c * 1024 + bin];
        }
#pragma unroll
        for (int u = 0; u < kBatch; u++)
            if (cb + u < c1) {
                acc.a_start[(size_t)(cb + u) * 1024 + bin] = A;
                A = al[u] * A + be[u];
            }
    }
    if (g == kCombineGroups - 1) {                               // groups past the last chunk are identities
        if (st_out) st_out->avg[bin] = A;
        if (summary) summary[1 + bin] = A;
    }
    if (g == 0 && st_in) noise_rows[bin] = st_in->noise[bin];    // row 0: the estimate carried in
    __syncthreads();                                             // a_start is read back by other threads of this workgroup
    if (complete_rows)
        for (int r = 1 + g; r <= n_snap; r += kCombineGroups) {
            float *row = noise_rows + (size_t)r * 1024 + bin;
            *row = acc.lat_alpha[r] * acc.a_start[(size_t)acc.lat_chunk[r] * 1024 + bin] + *row;
        }
    __syncthreads();
    if (g == 0) {
        if (st_out) st_out->noise[bin] = n_snap > 0 ? noise_rows[(size_t)n_snap * 1024 + bin] : st_in->noise[bin];
        if (last) {
            last[1 + bin] = n_snap > 0 ? noise_rows[(size_t)n_snap * 1024 + bin] : 0.0f;
            if (bin == 0) last[0] = (float)n_snap;
        }
    }
}

// ---------------------------------------------------------------------------------------
// A8 (SS:233-242): Y = (|X| - N) e^{j phase(X)}; no clamp at zero; X == 0 -> phase 0 -> (-N, 0).
// A9 (WF:196-213): Y = |X| (1 - min(1, N^2/|X|^2)) e^{j phase(X)}; 0/0 stays NaN as in the reference.
//
// Which spectral-subtraction frames FP32 cannot hold.  In a bin far below its noise value the output is -N e^{j phase(X)}:
// its size is N however small X is, and its direction is the phase of X -- which a FP32 transform leaves arbitrary once
// |X| is at its own rounding, eps = 2^-23 sqrt(E) per bin (E = the energy of the windowed samples that share the
// transform; tests/mfcc_fp32_ref.py pins that constant for these radix-8 passes).  Rounding eps in X[k] moves Y[k] by
// eps along X (the gain is near 1 or below) and by eps N / |X| across it, so the frame's samples are off, relative to
// their own root mean square (Parseval on both sides), by
//     rho^2 = eps^2 sum_k (1 + (N_k / |X_k|)^2) / sum_k |Y_k|^2 .
// q = N / |X| is the gain's own subtrahend; E is summed over the windowed samples before the forward transform and
// sum |Y|^2 = n_fft sum y^2 over the samples after the inverse one, and each sum goes through the wave to a scalar
// register as soon as it is complete, so nothing of this stays in vector registers across a transform.  A frame with
// rho above kPhaseRho = half the project's bar of 1e-5 is computed again in FP64 (denoise_redo_f64_kernel);
// tests/denoise_fp32_ref.py restates rho and the FP32 chain on the CPU, where no frame with rho under 9.9e-6 misses
// half its bar: a margin of two (the constant was not tuned on the device).  Wiener's gain has no such amplifier (its
// term is (1 + 2 r)^2, r = min(1, N^2 / |X|^2)); only the 512-point kernels evaluate it, for the partner's rounding.  Bins 0 and n_fft / 2 of a real frame are real: rounding cannot turn them, only flip their
// sign, and only when they are at the rounding itself; they count when |X| < 16 eps.  A bin FP32 rounded to exactly
// zero counts as q = infinity (or NaN); an all-zero transform (E = 0) is exact.  Two 512-point frames that share a
// transform share its rounding: E is the pair's, and the 1 in the sum is what a quiet frame takes from a loud partner.
struct PhaseStat { float e, err; };        // wave-uniform: sum |v|^2 of the transform's input (= E / 4: the window is halved), sum (1 + q^2)
#ifndef JDSP_PHASE_RHO
#define JDSP_PHASE_RHO 5.0e-6f
#endif
constexpr float kPhaseRho = JDSP_PHASE_RHO;
// rho^2 > kPhaseRho^2  <=>  err * e * phase_k() > sum y^2, with e = E / 4
template <int NFFT>
__device__ __forceinline__ constexpr float phase_k() { return 4.0f * 1.4210854715202004e-14f / ((float)NFFT * kPhaseRho * kPhaseRho); }
// a real bin counts when |X|^2 < (16 eps)^2 = kRealBinK e: a lane's threshold for the bins that may be real
constexpr float kRealBinK = 256.0f * 4.0f * 1.4210854715202004e-14f;
__device__ __forceinline__ float real_bin_thr(float e, bool real) { return real ? kRealBinK * e : __builtin_inff(); }

// the frame's verdict; ysq = this lane's share of sum y^2 over the frame's samples
template <int NFFT>
__device__ __forceinline__ bool phase_unsafe(float e, float err, float ysq)
{
    return e > 0.0f && !(err * e * phase_k<NFFT>() <= wave_sum_f32(ysq));
}
__device__ __forceinline__ float sumsq(const float2 (&v)[8])
{
    float a = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; r++) a += v[r].x * v[r].x + v[r].y * v[r].y;
    return a;
}

// one frame more on the list {count, frames...} of denoise_redo_f64_kernel
__device__ __forceinline__ void phase_redo(int *__restrict__ redo, long j, int lane)
{
    if (lane == 0) redo[1 + atomicAdd(redo, 1)] = (int)j;
}

// One frame: samples -> y = IDFT(gain(DFT(window * frame))) / 1024, returned in the transform layout: y[d] =
// (y[2 lane + 128 d], y[2 lane + 128 d + 1]).  Every mirror pair of bins is owned by one lane (frame_io.h,
// PairTwiddles): five items per lane, the gain evaluated on the 640 bins m, m + 512 (m = lane + 64 d, d < 5) and the
// rest of the inverse transform's input taken from the Hermitian symmetry -- which holds because the gain is real and
// N[1024 - k] = N[k] up to the rounding of the estimate (|X[k]| and |X[1024 - k]| of a real frame, 1e-7 apart in
// FP32; the reference's own FFTW spectrum is symmetric to 1e-16).  The reference's 1/1024 after the inverse transform
// (SS:248, a power of two: exact wherever it is applied) is folded into the gain, so the noise values arrive
// pre-multiplied by it.
struct NoisePairRegs { float lo[5], hi[5]; };
template <int MODE>
__device__ __forceinline__ void load_noise_pair_regs(NoisePairRegs &n, const float *__restrict__ row, int lane)
{
    // spectral subtraction: N / 1024; Wiener: N as is (its gain is a ratio)
    const float sc = MODE == 0 ? (1.0f / 1024.0f) : 1.0f;
#pragma unroll
    for (int d = 0; d < 5; d++) { n.lo[d] = sc * row[lane + 64 * d]; n.hi[d] = sc * row[lane + 64 * d + 512]; }
}

// The gain of one bin (A8 / A9 above) times 2^-LOG2N, the reference's 1/n_fft (1024 or 512): x is the bin, n its noise
// value as load_noise_pair_regs left it (spectral subtraction: already scaled).  err collects the bin's term of
// phase_unsafe's sum, scaled by 2^-2 LOG2N; w: how many bins of the spectrum this value stands for (a lane that owns a
// mirror pair evaluates one of the two); maybe_real: the bin may be one of the two real ones, which count only under
// rthr (real_bin_thr).  Hardware reciprocal / reciprocal square root (1 ulp): the bar is 1e-5, not IEEE division.
template <int MODE, int LOG2N = 10>
__device__ __forceinline__ float2 apply_gain_scaled(float2 x, float n, float &err, float w, bool maybe_real = false,
                                                    float rthr = 0.0f)
{
    const float c = 1.0f / (float)(1 << LOG2N);
    const float p = x.x * x.x + x.y * x.y;
    if (MODE == 0) {
        const float q = n * __frsqrt_rn(p);                   // N / (1024 |X|); p == 0 gives inf / NaN: the frame goes to FP64
        const float g = c - q;                                  // (|X| - N) / (1024 |X|); p == 0: replaced below
        const bool zero = p == 0.0f;
        if (maybe_real) w = p < rthr ? w : 0.0f;                // (maybe_real is a compile-time fact of every call)
        err += w * (q * q + c * c);
        return make_float2(zero ? -n : x.x * g, zero ? 0.0f : x.y * g);
    } else {
        // v_rcp_f32 (1 ulp; __frcp_rn() expands to the IEEE division sequence, a dozen instructions per bin)
        float r = (n * n) * __builtin_amdgcn_rcpf(p);                    // 0 * inf = NaN keeps the reference's 0/0
        if (r >= 1.0f) r = 1.0f;
        const float g = c - c * r;
        const float t = c + 2.0f * c * r;                       // Wiener: rounding eps in X moves Y by at most (1 + 2 r) eps
        err += w * (t * t);
        return make_float2(x.x * g, x.y * g);
    }
}

template <int MODE>
__device__ __forceinline__ void denoise_frame_pairs(const unsigned int *raw, const FrameTables &t, const PairTwiddles &pw_regs,
                                                    const float2 *__restrict__ table, float2 *lds, int lane,
                                                    const NoisePairRegs &n, float2 (&y)[8], PhaseStat &ps)
{
    // Spectral subtraction's criterion sums (phase_unsafe) need registers the persistent wave does not have at four
    // waves per SIMD (kept for the run, the tables and the sums spill: 28 to 188 bytes per lane in every arrangement
    // tried).  There the window and the five pair twiddles are fetched per frame (6.5 KB per wave, the same lines
    // every frame: L1 hits) instead of being kept for the whole run: 125 registers, no scratch.
    PairTwiddles pw_frame;
    int pl = lane;
    if (MODE == 0) {
        asm volatile("" : "+v"(pl));                            // per frame: not a loop invariant to hoist (and spill)
        load_pair_twiddles(pw_frame, table, pl);
    }
    const PairTwiddles &pw = MODE == 0 ? pw_frame : pw_regs;
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const float2 s = unpack_i16x2(raw[r]);
        const float2 w = MODE == 0 ? table[kStftWin + pl + 64 * r] : t.win[r];
        v[r] = make_float2(s.x * w.x, s.y * w.y);
    }
    if (MODE == 0) ps.e = wave_sum_f32(sumsq(v));
    float err = 0.0f;
    wave_fft512<false>(v, lds, lane, t.tw);
    float2 zr[5], ret[4];
    wave_lds_fence();                                            // the transform's last exchange reads are done
    pair_fetch_lds(v, lds, lane, zr);
#pragma unroll
    for (int d = 0; d < 5; d++) {
        const float2 e = cadd_conj(v[d], zr[d]);
        const float2 o = csub_conj_mj(v[d], zr[d]);
        const float2 p = cmul(pw.w[d], o);
        // bins m and m + 512 stand for their mirrors 1024 - m and 512 - m too where those have no owner: m = 1..192
        const float w = d < 3 ? ((d == 0 && lane == 0) ? 1.0f : 2.0f) : ((d == 3 && lane == 0) ? 2.0f : 1.0f);
        const float rthr = real_bin_thr(ps.e, lane == 0);       // d == 0, lane 0: the bins 0 and 512
        const float2 lo = apply_gain_scaled<MODE>(cadd(e, p), n.lo[d], err, w, d == 0, rthr);      // Y[m] / 1024
        const float2 hi = apply_gain_scaled<MODE>(csub(e, p), n.hi[d], err, w, d == 0, rthr);      // Y[m + 512] / 1024
        if (d < 4) {
            presplit_inv_pair(lo, hi, pw.w[d], y[d], ret[d]);
        } else {
            y[d] = presplit_inv_reg(lo, hi, pw.w[d]);
        }
    }
    if (MODE == 0) ps.err = wave_sum_f32(err) * 1048576.0f;            // the gain's 2^-20 undone
    pair_return_lds(ret, lds, lane, y);
    wave_fft512<true>(y, lds, lane, t.tw);
    wave_lds_fence();
}

// Every wave of a run kernel walks the priority levels, one step per loop iteration (see fastconv1024_pairs_kernel: a
// SIMD serves equal-priority waves by age, and equal shares then finish far apart).  s_setprio takes an immediate.
__device__ __forceinline__ void step_priority(unsigned &prio_step)
{
    switch (prio_step++ & 3u) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}

// Which noise row block j (local index) uses.  Single-GPU: the plan's version.  Sharded
// (DenoiseShard): the plan is indexed by GLOBAL block number and the local row table starts at
// the estimate in effect at the block before the shard (row 0).
__device__ __forceinline__ const float *noise_row(const float *__restrict__ rows, const int *__restrict__ ver_base,
                                                  const unsigned long long *__restrict__ snap_mask, long j,
                                                  const DenoiseShard &sh)
{
    int v = version_of(ver_base, snap_mask, j + sh.ver_block_off);
    if (sh.ver_row_off) v -= *sh.ver_row_off;
    if (v < 0) v = 0;
    return rows + (size_t)v * 1024;
}
// The same with *sh.ver_row_off read once by the caller (a persistent wave's loop: read inside it, that load is a
// vector load with an s_waitcnt vmcnt(0) behind it -- which also waits for the block prefetch issued just before)
__device__ __forceinline__ const float *noise_row_at(const float *__restrict__ rows, const int *__restrict__ ver_base,
                                                     const unsigned long long *__restrict__ snap_mask, long j,
                                                     long ver_block_off, int row_off)
{
    int v = version_of(ver_base, snap_mask, j + ver_block_off) - row_off;
    if (v < 0) v = 0;
    return rows + (size_t)v * 1024;
}

// A8/A9/A10 for a call's blocks: one wave walks `run` consecutive blocks, and the launch picks `run` so that the whole
// batch is ONE round of resident waves (resident_run; the handle's "blocks_per_wave" option sets it instead).  Waves
// that come in several rounds leave wave slots idle at the end of the last one -- with 8 blocks per wave a 65,536-block
// batch was 8,192 waves = 2.67 rounds of the 3,072 then resident, 27 frame times per wave slot for 24 of work -- and
// every wave pays one halo frame, 1/run of its work.  The frame of block j is [block j - 1, block j]; a wave's first
// output needs the second half of the frame before it, so that halo frame (js = j0 - 1) goes through the SAME loop
// body as every other frame with emission off: one inlined copy of the arithmetic, so the samples do not depend on
// where the waves, or the calls, are cut.  No halo where the call's first block takes the carried overlap (j0 == 0)
// or the frame before is the stream's void first one.  A wave needs the next block's samples only one iteration
// later, so they are loaded at the top of the iteration that precedes their use (4 dwords per lane).
#ifndef JDSP_DENOISE_RESIDENT
#define JDSP_DENOISE_RESIDENT 4      // waves per SIMD the run kernel's register budget allows
#endif
template <int MODE>
__global__ __launch_bounds__(64, JDSP_DENOISE_RESIDENT) void denoise_run_kernel(
    const short *__restrict__ pcm, long n_blocks, long calls_before, const DenoiseState *__restrict__ st_in,
    DenoiseState *st_out, const int *__restrict__ ver_base, const unsigned long long *__restrict__ snap_mask,
    const float *__restrict__ noise_rows, const float2 *__restrict__ table, short *__restrict__ out,
    float *__restrict__ precast, DenoiseShard sh, int run, int *__restrict__ redo)
{
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    const int lane = threadIdx.x;
    PhaseStat ps;
    const long per_xcd = (gridDim.x + 7) >> 3;                // XCD-aware run order (speed only)
    const long j0 = ((long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3)) * run;
    if (j0 >= n_blocks) return;
    const long j1 = j0 + run < n_blocks ? j0 + run : n_blocks;

    FrameTables t;
    load_frame_tables(t, table, lane);
    PairTwiddles sw;
    load_pair_twiddles(sw, table, lane);
    NoisePairRegs nz;

    unsigned int raw[8], nxt[4], tk[4];
    float2 tail[4], y[8];
    const float *cur_row = nullptr;
    const int row_off = sh.ver_row_off ? *sh.ver_row_off : 0;          // once: see noise_row_at
    const long js = (j0 == 0 || calls_before + j0 - 1 == 0) ? j0 : j0 - 1;
    if (j0 == 0) {
        // rgsdOveraped[512..1023] carried over from the previous call
#pragma unroll
        for (int d = 0; d < 4; d++) tail[d] = *reinterpret_cast<const float2 *>(&st_in->tail[2 * lane + 128 * d]);
    } else {
        // empty: the halo frame fills it, or the stream's first call only stashed its block (SS:211-216)
#pragma unroll
        for (int d = 0; d < 4; d++) tail[d] = make_float2(0.f, 0.f);
    }
    load_block_pairs(pcm, n_blocks, st_in, js - 1, lane, nxt);
#pragma unroll
    for (int r = 0; r < 4; r++) raw[r + 4] = nxt[r];
    load_block_pairs(pcm, n_blocks, st_in, js, lane, tk);
    const long first_emit = sh.emit_from;                     // SS:260-263: calls 1 and 2 emit nothing
    unsigned prio_step = blockIdx.x >> 10;                    // step_priority: one step per block
    // vmcnt counts loads and stores together, in issue order, and across the loop's back edge the compiler waits for
    // vmcnt(0): taking the prefetched block at the TOP of an iteration waited for the previous block's output stores to
    // complete, every block.  It is taken (tk <- nxt) just before this block's stores instead (see fastconv1024_pairs_kernel).
    for (long j = js; j < j1; j++) {
        step_priority(prio_step);
        unsigned int cur[4];
#pragma unroll
        for (int r = 0; r < 4; r++) { cur[r] = tk[r]; raw[r] = raw[r + 4]; raw[r + 4] = tk[r]; }
        if (j + 1 < j1) load_block_pairs(pcm, n_blocks, st_in, j + 1, lane, nxt);      // needed one iteration from now
        if (calls_before + j == 0) {
#pragma unroll
            for (int d = 0; d < 8; d++) y[d] = make_float2(0.f, 0.f);
        } else {
            const float *row = noise_row_at(noise_rows, ver_base, snap_mask, j, sh.ver_block_off, row_off);
            if (row != cur_row) {                                // wave-uniform: a new estimate was latched
                cur_row = row;
                load_noise_pair_regs<MODE>(nz, row, lane);
            }
            denoise_frame_pairs<MODE>(raw, t, sw, table, lds, lane, nz, y, ps);
            // a frame FP32 cannot hold (phase_unsafe): again, in FP64, if one of its two blocks is emitted (the halo
            // frame is listed by the wave that owns it)
            if (MODE == 0 && j >= j0 && j + 1 >= sh.emit_from && phase_unsafe<1024>(ps.e, ps.err, sumsq(y))) phase_redo(redo, j, lane);
        }
        float2 o[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            o[d] = make_float2(tail[d].x + y[d].x, tail[d].y + y[d].y);      // SS:248 overlap-add
            tail[d] = y[d + 4];                                               // SS:255-256
        }
#pragma unroll
        for (int r = 0; r < 4; r++) { tk[r] = nxt[r]; asm volatile("" : "+v"(tk[r])); }
        __builtin_amdgcn_sched_barrier(0);
        if (j >= j0 && j >= first_emit && j < sh.emit_to) {
            const long oi = j - first_emit;
            unsigned int *dst = reinterpret_cast<unsigned int *>(out + oi * 512) + lane;
#pragma unroll
            for (int d = 0; d < 4; d++)                      // four coalesced 256-byte stores, in the layout as is
                __builtin_nontemporal_store(cast_i16x2_bits(o[d].x, o[d].y), dst + 64 * d);
            if (precast) {
#pragma unroll
                for (int d = 0; d < 4; d++) *reinterpret_cast<float2 *>(precast + oi * 512 + 2 * lane + 128 * d) = o[d];
            }
        }
        if (j == n_blocks - 1) {
#pragma unroll
            for (int r = 0; r < 4; r++) reinterpret_cast<unsigned int *>(st_out->prev)[lane + 64 * r] = cur[r];   // SS:257
#pragma unroll
            for (int d = 0; d < 4; d++) *reinterpret_cast<float2 *>(&st_out->tail[2 * lane + 128 * d]) = tail[d];
        }
    }
}

// ---------------------------------------------------------------------------------------
// Multi-GPU sharding of the noise estimate.  Rank r owns blocks [b0, b1) of the
// global stream.  The run-length plan is replicated (every rank runs plan_kernel over the
// all-gathered voice flags); the running average A (SS:182-187) is an affine recurrence
// A <- a*A + b over the events, so each rank reduces its own events to one (alpha, beta[1024])
// pair, the pairs are all-gathered, and every rank folds the pairs of the ranks before it to get
// the A it starts from.  Latched estimates (SS:189-193) are then absolute, and only the last
// one per rank has to travel.
__global__ void event_range_kernel(const int *__restrict__ events, const DenoisePlan *__restrict__ plan,
                                   const int *__restrict__ ver_base, const unsigned long long *__restrict__ snap_mask,
                                   long b0, long b1, int *__restrict__ range)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int n = plan->n_events;
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (events[mid] < b0) lo = mid + 1; else hi = mid; }
    range[0] = lo;
    hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (events[mid] < b1) lo = mid + 1; else hi = mid; }
    range[1] = lo;
    range[2] = b0 > 0 ? version_of(ver_base, snap_mask, b0 - 1) : 0;     // latches before the shard = row offset
    range[3] = (b1 > b0 ? version_of(ver_base, snap_mask, b1 - 1) : range[2]) - range[2];   // latches inside it
}

// A entering rank `rank` = the pairs of the ranks before it applied in order.
__global__ __launch_bounds__(256) void fold_summaries_kernel(const float *__restrict__ all, int rank, float *__restrict__ a_in)
{
    const int bin = blockIdx.x * blockDim.x + threadIdx.x;
    float a = 0.f;
    for (int q = 0; q < rank; q++) a = all[(size_t)q * 1025] * a + all[(size_t)q * 1025 + 1 + bin];
    a_in[bin] = a;
}

// rows[0] = the estimate in effect at the block before the shard: the last latch of the nearest
// earlier rank that has one (zeros if none: rgdEstimatedNS starts at 0, SS:70).
__global__ __launch_bounds__(256) void select_row0_kernel(const float *__restrict__ last_all, int rank, float *__restrict__ rows)
{
    const int bin = blockIdx.x * blockDim.x + threadIdx.x;
    float v = 0.f;
    for (int q = rank - 1; q >= 0; q--)
        if (last_all[(size_t)q * 1025] > 0.f) { v = last_all[(size_t)q * 1025 + 1 + bin]; break; }
    rows[bin] = v;
}

// ---------------------------------------------------------------------------------------
// block_len 512, or 256 (frames of 512); w_hi = the second half of the FP64 Hamming(2 block_len)
int launch_vad(hipStream_t s, int block_len, const short *pcm, long n_blocks, const double *w_hi, int use_zcr,
               unsigned char *flags, long long *dbg_energy, int *dbg_zcr)
{
    if (n_blocks <= 0) return 0;
    const dim3 grid((unsigned)((n_blocks + kVadBlocksPerWave - 1) / kVadBlocksPerWave));
    const bool trace = dbg_energy || dbg_zcr;
    if (block_len == 512) {
        if (!trace) hipLaunchKernelGGL(vad_flags_kernel<8>, grid, dim3(64), 0, s, pcm, n_blocks, w_hi, use_zcr, flags);
        else hipLaunchKernelGGL(vad_kernel<8>, grid, dim3(64), 0, s, pcm, n_blocks, w_hi, use_zcr, flags, dbg_energy, dbg_zcr);
    } else {
        if (!trace) hipLaunchKernelGGL(vad_flags_kernel<4>, grid, dim3(64), 0, s, pcm, n_blocks, w_hi, use_zcr, flags);
        else hipLaunchKernelGGL(vad_kernel<4>, grid, dim3(64), 0, s, pcm, n_blocks, w_hi, use_zcr, flags, dbg_energy, dbg_zcr);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_denoise_plan(hipStream_t s, const unsigned char *flags, long n_blocks, const DenoiseState *st_in,
                        DenoiseState *st_out, int *ver_base, unsigned long long *snap_mask, int *events, int *ev_n,
                        DenoisePlan *plan)
{
    hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(1024), 0, s, flags, n_blocks, &st_in->run_len, st_out, ver_base,
                       snap_mask, events, ev_n, plan, 10, (int *)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the same scan for callers with their own state layout (mvdr_kernels.hip)
int launch_run_plan(hipStream_t s, const unsigned char *flags, long n_blocks, const int *run_len_in, int *run_len_out,
                    int latch_run, int *ver_base, unsigned long long *snap_mask, int *events, int *ev_n,
                    DenoisePlan *plan)
{
    hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(1024), 0, s, flags, n_blocks, run_len_in, (DenoiseState *)nullptr,
                       ver_base, snap_mask, events, ev_n, plan, latch_run, run_len_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Blocks per wave of the run kernels (denoise_run_kernel, denoise_batch_kernel) for one round of resident waves:
// JDSP_DENOISE_RESIDENT per SIMD, 4 SIMDs per CU; never fewer than 4 blocks per wave (a quarter of halo overhead at
// most).  The grid is ceil(n_blocks / run) waves, rounded up to eight.
static long resident_run(int n_cu, long n_blocks)
{
    const long slots = (long)(n_cu > 0 ? n_cu : 256) * 4 * JDSP_DENOISE_RESIDENT;
    long waves = (n_blocks + 3) / 4;
    if (waves > slots) waves = slots;
    return (n_blocks + waves - 1) / waves;
}

static int launch_denoise1024(hipStream_t s, int mode, int k_opt, int n_cu, const short *pcm, long n_blocks,
                             long calls_before, const DenoiseState *st_in, DenoiseState *st_out, const int *ver_base,
                             const unsigned long long *snap_mask, const float *noise_rows, const float2 *table, short *out,
                             float *precast, const DenoiseShard &sh, int *redo)
{
    const long run = k_opt > 0 ? k_opt : resident_run(n_cu, n_blocks);
    const long grid = ((n_blocks + run - 1) / run + 7) / 8 * 8;
    if (mode == 0)
        hipLaunchKernelGGL(denoise_run_kernel<0>, dim3((unsigned)grid), dim3(64), 0, s, pcm, n_blocks, calls_before, st_in,
                           st_out, ver_base, snap_mask, noise_rows, table, out, precast, sh, (int)run, redo);
    else
        hipLaunchKernelGGL(denoise_run_kernel<1>, dim3((unsigned)grid), dim3(64), 0, s, pcm, n_blocks, calls_before, st_in,
                           st_out, ver_base, snap_mask, noise_rows, table, out, precast, sh, (int)run, redo);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// =======================================================================================
// FFT_PROCESSING_SIZE 512, BLOCK_LEN = KEEP_LEN 256 -- the same programs with the macros of SS:53-55 / WF:42-44 at
// half their values, which is how BASELINE config 3 words the workload ("512-pt STFT 50 % hop").
//
// A 512-sample real frame is half of the wave transform's work, so TWO consecutive frames ride one 512-point
// complex transform: z[n] = a[n] + j b[n] (both already windowed), Z = FFT512(z), and
//     A[k] = (Z[k] + conj Z[512-k]) / 2,      B[k] = -j (Z[k] - conj Z[512-k]) / 2
// are the two frames' spectra (the 1/2 is folded into the window table, as everywhere).  Every lane owns the bin
// pairs (k, 512-k), k = lane + 64 q, so A[512-k] = conj A[k] costs nothing; the per-bin gain (SS:233-242 /
// WF:196-213) is applied to both frames and to both bins of a pair with their own N[k], N[512-k]; the gained
// spectra go back into ONE inverse transform as Y = Ya + j Yb, whose real and imaginary parts are the two frames'
// time signals (both spectra are Hermitian).  Overlap-add with hop 256 pairs "lane + 64 d" registers exactly as
// the 1024-point kernel does with hop 512: y[d], d < 4, is the first half of a frame, y[d + 4] its second half.
//
// One wave owns an odd run of consecutive blocks: pairs (j0-1, j0), (j0+1, j0+2), ...; the first frame of the first pair
// is the halo that rebuilds the overlap tail (its output block belongs to the previous wave).

// Sample s of this call's stream; s in [-256, 0) is the previous call's last block (state), anything else
// outside the call is silence.  s = base + lane + 64 t with base a multiple of 256: every branch is wave-uniform.
__device__ __forceinline__ float dn512_sample(const short *__restrict__ pcm, long n_samples,
                                              const DenoiseState *__restrict__ st_in, long s)
{
    if (s >= 0) return s < n_samples ? (float)pcm[s] : 0.f;
    if (s >= -256 && st_in) return (float)st_in->prev[256 + s];
    return 0.f;
}

// z = (a + j b) * window -> natural-order image of Zh = FFT512(z) in LDS (slot 512 = slot 0)
__device__ __forceinline__ void dn512_forward(const float (&xa)[8], const float (&xb)[8], const float (&win)[8],
                                              const WaveTwiddles &tw, float2 *lds, int lane)
{
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) v[r] = make_float2(xa[r] * win[r], xb[r] * win[r]);
    wave_fft512<false>(v, lds, lane, tw);
    store_natural_image(lds, lane, v);
    wave_lds_fence();
}

// A12 on 512-point frames, chunked like noise_accum_kernel; events e and e + 1 of a chunk share a transform (frame pair
// a + j b).  |X[512 - k]| = |X[k]| of a real frame: lane l keeps the maps of bins l + 64 q (q < 4) and writes each to its
// mirror bin as well (the carried-in average is symmetric for the same reason); bin 256 is lane 0's.
__global__ __launch_bounds__(64) void noise_accum512_kernel(const short *__restrict__ pcm, long n_blocks,
                                                            const DenoiseState *__restrict__ st_in,
                                                            const int *__restrict__ events, const int *__restrict__ ev_n,
                                                            const DenoisePlan *__restrict__ plan,
                                                            const int *__restrict__ ver_base,
                                                            const unsigned long long *__restrict__ snap_mask,
                                                            const float2 *__restrict__ table,
                                                            const float *__restrict__ win512, NoiseAccum acc,
                                                            float *__restrict__ noise_rows, int latch_run,
                                                            const int *__restrict__ range, long ext0)
{
    // range / ext0: a sharded run's slice of the event list and the global index of pcm's first block, as in
    // noise_accum_kernel (st_in is then NULL: a rank's events never reach back past its halo)
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    const int lane = threadIdx.x;
    const int e_base = range ? range[0] : 0, row_off = range ? range[2] : 0;
    const int n_events = range ? range[1] - range[0] : plan->n_events;
    const ChunkGeom cg = chunk_geom(n_events, (int)gridDim.x);
    const int chunk = blockIdx.x;
    if (chunk >= cg.n_chunks) return;
    const int e0 = chunk * cg.per_chunk;
    const int e1 = e0 + cg.per_chunk < n_events ? e0 + cg.per_chunk : n_events;
    WaveTwiddles tw;
    load_wave_twiddles(tw, table, lane);
    float win[8];
#pragma unroll
    for (int r = 0; r < 8; r++) win[r] = win512[lane + 64 * r];
    const long n_samples = n_blocks * 256;
    float b[4] = {0.f, 0.f, 0.f, 0.f}, b256 = 0.f, alpha = 1.0f;
    auto put = [&](float *row) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = lane + 64 * q;
            row[k] = b[q];
            row[(512 - k) & 511] = b[q];
        }
        if (lane == 0) row[256] = b256;
    };
    auto step = [&](const float (&m)[4], float m256, int e) {
        const int n = ev_n[e_base + e];
        const float h = n >= 3 ? 0.5f : 1.0f;                    // SS:182-187
#pragma unroll
        for (int q = 0; q < 4; q++) b[q] = (b[q] + m[q]) * h;
        b256 = (b256 + m256) * h;
        alpha *= h;
        if (n == latch_run) {                                    // SS:189-193
            const int row = version_of(ver_base, snap_mask, events[e_base + e]) - row_off;
            put(noise_rows + (size_t)row * 1024);
            if (lane == 0) { acc.lat_alpha[row] = alpha; acc.lat_chunk[row] = chunk; }
        }
    };
    for (int e = e0; e < e1; e += 2) {
        const int ea = e, eb = e + 1 < e1 ? e + 1 : e;
        const long sa = ((long)events[e_base + ea] - ext0 - 1) * 256, sb = ((long)events[e_base + eb] - ext0 - 1) * 256;   // [previous block, block] (SS:165-170)
        float xa[8], xb[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            xa[r] = dn512_sample(pcm, n_samples, st_in, sa + lane + 64 * r);
            xb[r] = dn512_sample(pcm, n_samples, st_in, sb + lane + 64 * r);
        }
        dn512_forward(xa, xb, win, tw, lds, lane);
        float ma[4], mb[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = lane + 64 * q;
            const float2 zk = lds[k], zm = lds[512 - k];
            const float2 A = cadd_conj(zk, zm), B = csub_conj_mj(zk, zm);
            ma[q] = __builtin_amdgcn_sqrtf(A.x * A.x + A.y * A.y);      // hardware square root, 1 ulp (see noise_accum_kernel)
            mb[q] = __builtin_amdgcn_sqrtf(B.x * B.x + B.y * B.y);
        }
        const float2 z = lds[256];
        wave_lds_fence();
        step(ma, fabsf(2.f * z.x), ea);
        if (eb != ea) step(mb, fabsf(2.f * z.y), eb);
    }
    put(acc.chunk_beta + (size_t)chunk * 1024);
    if (lane == 0) acc.chunk_alpha[chunk] = alpha;
}

// The spectrum stays in registers and every mirror pair of bins is owned by one lane (frame_io.h, pair_fetch_lds /
// pair_return_lds): after the forward transform lane l works on k = l + 64 d, d < 5 -- A[k], B[k] from Z[k] and
// Z[512 - k], ONE gain per frame and bin (N[512 - k] = N[k]: the estimate of a real frame's spectrum is symmetric by
// construction, noise_accum512_kernel writes both from one value), Z'[k] = Ya + j Yb kept and Z'[512 - k] =
// conj(Ya - j Yb) sent to its owner.  Ten gains per lane and frame pair, no natural-order image and no Y image; the wave
// is persistent over `run` consecutive blocks (run odd), keeps both frames' noise values in registers until the estimate
// changes, and requests the next pair's two new blocks before this pair's arithmetic.  The reference's 1/512 (SS:248) is
// folded into the gain.  (Against a fixed seven blocks per wave with LDS images: profiles/r02_denoise512_run.txt.)
template <int MODE>
__device__ __forceinline__ void load_noise512_regs(float (&n)[5], const float *__restrict__ row, int lane)
{
    const float sc = MODE == 0 ? (1.0f / 512.0f) : 1.0f;
#pragma unroll
    for (int d = 0; d < 5; d++) n[d] = sc * row[(lane + 64 * d) & 511];   // d = 4: bins 256..319 (bin k and 512 - k share a value)
}

// waves per SIMD: spectral subtraction fits 128 registers; Wiener with its NaN isolation does not (spills at 128:
// 97 us against 89 us at three waves, profiles/r02_denoise512_run.txt)
#define JDSP_DENOISE512_WAVES(MODE) ((MODE) == 0 ? 4 : 3)
template <int MODE>
__global__ __launch_bounds__(64, JDSP_DENOISE512_WAVES(MODE)) void denoise512_run_kernel(
    const short *__restrict__ pcm, long n_blocks, long calls_before, const DenoiseState *__restrict__ st_in,
    DenoiseState *st_out, const int *__restrict__ ver_base, const unsigned long long *__restrict__ snap_mask,
    const float *__restrict__ noise_rows, const float2 *__restrict__ table, const float *__restrict__ win512,
    short *__restrict__ out, float *__restrict__ precast, DenoiseShard sh, int run, int *__restrict__ redo)
{
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    const int lane = threadIdx.x;
    const long per_xcd = (gridDim.x + 7) >> 3;                // XCD-aware run order (speed only)
    const long j0 = ((long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3)) * run;
    if (j0 >= n_blocks) return;
    const long j1 = j0 + run < n_blocks ? j0 + run : n_blocks;
    const long n_samples = n_blocks * 256;
    WaveTwiddles tw;
    load_wave_twiddles(tw, table, lane);
    float win[8];
#pragma unroll
    for (int r = 0; r < 8; r++) win[r] = win512[lane + 64 * r];

    // blocks ja - 1, ja, ja + 1 of the current pair (ja, ja + 1), samples lane + 64 t of each
    // (the next pair's blocks stay raw halfwords until the rotation at the bottom of the loop: a conversion next to the
    // loads sits inside their wave-uniform branch, and the s_waitcnt with it -- the "prefetch" then costs a full memory
    // round trip per pair before the transforms start)
    float xk[3][4];
    int nx[2][4];
    if (j0 >= 2 && j0 + 1 <= n_blocks) {                      // all three inside this call's buffer (wave-uniform): twelve
        const short *src = pcm + (j0 - 2) * 256 + lane;       // loads in flight together; guarded, each waits for itself
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
            for (int t = 0; t < 4; t++) xk[b][t] = (float)src[256 * b + 64 * t];
    } else {
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
            for (int t = 0; t < 4; t++) xk[b][t] = dn512_sample(pcm, n_samples, st_in, (j0 - 2 + b) * 256 + lane + 64 * t);
    }
    const int row_off = sh.ver_row_off ? *sh.ver_row_off : 0;
    float na[5], nb[5], tail[4];
    const float *row_a = nullptr, *row_b = nullptr;
    const long first_emit = sh.emit_from;
    bool halo = true;                                         // frame j0 - 1 only rebuilds the overlap tail
    unsigned prio_step = blockIdx.x >> 10;                    // step_priority: one step per frame pair
    for (long ja = j0 - 1; ja < j1; ja += 2) {
        step_priority(prio_step);
        const long jb = ja + 1;
        if (ja + 2 < j1) {                                    // the next pair's two new blocks, needed one iteration from now
            if (ja + 2 >= 0 && ja + 4 <= n_blocks) {            // both inside this call's buffer (wave-uniform)
                const short *src = pcm + (ja + 2) * 256 + lane;
#pragma unroll
                for (int t = 0; t < 4; t++) { nx[0][t] = src[64 * t]; nx[1][t] = src[256 + 64 * t]; }
            } else {
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int t = 0; t < 4; t++) nx[b][t] = (int)dn512_sample(pcm, n_samples, st_in, (ja + 2 + b) * 256 + lane + 64 * t);
            }
        }
        {
            const float *ra = noise_row_at(noise_rows, ver_base, snap_mask, ja >= 0 ? ja : 0, sh.ver_block_off, row_off);
            const float *rb = noise_row_at(noise_rows, ver_base, snap_mask, jb < n_blocks ? jb : n_blocks - 1, sh.ver_block_off, row_off);
            if (ra != row_a) { row_a = ra; load_noise512_regs<MODE>(na, ra, lane); }     // wave-uniform: a new estimate was latched
            if (rb != row_b) { row_b = rb; load_noise512_regs<MODE>(nb, rb, lane); }
        }
        float2 v[8], y[8];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            v[r] = make_float2(xk[0][r] * win[r], xk[1][r] * win[r]);
            v[r + 4] = make_float2(xk[1][r] * win[r + 4], xk[2][r] * win[r + 4]);
        }
        float e_pair = 0.0f;                                      // wave-uniform: the two frames share the transform's rounding
        e_pair = wave_sum_f32(sumsq(v));
        wave_fft512<false>(v, lds, lane, tw);
        float2 zr[5], ya[5], yb[5], ret[4];
        wave_lds_fence();
        pair_fetch_lds(v, lds, lane, zr);
        float ea = 0.0f, eb = 0.0f;
#pragma unroll
        for (int d = 0; d < 5; d++) {
            // bin k stands for its mirror 512 - k too where that has no owner: k = 1..192
            const float w = d < 3 ? ((d == 0 && lane == 0) ? 1.0f : 2.0f) : ((d == 3 && lane == 0) ? 2.0f : 1.0f);
            const float rthr = real_bin_thr(e_pair, lane == 0);   // d == 0 or 4, lane 0: the bins 0 and 256
            ya[d] = apply_gain_scaled<MODE, 9>(cadd_conj(v[d], zr[d]), na[d], ea, w, d == 0 || d == 4, rthr);        // frame a, bin lane + 64 d
            yb[d] = apply_gain_scaled<MODE, 9>(csub_conj_mj(v[d], zr[d]), nb[d], eb, w, d == 0 || d == 4, rthr);     // frame b
        }
        float err_a = 0.0f, err_b = 0.0f;                         // wave-uniform; the gain's 2^-18 undone
        err_a = wave_sum_f32(ea) * 262144.0f;
        err_b = wave_sum_f32(eb) * 262144.0f;
        // A frame with a non-finite bin (Wiener's 0/0 on an all-zero frame before any estimate, WF:204) has an all-NaN
        // inverse transform in the reference.  Here it must not poison the frame it shares the transform with: its
        // spectrum goes in as zero and its samples come out as NaN.
        bool bad_a = false, bad_b = false;
        if (MODE == 1) {
            float ta = 0.f, tb = 0.f;                                 // NaN iff some bin is NaN or inf
#pragma unroll
            for (int d = 0; d < 5; d++) { ta += (ya[d].x + ya[d].y) * 0.f; tb += (yb[d].x + yb[d].y) * 0.f; }
            bad_a = __ballot(ta != ta) != 0ull;
            bad_b = __ballot(tb != tb) != 0ull;
        }
#pragma unroll
        for (int d = 0; d < 5; d++) {
            const float2 ak = bad_a ? make_float2(0.f, 0.f) : ya[d], bk = bad_b ? make_float2(0.f, 0.f) : yb[d];
            y[d] = cadd_pj(ak, bk);                                   // Z'[k] = Ya[k] + j Yb[k]
            if (d < 4) ret[d] = cconj_sub_j(ak, bk);                  // Z'[512 - k] = conj(Ya[k]) + j conj(Yb[k])
        }
        pair_return_lds(ret, lds, lane, y);
        wave_fft512<true>(y, lds, lane, tw);
        wave_lds_fence();
        if (MODE == 1) {
#pragma unroll
            for (int d = 0; d < 8; d++) y[d] = make_float2(bad_a ? __builtin_nanf("") : y[d].x, bad_b ? __builtin_nanf("") : y[d].y);
        }
        // the very first call of a stream only stashes its block (SS:211-216): no transform, empty overlap
        const bool a_void = calls_before + ja <= 0, b_void = calls_before + jb <= 0;
        {
            // frames FP32 cannot hold (phase_unsafe; the halo frame is its own wave's): again, in FP64.  Wiener too at
            // this frame size: its gain has no amplifier, but a quiet frame still takes a loud partner's rounding.
            float sa = 0.0f, sb = 0.0f;
#pragma unroll
            for (int d = 0; d < 8; d++) { sa += y[d].x * y[d].x; sb += y[d].y * y[d].y; }
            if (!halo && !a_void && ja + 1 >= sh.emit_from && phase_unsafe<512>(e_pair, err_a, sa)) phase_redo(redo, ja, lane);
            if (jb < n_blocks && !b_void && jb + 1 >= sh.emit_from && phase_unsafe<512>(e_pair, err_b, sb)) phase_redo(redo, jb, lane);
        }
        float oa[4], ob[4], tail_b[4];
        if (halo) {
            if (j0 == 0) {
#pragma unroll
                for (int d = 0; d < 4; d++) tail[d] = st_in->tail[lane + 64 * d];       // rgsdOveraped carried over
            } else {
#pragma unroll
                for (int d = 0; d < 4; d++) tail[d] = a_void ? 0.f : y[d + 4].x;
            }
        } else {
#pragma unroll
            for (int d = 0; d < 4; d++) {
                oa[d] = tail[d] + (a_void ? 0.f : y[d].x);                              // SS:248 overlap-add
                tail[d] = a_void ? 0.f : y[d + 4].x;                                    // SS:255-256
            }
        }
#pragma unroll
        for (int d = 0; d < 4; d++) {
            ob[d] = tail[d] + (b_void ? 0.f : y[d].y);
            tail_b[d] = b_void ? 0.f : y[d + 4].y;
        }
        if (ja + 2 < j1) {                                        // the next pair's samples are taken before this pair's stores
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int t = 0; t < 4; t++) asm volatile("" : "+v"(nx[b][t]));
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const long j = half ? jb : ja;
            if ((half == 0 && halo) || j >= n_blocks) continue;
            const float *o = half ? ob : oa;
            if (j >= first_emit && j < sh.emit_to) {
                const long oi = j - first_emit;
#pragma unroll
                for (int d = 0; d < 4; d++) out[oi * 256 + lane + 64 * d] = (short)cast_i16_bits(o[d]);
                if (precast) {
#pragma unroll
                    for (int d = 0; d < 4; d++) precast[oi * 256 + lane + 64 * d] = o[d];
                }
            }
            if (j == n_blocks - 1) {                                                    // SS:257 and the overlap carried out
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    st_out->prev[lane + 64 * d] = pcm[j * 256 + lane + 64 * d];
                    st_out->tail[lane + 64 * d] = half ? tail_b[d] : tail[d];
                }
            }
        }
#pragma unroll
        for (int d = 0; d < 4; d++) {
            tail[d] = tail_b[d];
            xk[0][d] = xk[2][d];
            xk[1][d] = (float)nx[0][d];
            xk[2][d] = (float)nx[1][d];
        }
        halo = false;
    }
}

static int launch_denoise512(hipStream_t s, int mode, int n_cu, const short *pcm, long n_blocks, long calls_before,
                             const DenoiseState *st_in, DenoiseState *st_out, const int *ver_base,
                             const unsigned long long *snap_mask, const float *noise_rows, const float2 *table,
                             const float *win512, short *out, float *precast, const DenoiseShard &sh, int *redo)
{
    // one round of resident waves (4 per SIMD); an odd number of blocks per wave, 7 at least
    const long slots = (long)(n_cu > 0 ? n_cu : 256) * 4 * JDSP_DENOISE512_WAVES(mode);
    long run = (n_blocks + slots - 1) / slots;
    if (run < 7) run = 7;
    run |= 1;
    const long waves = (n_blocks + run - 1) / run;
    const long grid = (waves + 7) / 8 * 8;
    if (mode == 0)
        hipLaunchKernelGGL(denoise512_run_kernel<0>, dim3((unsigned)grid), dim3(64), 0, s, pcm, n_blocks, calls_before, st_in,
                           st_out, ver_base, snap_mask, noise_rows, table, win512, out, precast, sh, (int)run, redo);
    else
        hipLaunchKernelGGL(denoise512_run_kernel<1>, dim3((unsigned)grid), dim3(64), 0, s, pcm, n_blocks, calls_before, st_in,
                           st_out, ver_base, snap_mask, noise_rows, table, win512, out, precast, sh, (int)run, redo);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------
// The frames on the list {count, frames...} again, in FP64 from the samples on, as the reference computes them
// (SS:226-256 / WF:181-228): Hamming with the reference's PI, an n_fft-point complex transform of the real frame, the
// gain on every bin with its own noise value (Y = (|X| - N) e^{j phase(X)} written as X (1 - N / |X|); Wiener
// X (1 - min(1, N^2 / |X|^2)), 0 / 0 staying NaN), the inverse transform, its real part, 1 / n_fft.  The transform is a
// radix-2 in LDS: bit-reversed load, log2(n_fft) passes of n_fft / 2 butterflies over the workgroup's 256 threads,
// twiddles from a table of exact cosines and sines -- 20 passes per frame, not n_fft^2 multiply-adds.  A listed frame f
// adds into the blocks f and f + 1, so the workgroup computes the frames f - 1, f and f + 1 and writes both blocks
// again, and the overlap carried out of the call if f is its last frame.  Workgroups of neighbouring listed frames write
// the block between them twice, with the same values.
template <int NFFT>
__device__ __forceinline__ double redo_sample(const short *__restrict__ pcm, long n_samples,
                                              const DenoiseState *__restrict__ st_in, long s)
{
    constexpr int B = NFFT / 2;
    if (s >= 0) return s < n_samples ? (double)pcm[s] : 0.0;
    if (s >= -B) return (double)st_in->prev[B + s];             // (every launcher passes a state)
    return 0.0;
}

// buf (bit-reversed order in, natural order out) <- its transform; every thread of the workgroup calls it
template <int NFFT, bool INV>
__device__ __forceinline__ void redo_fft_lds(double2 *buf, const double2 *tw, int tid)
{
#pragma unroll 1
    for (int half = 1; half < NFFT; half <<= 1) {
        const int step = NFFT / (2 * half);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NFFT / 512; r++) {
            const int b = tid + 256 * r, pos = b & (half - 1), i0 = ((b - pos) << 1) + pos, i1 = i0 + half;
            double2 w = tw[pos * step];
            if (INV) w.y = -w.y;
            const double2 u = buf[i0], v = buf[i1];
            const double2 t = make_double2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
            buf[i0] = make_double2(u.x + t.x, u.y + t.y);
            buf[i1] = make_double2(u.x - t.x, u.y - t.y);
        }
    }
    __syncthreads();
}

// buf holds a frame's windowed samples in bit-reversed order: its transform, the gain against `row`, the inverse
// transform, and its real part / n_fft (SS:248) into y[0 .. NFFT); every thread of the workgroup calls it
template <int NFFT>
__device__ __forceinline__ void redo_gain_frame(double2 *buf, const double2 *tw, const float *__restrict__ row, int mode,
                                                int tid, double *y)
{
    constexpr int R = NFFT / 256, LOG = NFFT == 1024 ? 10 : 9;
    redo_fft_lds<NFFT, false>(buf, tw, tid);
    double2 Y[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int k = tid + 256 * r;
        const double2 X = buf[k];
        const double nk = (double)row[k];
        if (mode == 1) {                                     // WF:196-213; 0 / 0 stays NaN as in the reference
            double rk = nk * nk / (X.x * X.x + X.y * X.y);
            if (rk >= 1.0) rk = 1.0;                         // (a NaN stays one: fmin would drop it)
            Y[r] = make_double2(X.x * (1.0 - rk), X.y * (1.0 - rk));
        } else {
            const double mag = sqrt(X.x * X.x + X.y * X.y);
            if (mag == 0.0) {
                Y[r] = make_double2(-nk, 0.0);               // phase 0 (SS:233-242)
            } else {
                const double g = 1.0 - nk / mag;
                Y[r] = make_double2(X.x * g, X.y * g);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; r++) buf[__brev((unsigned)(tid + 256 * r)) >> (32 - LOG)] = Y[r];
    redo_fft_lds<NFFT, true>(buf, tw, tid);
#pragma unroll
    for (int r = 0; r < R; r++) y[tid + 256 * r] = buf[tid + 256 * r].x * (1.0 / NFFT);     // SS:248
}

// What differs between a stream and a batch in the pass below.  seek(f): at the listed frame f.  Then for q < 3, the
// frames f - 1 + q: have(q), whether the frame exists and adds anything; sample(q, i), its sample i; row(q), its noise
// row.  And for q < 2, the blocks f + q: writes(q), whether this launch may write the block; carried(q) / carry(i), an
// overlap that comes from outside the call instead of from frame f - 1 + q; store(q, i, o); finish(), after both.
//
// A stream: frames outside the call add nothing here, block 0 takes the overlap carried in instead; the very first
// call of a stream only stashes its block (SS:211-216).  Samples before the call come from the state's previous block.
template <int NFFT> struct RedoStream {
    static constexpr int B = NFFT / 2;
    const short *pcm;
    long n_blocks, calls_before;
    const DenoiseState *st_in;
    DenoiseState *st_out;
    const int *ver_base;
    const unsigned long long *snap_mask;
    const float *noise_rows;
    short *out;
    float *precast;
    const DenoiseShard &sh;
    long f;
    __device__ __forceinline__ void seek(long f_) { f = f_; }
    __device__ __forceinline__ bool have(int q) const
    {
        const long j = f - 1 + q;
        return j >= 0 && j < n_blocks && calls_before + j > 0;
    }
    __device__ __forceinline__ double sample(int q, int i) const
    {
        return redo_sample<NFFT>(pcm, n_blocks * B, st_in, (f - 2 + q) * B + i);
    }
    __device__ __forceinline__ const float *row(int q) const { return noise_row(noise_rows, ver_base, snap_mask, f - 1 + q, sh); }
    __device__ __forceinline__ bool writes(int q) const { return f + q < n_blocks && f + q >= sh.emit_from && f + q < sh.emit_to; }
    __device__ __forceinline__ bool carried(int q) const { return f + q == 0; }
    __device__ __forceinline__ double carry(int i) const { return (double)st_in->tail[i]; }     // rgsdOveraped carried over
    __device__ __forceinline__ void store(int q, int i, float o) const
    {
        const long at = (f + q - sh.emit_from) * B + i;
        out[at] = (short)cast_i16_bits(o);
        if (precast) precast[at] = o;
    }
    __device__ __forceinline__ void finish(const double *rest, int tid) const
    {
        if (f != n_blocks - 1) return;
#pragma unroll
        for (int r = 0; r < NFFT / 512; r++) st_out->tail[tid + 256 * r] = (float)rest[tid + 256 * r];   // SS:255-256
    }
};

// A batch: a listed global frame f of utterance u (local b) adds into the outputs of the local blocks b and b + 1, so
// the frames b - 1, b, b + 1 that exist are the local blocks 1 .. B_u - 1 (block 0 only stashes its samples): never the
// previous utterance's last frame, never the next one's first.  Both outputs are written where the run kernel writes
// them: at the time of the local blocks b - 1 and b, if those are 1 .. B_u - 2.
struct RedoBatch {
    const short *pcm;
    const long long *sample_first, *block_first;
    long n_utts;
    const int *row_idx;
    const float *noise_rows;
    short *out;               // may be NULL
    float *precast;           // may be NULL
    long ub, n_own, first, b;
    __device__ __forceinline__ void seek(long f)
    {
        const long u = ragged_find_utt(block_first, n_utts, f);
        ub = uniform_i64(block_first + u);
        n_own = uniform_i64(block_first + u + 1) - ub;
        first = uniform_i64(sample_first + u);
        b = f - ub;
    }
    __device__ __forceinline__ bool have(int q) const { return b - 1 + q >= 1 && b - 1 + q < n_own; }
    __device__ __forceinline__ double sample(int q, int i) const { return (double)pcm[first + (b - 2 + q) * 512 + i]; }
    __device__ __forceinline__ const float *row(int q) const { return noise_rows + (size_t)row_idx[ub + b - 1 + q] * 1024; }
    __device__ __forceinline__ bool writes(int q) const { return b + q >= 2 && b + q < n_own; }
    __device__ __forceinline__ bool carried(int) const { return false; }
    __device__ __forceinline__ double carry(int) const { return 0.0; }
    __device__ __forceinline__ void store(int q, int i, float o) const
    {
        const long at = first + (b + q - 1) * 512 + i;
        if (out) out[at] = (short)cast_i16_bits(o);
        if (precast) precast[at] = o;
    }
    __device__ __forceinline__ void finish(const double *, int) const {}
};

// One workgroup per listed frame (grid-stride over the list)
template <int NFFT, class Src>
__device__ __forceinline__ void redo_f64_run(const int *__restrict__ redo, int mode, Src src)
{
    constexpr int B = NFFT / 2, R = NFFT / 256, LOG = NFFT == 1024 ? 10 : 9;
    __shared__ double2 tw[B];
    __shared__ double2 buf[NFFT];
    __shared__ double yy[3][NFFT];
    const int tid = threadIdx.x;
    const long n_redo = redo[0];
    if ((long)blockIdx.x >= n_redo) return;                     // (the whole workgroup)
    double win[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int i = tid + 256 * r;
        if (i < B) {
            double sn, cs;
            sincospi(2.0 * (double)i / (double)NFFT, &sn, &cs);
            tw[i] = make_double2(cs, -sn);
        }
        win[r] = 0.54 - 0.46 * cos(2 * 3.141592 * i / (NFFT - 1));    // SS:226
    }
    for (long it = blockIdx.x; it < n_redo; it += gridDim.x) {
        src.seek(redo[1 + it]);
        for (int q = 0; q < 3; q++) {
            const bool have = src.have(q);                       // (uniform)
            __syncthreads();
            if (!have) {
#pragma unroll
                for (int r = 0; r < R; r++) yy[q][tid + 256 * r] = 0.0;
                continue;
            }
            const float *row = src.row(q);
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int i = tid + 256 * r;
                buf[__brev((unsigned)i) >> (32 - LOG)] = make_double2(src.sample(q, i) * win[r], 0.0);
            }
            redo_gain_frame<NFFT>(buf, tw, row, mode, tid, yy[q]);
        }
        __syncthreads();
        for (int q = 0; q < 2; q++) {
            if (!src.writes(q)) continue;
#pragma unroll
            for (int r = 0; r < R / 2; r++) {
                const int i = tid + 256 * r;
                const double t = src.carried(q) ? src.carry(i) : yy[q][B + i];
                src.store(q, i, (float)(t + yy[q + 1][i]));      // SS:248 overlap-add
            }
        }
        src.finish(yy[1] + B, tid);
    }
}

template <int NFFT>
__global__ __launch_bounds__(256) void denoise_redo_f64_kernel(
    const short *__restrict__ pcm, long n_blocks, long calls_before, const DenoiseState *__restrict__ st_in,
    DenoiseState *st_out, const int *__restrict__ ver_base, const unsigned long long *__restrict__ snap_mask,
    const float *__restrict__ noise_rows, short *__restrict__ out, float *__restrict__ precast, DenoiseShard sh,
    const int *__restrict__ redo, int mode)
{
    redo_f64_run<NFFT>(redo, mode, RedoStream<NFFT>{pcm, n_blocks, calls_before, st_in, st_out, ver_base, snap_mask,
                                                    noise_rows, out, precast, sh, 0});
}

constexpr int kRedoGrid = 1024;
static void launch_denoise_redo(hipStream_t s, int n_fft, const short *pcm, long n_blocks, long calls_before,
                                const DenoiseState *st_in, DenoiseState *st_out, const int *ver_base,
                                const unsigned long long *snap_mask, const float *noise_rows, short *out, float *precast,
                                const DenoiseShard &sh, const int *redo, int mode)
{
    const dim3 grid((unsigned)(n_blocks < kRedoGrid ? n_blocks : kRedoGrid));
    if (n_fft == 512)
        hipLaunchKernelGGL(denoise_redo_f64_kernel<512>, grid, dim3(256), 0, s, pcm, n_blocks, calls_before, st_in, st_out,
                           ver_base, snap_mask, noise_rows, out, precast, sh, redo, mode);
    else
        hipLaunchKernelGGL(denoise_redo_f64_kernel<1024>, grid, dim3(256), 0, s, pcm, n_blocks, calls_before, st_in, st_out,
                           ver_base, snap_mask, noise_rows, out, precast, sh, redo, mode);
}

// =======================================================================================
// Ragged calls over one concatenated block axis (ragged_batch.h), in two forms:
//   a batch of ragged utterances, each a fresh stream of main() (jdsp_denoise_batch*, include/jdsp.h);
//   the chunks of LIVE streams (jdsp_denoise_streams*; DenoiseLive, jdsp_internal.h): the batch's layout with chunks for
//   utterances, but a chunk continues its stream instead of starting one.  Bit for bit the stream's emitted blocks are
//   what the batch writes for ONE utterance of all its blocks, however they are cut.
// Both forms are the same code below (a "chunk" is an utterance of the batch or a chunk of a live call); a carrier per
// form, in the manner of RedoBatch / RedoLive, spells out in one-line members what a fresh chunk and a continued one
// differ in.  After the VAD over the block axis (vad_flags_batch_kernel above):
//   noise_chain         one wave per CHUNK walks its flags in order: main()'s run-length counter (SS:98-109), the
//                       running average A <- h (A + |X|) of its events in registers (SS:165-187), a latch at run length
//                       10 (SS:189-193) into the call's row table, and per block the index of the row in force.
//                       noise_batch_kernel (NoiseBatch): all three start from zero.  noise_live_kernel (NoiseLive): from
//                       the stream's carried run length, average and estimate.
//   denoise_chunk_walk  denoise_run_kernel's frame over the block axis: the waves are planned over all blocks, a wave
//                       finds its chunk by ragged_batch.h's search and walks on.  denoise_batch_kernel (WalkBatch, empty):
//                       a chunk starts a stream.  denoise_live_kernel (WalkLive): where the halo frame would lie in front
//                       of the chunk, the carried tail (that frame's y[d + 4]) and the carried previous block stand in.
//   redo_f64_run        the listed frames again in FP64, inside their chunk's bounds (RedoBatch), or from the stream's
//                       last two blocks and carried estimate where the frame lies in front of the chunk (RedoLive)
//   denoise_live_commit_kernel   live only: flips the parities, counts the blocks, reports E_c
// A chunk holds a few hundred events where a handle's own stream holds tens of thousands, so the chain is not cut into
// affine maps here: cutting it at positions of the call would make a chunk's bits depend on where it stands.
// The batch's row table: row 0 is zeros (nothing latched yet), shared by all utterances; an utterance of B blocks latches
// at most floor(B / 10) times and sum floor(B_u / 10) <= floor(sum B_u / 10), so utterance u's rows start at
// 1 + block_first[u] / 10 and no prefix sum over the utterances is needed.  The live table: the two estimate copies of
// every stream, then chunk c's rows from 2 n_streams + c + block_first[c] / 11 (a chunk of B blocks latches
// 1 + (B - 1) / 11 times at most).
__device__ __forceinline__ void load_pairs(const short *__restrict__ block, int lane, unsigned int (&q)[4])
{
    const unsigned int *src = reinterpret_cast<const unsigned int *>(block) + lane;
#pragma unroll
    for (int r = 0; r < 4; r++) q[r] = src[64 * r];
}

struct LiveChunk {
    long s, N;                                                   // the stream, the blocks it had seen
    int p;                                                       // the copy of prev / tail / listed it starts from
};
__device__ __forceinline__ LiveChunk live_chunk(const long long *__restrict__ stream_id, const int *__restrict__ parity,
                                                const long long *__restrict__ seen, long c)
{
    LiveChunk k;
    k.s = uniform_i64(stream_id + c);
    k.p = __builtin_amdgcn_readfirstlane(parity[k.s]) & 1;
    k.N = uniform_i64(seen + k.s);
    return k;
}

// The running average of a chunk's wave in registers, in noise_accum_kernel's pair-owned layout: the bins m, m + 512 of
// m = lane + 64 d; a row is stored as the ten own values plus the mirrors of m = 1..192.  The event's arithmetic and
// the row's store are that kernel's, which keeps its own text: with all three noise kernels on this struct the
// compiler orders eight zero moves in denoise_run_kernel<0>'s prologue differently, and no kernel outside the chain
// and the walk was to change (profiles/r21_denoise_one_walk.txt).
struct NoiseAvg {
    static constexpr int ND = 5;
    float lo[ND], hi[ND];
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int d = 0; d < ND; d++) lo[d] = hi[d] = 0.0f;
    }
    // one EstimateNoiseSpectrum event, A <- h (A + |FFT(window * [prev, cur])|): the blocks as load_block_pairs gives them
    __device__ __forceinline__ void accumulate(const unsigned int (&prev)[4], const unsigned int (&cur)[4],
                                               const FrameTables &t, const PairTwiddles &pw, float2 *lds, int lane, float h)
    {
        float2 v[8], zr[ND];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float2 s0 = unpack_i16x2(prev[r]), s1 = unpack_i16x2(cur[r]);
            v[r] = make_float2(s0.x * t.win[r].x, s0.y * t.win[r].y);
            v[r + 4] = make_float2(s1.x * t.win[r + 4].x, s1.y * t.win[r + 4].y);
        }
        wave_fft512<false>(v, lds, lane, t.tw);
        wave_lds_fence();
        pair_fetch_lds(v, lds, lane, zr);
#pragma unroll
        for (int d = 0; d < ND; d++) {
            const float2 ev = cadd_conj(v[d], zr[d]), od = csub_conj_mj(v[d], zr[d]);
            const float2 tw = cmul(pw.w[d], od);
            const float2 a = cadd(ev, tw), b = csub(ev, tw);
            // hardware square root, 1 ulp (see noise_accum_kernel)
            lo[d] = (lo[d] + __builtin_amdgcn_sqrtf(a.x * a.x + a.y * a.y)) * h;
            hi[d] = (hi[d] + __builtin_amdgcn_sqrtf(b.x * b.x + b.y * b.y)) * h;
        }
    }
    __device__ __forceinline__ void store_row(float *row, int lane) const
    {
#pragma unroll
        for (int d = 0; d < ND; d++) { row[lane + 64 * d] = lo[d]; row[lane + 64 * d + 512] = hi[d]; }
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int m = lane + 64 * d;
            if (m >= 1 && m <= 192) { row[1024 - m] = lo[d]; row[512 - m] = hi[d]; }
        }
    }
};

// What a fresh chunk and a continued one differ in, in the chain below.  start(): the average and the run length the chunk
// begins with; row_in_force(): the row before its first latch; first_row(ub): the first row of the call's table it may
// latch into; before(): the block in front of its first block; latch(): the second destination of a latched average;
// finish(): after the last block.
struct NoiseBatch {
    float *noise_last;        // [n_utts][1024] or NULL: the estimate each utterance ends with
    long u;
    __device__ __forceinline__ int start(NoiseAvg &a, int) const { a.zero(); return 0; }
    __device__ __forceinline__ int row_in_force() const { return 0; }
    __device__ __forceinline__ int first_row(long ub) const { return 1 + (int)(ub / 10); }
    // never read: the run length starts at 0
    __device__ __forceinline__ const short *before(const short *own) const { return own - 512; }
    __device__ __forceinline__ void latch(const NoiseAvg &a, int lane) const
    {
        if (noise_last) a.store_row(noise_last + (size_t)u * 1024, lane);
    }
    __device__ __forceinline__ void finish(const NoiseAvg &, int, bool latched, int lane) const
    {
        if (!noise_last || latched) return;                      // nothing latched: rgdEstimatedNS is still zero (SS:70)
#pragma unroll
        for (int r = 0; r < 16; r++) noise_last[(size_t)u * 1024 + lane + 64 * r] = 0.0f;
    }
};

struct NoiseLive {
    DenoiseLive lv;
    long c;                   // the chunk
    LiveChunk k;
    int ep;                   // the estimate copy in force
    __device__ __forceinline__ float *avg() const { return lv.avg + (size_t)k.s * kLiveAvgFloats; }
    __device__ __forceinline__ int start(NoiseAvg &a, int lane) const
    {
#pragma unroll
        for (int d = 0; d < NoiseAvg::ND; d++) { a.lo[d] = avg()[lane + 64 * d]; a.hi[d] = avg()[320 + lane + 64 * d]; }
        return __builtin_amdgcn_readfirstlane(lv.run_len[k.s]);
    }
    __device__ __forceinline__ int row_in_force() const { return (int)(ep * lv.n_streams + k.s); }
    __device__ __forceinline__ int first_row(long ub) const { return (int)(2 * lv.n_streams + c + ub / 11); }
    __device__ __forceinline__ const short *before(const short *) const                      // the stream's last block
    {
        return lv.prev + ((size_t)k.p * lv.n_streams + k.s) * 1024 + 512;
    }
    __device__ __forceinline__ void latch(const NoiseAvg &a, int lane) const                 // the stream's next estimate
    {
        a.store_row(lv.rows + ((size_t)(ep ^ 1) * lv.n_streams + k.s) * 1024, lane);
    }
    __device__ __forceinline__ void finish(const NoiseAvg &a, int run_len, bool latched, int lane) const
    {
#pragma unroll
        for (int d = 0; d < NoiseAvg::ND; d++) { avg()[lane + 64 * d] = a.lo[d]; avg()[320 + lane + 64 * d] = a.hi[d]; }
        if (lane == 0) {
            lv.run_len[k.s] = run_len;
            lv.latched[c] = latched;
        }
    }
};

// own: the chunk's samples; ub, n_own: its first block on the block axis, its blocks; rows: the call's row table
template <class Carry>
__device__ __forceinline__ void noise_chain(const short *own, long ub, long n_own, const unsigned char *__restrict__ flags,
                                            const float2 *__restrict__ table, float *rows, int *__restrict__ row_idx,
                                            Carry cy)
{
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    const int lane = threadIdx.x;
    FrameTables t;
    load_frame_tables(t, table, lane);
    PairTwiddles pw;
    load_pair_twiddles(pw, table, lane);
    NoiseAvg a;
    int run_len = cy.start(a, lane);                             // iNumOfIteration (SS:72)
    int row = cy.row_in_force(), next_row = cy.first_row(ub);
    bool latched = false;
    for (long c = 0; c < n_own; c += 64) {
        const int n = n_own - c < 64 ? (int)(n_own - c) : 64;
        const unsigned long long voice = __ballot(lane < n && flags[ub + c + lane] != 0);
        int mine = 0;                                            // the row of block c + lane
        for (int i = 0; i < n; i++) {
            if ((voice >> i) & 1ull) {
                run_len = 0;                                     // SS:108
            } else {
                run_len = run_len < 11 ? run_len + 1 : 11;       // saturated: only >= 2, >= 3 and == 10 are asked of it
                if (run_len >= 2) {                              // SS:103-105: EstimateNoiseSpectrum
                    const short *cur_block = own + (c + i) * 512;
                    unsigned int prev[4], cur[4];
                    load_pairs(c + i == 0 ? cy.before(own) : cur_block - 512, lane, prev);   // rgssKeepBuffer (SS:165-170)
                    load_pairs(cur_block, lane, cur);
                    a.accumulate(prev, cur, t, pw, lds, lane, run_len >= 3 ? 0.5f : 1.0f);   // SS:182-187
                    if (run_len == 10) {                         // SS:189-193; it applies to this block already
                        row = next_row++;
                        latched = true;
                        a.store_row(rows + (size_t)row * 1024, lane);
                        cy.latch(a, lane);
                    }
                }
            }
            if (lane == i) mine = row;
        }
        if (lane < n) row_idx[ub + c + lane] = mine;
    }
    cy.finish(a, run_len, latched, lane);
}

__global__ __launch_bounds__(64) void noise_batch_kernel(const short *__restrict__ pcm,
                                                         const long long *__restrict__ sample_first,
                                                         const long long *__restrict__ block_first,
                                                         const unsigned char *__restrict__ flags,
                                                         const float2 *__restrict__ table, float *__restrict__ rows,
                                                         int *__restrict__ row_idx, float *__restrict__ noise_last)
{
    const long u = blockIdx.x;
    const long ub = uniform_i64(block_first + u), n_own = uniform_i64(block_first + u + 1) - ub;
    const short *own = pcm + uniform_i64(sample_first + u);
    noise_chain(own, ub, n_own, flags, table, rows, row_idx, NoiseBatch{noise_last, u});
}

__global__ __launch_bounds__(64) void noise_live_kernel(const short *__restrict__ pcm,
                                                        const long long *__restrict__ stream_id,
                                                        const long long *__restrict__ sample_first,
                                                        const long long *__restrict__ block_first,
                                                        const unsigned char *__restrict__ flags,
                                                        const float2 *__restrict__ table, int *__restrict__ row_idx,
                                                        DenoiseLive lv)
{
    const long c = blockIdx.x;
    const long ub = uniform_i64(block_first + c), n_own = uniform_i64(block_first + c + 1) - ub;
    const short *own = pcm + uniform_i64(sample_first + c);     // (with the loads above: nothing it waits for)
    if (n_own <= 0) return;                                      // the stream is not touched (the commit skips it too)
    const LiveChunk k = live_chunk(stream_id, lv.parity, lv.seen, c);
    const int ep = __builtin_amdgcn_readfirstlane(lv.est_parity[k.s]) & 1;
    noise_chain(own, ub, n_own, flags, table, lv.rows, row_idx, NoiseLive{lv, c, k, ep});
}

// What the walk below asks of a chunk that continues a stream; for a chunk that starts one (WalkBatch) every answer is
// a constant and the struct is empty, so denoise_batch_kernel carries no state operand and no dead branch.
//   seek(c)        the wave starts in chunk c
//   seek_next(c)   the next block is the first of chunk c; step(): the walk goes on to the next block
//   seen()         N, the blocks the chunk's stream had seen: block j of a chunk at ub has stream index N + (j - ub)
//   enter()        at the chunk's first block: the stream's last block into raw[0..3], its overlap into tail; returns
//                  whether the stream's last frame went to the FP64 pass
//   keep_blocks()  at the chunk's last block, in the wave that owns it, BEFORE the frame: the stream's last two blocks
//                  (the first of them is not kept across the frame: stored after it, it costs scratch)
//   keep_tail()    the same place AFTER the stores: the overlap and the word the next call starts from
//   lists(B)       whether a frame FP32 cannot hold, in a chunk of B blocks, goes to the FP64 pass
//   emit_at()      where the output of block j goes
struct WalkBatch {
    __device__ __forceinline__ void seek(long) {}
    __device__ __forceinline__ void seek_next(long) {}
    __device__ __forceinline__ void step() {}
    static __device__ __forceinline__ constexpr long seen() { return 0; }
    __device__ __forceinline__ int enter(unsigned int (&)[8], float2 (&)[4], int) const { return 0; }
    __device__ __forceinline__ void keep_blocks(const unsigned int (&)[8], int) const {}
    __device__ __forceinline__ void keep_tail(const float2 (&)[4], int, int) const {}
    // fewer than three blocks: nothing of the utterance is emitted
    __device__ __forceinline__ bool lists(long n_own) const { return n_own >= 3; }
    // time-aligned: the output of local block b stands at the time of local block b - 1
    __device__ __forceinline__ long emit_at(long base, long j) const { return base + (j - 1) * 512; }
};

// The state's loads and stores form their lane offsets per chunk from an opaque copy of the lane: formed from `lane`
// itself they are loop invariants, hoisted out of the run and kept in registers the frame needs.
struct WalkLive {
    const long long *stream_id;
    const int *parity;
    const long long *seen_;
    DenoiseLive lv;
    LiveChunk k, kn;          // of the block, of the next block
    static __device__ __forceinline__ int opaque(int lane) { asm volatile("" : "+v"(lane)); return lane; }
    __device__ __forceinline__ size_t copy(int p) const { return (size_t)p * lv.n_streams + k.s; }
    __device__ __forceinline__ void seek(long c) { k = kn = live_chunk(stream_id, parity, seen_, c); }
    __device__ __forceinline__ void seek_next(long c) { kn = live_chunk(stream_id, parity, seen_, c); }
    __device__ __forceinline__ void step() { k = kn; }
    __device__ __forceinline__ long seen() const { return k.N; }
    __device__ __forceinline__ int enter(unsigned int (&raw)[8], float2 (&tail)[4], int lane) const   // (zeros when fresh)
    {
        const int sl = opaque(lane);
        unsigned int hp[4];
        load_pairs(lv.prev + copy(k.p) * 1024 + 512, sl, hp);
#pragma unroll
        for (int r = 0; r < 4; r++) raw[r] = hp[r];
        const float2 *tl = reinterpret_cast<const float2 *>(lv.tail + copy(k.p) * 512) + sl;
#pragma unroll
        for (int d = 0; d < 4; d++) tail[d] = tl[64 * d];
        return __builtin_amdgcn_readfirstlane(lv.listed[copy(k.p)]);
    }
    __device__ __forceinline__ void keep_blocks(const unsigned int (&raw)[8], int lane) const
    {
        unsigned int *pv = reinterpret_cast<unsigned int *>(lv.prev + copy(k.p ^ 1) * 1024) + opaque(lane);
#pragma unroll
        for (int r = 0; r < 8; r++) pv[64 * r] = raw[r];
    }
    __device__ __forceinline__ void keep_tail(const float2 (&tail)[4], int listed, int lane) const
    {
        float2 *tl = reinterpret_cast<float2 *>(lv.tail + copy(k.p ^ 1) * 512) + opaque(lane);
#pragma unroll
        for (int d = 0; d < 4; d++) tl[64 * d] = tail[d];
        if (lane == 0) lv.listed[copy(k.p ^ 1)] = listed;
    }
    __device__ __forceinline__ bool lists(long) const { return true; }
    // packed from the span's start: the first two blocks of a stream emit nothing (SS:260-263)
    __device__ __forceinline__ long emit_at(long base, long j) const { return base + (j - (k.N < 2 ? 2 - k.N : 0)) * 512; }
};

// denoise_run_kernel over the concatenated block axis.  Wave w owns the global blocks [w run, (w + 1) run); global
// block j of chunk u (block_first[u] <= j < block_first[u + 1]) has the stream index i = N + (j - block_first[u]) and
// its samples at base + 512 j.  Stream block 0 only stashes its samples (SS:211-216), so the overlap restarts from zero
// by itself where a stream begins; the frame of block i >= 1 is [block i - 1, block i], and with the overlap it gives
// the enhanced samples at the time of block i - 1, emitted when i >= 2 (SS:260-263: the first two calls emit nothing).
// So an utterance's first and last blocks are never written.  The halo frame in front of the wave's first block goes
// through the SAME loop body as every other frame (emission off), never into the chunk before: one inlined copy of
// the arithmetic, so the samples do not depend on where the waves are cut.
template <int MODE, class Carry>
__device__ __forceinline__ void denoise_chunk_walk(const short *__restrict__ pcm, const long long *__restrict__ sample_first,
                                                   const long long *__restrict__ block_first, long n_chunks, long n_blocks,
                                                   const int *__restrict__ row_idx, const float *__restrict__ rows,
                                                   const float2 *__restrict__ table, short *__restrict__ out,
                                                   float *__restrict__ precast, int run, int *__restrict__ redo, Carry cy)
{
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    const int lane = threadIdx.x;
    PhaseStat ps;
    const long per_xcd = (gridDim.x + 7) >> 3;                // XCD-aware run order (speed only)
    const long j0 = ((long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3)) * run;
    if (j0 >= n_blocks) return;
    const long j1 = j0 + run < n_blocks ? j0 + run : n_blocks;
    long u = ragged_find_utt(block_first, n_chunks, j0);
    long ub = uniform_i64(block_first + u), ue = uniform_i64(block_first + u + 1);
    long base = uniform_i64(sample_first + u) - ub * 512;      // global block j of this chunk starts at base + 512 j
    cy.seek(u);
    // stream index 0 or 1: the overlap entering block j0 is empty; the chunk's first block: it is the carried tail;
    // else the frame of block j0 - 1 rebuilds it
    const long js = (j0 > ub && cy.seen() + (j0 - ub) >= 2) ? j0 - 1 : j0;

    FrameTables t;
    load_frame_tables(t, table, lane);
    PairTwiddles sw;
    load_pair_twiddles(sw, table, lane);
    NoisePairRegs nz;
    unsigned int raw[8], nxt[4], tk[4];
    float2 tail[4], y[8];
#pragma unroll
    for (int d = 0; d < 4; d++) tail[d] = make_float2(0.f, 0.f);
    // the block in front of js, clamped into the chunk (unused where it is clamped: stream block 0 has no frame, and at
    // a continued chunk's first block cy.enter() brings it)
    load_pairs(pcm + base + (js > ub ? js - 1 : ub) * 512, lane, nxt);
#pragma unroll
    for (int r = 0; r < 4; r++) raw[r + 4] = nxt[r];
    load_pairs(pcm + base + js * 512, lane, tk);
    int cur_row = -1;
    int next_idx = __builtin_amdgcn_readfirstlane(row_idx[js]);
    unsigned prio_step = blockIdx.x >> 10;                    // step_priority: one step per block
    for (long j = js; j < j1; j++) {
        step_priority(prio_step);
#pragma unroll
        for (int r = 0; r < 4; r++) { raw[r] = raw[r + 4]; raw[r + 4] = tk[r]; }
        const int idx = next_idx;
        const bool last_owned = j + 1 == ue && j >= j0;         // the chunk's last block, in the wave that owns it
        int listed_in = 0, listed = 0;
        if (j == ub) listed_in = cy.enter(raw, tail, lane);
        if (last_owned) cy.keep_blocks(raw, lane);
        // the next block, needed one iteration from now (denoise_run_kernel); after a chunk's last block it is the
        // first block of the next non-empty one
        long un = u, ubn = ub, uen = ue, basen = base;
        if (j + 1 < j1) {
            if (j + 1 == ue) {
                ubn = ue;
                ragged_next_utt(block_first, n_chunks, un, uen);
                basen = uniform_i64(sample_first + un) - ubn * 512;
                cy.seek_next(un);
            }
            next_idx = row_idx[j + 1];
            load_pairs(pcm + basen + (j + 1) * 512, lane, nxt);
        }
        const long i = cy.seen() + (j - ub);                     // the block's index in its stream
        if (i == 0) {
            // the first call of a stream only stashes its block (SS:211-216): no output, empty overlap
#pragma unroll
            for (int d = 0; d < 8; d++) y[d] = make_float2(0.f, 0.f);
        } else {
            if (idx != cur_row) {                                // wave-uniform: another estimate is in force
                cur_row = idx;
                load_noise_pair_regs<MODE>(nz, rows + (size_t)idx * 1024, lane);
            }
            denoise_frame_pairs<MODE>(raw, t, sw, table, lds, lane, nz, y, ps);
            // a frame FP32 cannot hold (phase_unsafe): again, in FP64, if one of its two blocks is emitted
            if (MODE == 0 && j >= j0 && cy.lists(ue - ub) && phase_unsafe<1024>(ps.e, ps.err, sumsq(y))) {
                phase_redo(redo, j, lane);
                listed = 1;
            }
        }
        // the stream's last frame was listed: the FP64 pass owes this block its other half (RedoLive)
        if (MODE == 0 && listed_in && j >= j0) phase_redo(redo, ~j, lane);
        float2 o[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            o[d] = make_float2(tail[d].x + y[d].x, tail[d].y + y[d].y);      // SS:248 overlap-add
            tail[d] = y[d + 4];                                               // SS:255-256
        }
        // taken before this block's stores (denoise_run_kernel)
#pragma unroll
        for (int r = 0; r < 4; r++) { tk[r] = nxt[r]; asm volatile("" : "+v"(tk[r])); }
        next_idx = __builtin_amdgcn_readfirstlane(next_idx);
        __builtin_amdgcn_sched_barrier(0);
        if (j >= j0 && i >= 2) {
            const long at = cy.emit_at(base, j);
            if (out) {
                unsigned int *dst = reinterpret_cast<unsigned int *>(out + at) + lane;
#pragma unroll
                for (int d = 0; d < 4; d++) __builtin_nontemporal_store(cast_i16x2_bits(o[d].x, o[d].y), dst + 64 * d);
            }
            if (precast) {
#pragma unroll
                for (int d = 0; d < 4; d++) *reinterpret_cast<float2 *>(precast + at + 2 * lane + 128 * d) = o[d];
            }
        }
        if (last_owned) cy.keep_tail(tail, listed, lane);
        u = un; ub = ubn; ue = uen; base = basen; cy.step();
    }
}

template <int MODE>
__global__ __launch_bounds__(64, JDSP_DENOISE_RESIDENT) void denoise_batch_kernel(
    const short *__restrict__ pcm, const long long *__restrict__ sample_first, const long long *__restrict__ block_first,
    long n_utts, long n_blocks, const int *__restrict__ row_idx, const float *__restrict__ noise_rows,
    const float2 *__restrict__ table, short *__restrict__ out, float *__restrict__ precast, int run, int *__restrict__ redo)
{
    denoise_chunk_walk<MODE>(pcm, sample_first, block_first, n_utts, n_blocks, row_idx, noise_rows, table, out, precast, run,
                             redo, WalkBatch{});
}

template <int MODE>
__global__ __launch_bounds__(64, JDSP_DENOISE_RESIDENT) void denoise_live_kernel(
    const short *__restrict__ pcm, const long long *__restrict__ stream_id, const long long *__restrict__ sample_first,
    const long long *__restrict__ block_first, const int *__restrict__ parity, const long long *__restrict__ seen,
    long n_chunks, long n_blocks, const int *__restrict__ row_idx, const float2 *__restrict__ table,
    short *__restrict__ out, float *__restrict__ precast, int run, int *__restrict__ redo, DenoiseLive lv)
{
    denoise_chunk_walk<MODE>(pcm, sample_first, block_first, n_chunks, n_blocks, row_idx, lv.rows, table, out, precast, run,
                             redo, WalkLive{stream_id, parity, seen, lv, {}, {}});
}

__global__ __launch_bounds__(256) void denoise_redo_f64_batch_kernel(
    const short *__restrict__ pcm, const long long *__restrict__ sample_first, const long long *__restrict__ block_first,
    long n_utts, const int *__restrict__ row_idx, const float *__restrict__ noise_rows, short *__restrict__ out,
    float *__restrict__ precast, const int *__restrict__ redo, int mode)
{
    redo_f64_run<1024>(redo, mode, RedoBatch{pcm, sample_first, block_first, n_utts, row_idx, noise_rows, out, precast,
                                             0, 0, 0, 0});
}

// A listed entry e >= 0 is the global frame e, as in the batch; e < 0 is the frame in front of the chunk whose first
// block is ~e.  A frame with local index fb >= -1 exists when its stream index N + fb is >= 1; its samples come from
// the chunk or, before it, from the stream's last two blocks; the frame in front of the chunk takes the carried estimate.
struct RedoLive {
    const short *pcm;
    const long long *stream_id, *sample_first, *block_first;
    long n_chunks;
    const int *row_idx;
    DenoiseLive lv;
    short *out;               // may be NULL
    float *precast;           // may be NULL
    long ub, n_own, first, b, N;
    const short *hist;
    const float *est;
    __device__ __forceinline__ void seek(long e)
    {
        const long j = e < 0 ? ~e : e;
        const long c = ragged_find_utt(block_first, n_chunks, j);
        ub = uniform_i64(block_first + c);
        n_own = uniform_i64(block_first + c + 1) - ub;
        first = uniform_i64(sample_first + c);
        b = e < 0 ? -1 : j - ub;
        const LiveChunk k = live_chunk(stream_id, lv.parity, lv.seen, c);
        const int ep = __builtin_amdgcn_readfirstlane(lv.est_parity[k.s]) & 1;
        N = k.N;
        hist = lv.prev + ((size_t)k.p * lv.n_streams + k.s) * 1024;
        est = lv.rows + ((size_t)ep * lv.n_streams + k.s) * 1024;
    }
    __device__ __forceinline__ bool have(int q) const { return b - 1 + q >= -1 && b - 1 + q < n_own && N + b - 1 + q >= 1; }
    __device__ __forceinline__ double sample(int q, int i) const
    {
        const long at = (b - 2 + q) * 512 + i;
        return (double)(at >= 0 ? pcm[first + at] : hist[1024 + at]);
    }
    __device__ __forceinline__ const float *row(int q) const
    {
        return b - 1 + q >= 0 ? lv.rows + (size_t)row_idx[ub + b - 1 + q] * 1024 : est;
    }
    __device__ __forceinline__ bool writes(int q) const { return b + q >= 0 && b + q < n_own && N + b + q >= 2; }
    __device__ __forceinline__ bool carried(int) const { return false; }
    __device__ __forceinline__ double carry(int) const { return 0.0; }
    __device__ __forceinline__ void store(int q, int i, float o) const
    {
        const long at = first + (b + q - (N < 2 ? 2 - N : 0)) * 512 + i;
        if (out) out[at] = (short)cast_i16_bits(o);
        if (precast) precast[at] = o;
    }
    __device__ __forceinline__ void finish(const double *, int) const {}
};

__global__ __launch_bounds__(256) void denoise_redo_f64_live_kernel(
    const short *__restrict__ pcm, const long long *__restrict__ stream_id, const long long *__restrict__ sample_first,
    const long long *__restrict__ block_first, long n_chunks, const int *__restrict__ row_idx, DenoiseLive lv,
    short *__restrict__ out, float *__restrict__ precast, const int *__restrict__ redo, int mode)
{
    redo_f64_run<1024>(redo, mode, RedoLive{pcm, stream_id, sample_first, block_first, n_chunks, row_idx, lv, out, precast,
                                            0, 0, 0, 0, 0, nullptr, nullptr});
}

// one thread per chunk, behind every launch that read the state
__global__ __launch_bounds__(256) void denoise_live_commit_kernel(const long long *__restrict__ stream_id,
                                                                  const long long *__restrict__ block_first, long n_chunks,
                                                                  const int *__restrict__ latched, int *__restrict__ parity,
                                                                  int *__restrict__ est_parity, long long *__restrict__ seen,
                                                                  long long *__restrict__ n_emitted)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_chunks) return;
    const long long n_own = block_first[c + 1] - block_first[c];
    long long e = 0;
    if (n_own > 0) {
        const long long s = stream_id[c], N = seen[s];
        const long long silent = N < 2 ? 2 - N : 0;              // SS:260-263: the first two calls emit nothing
        e = n_own > silent ? n_own - silent : 0;
        parity[s] ^= 1;
        if (latched[c]) est_parity[s] ^= 1;
        seen[s] = N + n_own;
    }
    if (n_emitted) n_emitted[c] = e;
}

// one workgroup per listed stream
__global__ __launch_bounds__(256) void denoise_live_reset_kernel(const long long *__restrict__ stream_id, DenoiseLive lv,
                                                                 int *__restrict__ parity, int *__restrict__ est_parity,
                                                                 long long *__restrict__ seen)
{
    const long long s = stream_id[blockIdx.x];
    const int tid = threadIdx.x;
    for (int e = 0; e < 2; e++) {
        const size_t at = (size_t)e * lv.n_streams + s;
        for (int i = tid; i < 512; i += 256) {
            reinterpret_cast<unsigned int *>(lv.prev + at * 1024)[i] = 0u;
            lv.tail[at * 512 + i] = 0.0f;
        }
        for (int i = tid; i < 1024; i += 256) lv.rows[at * 1024 + i] = 0.0f;
        if (tid == 0) lv.listed[at] = 0;
    }
    for (int i = tid; i < kLiveAvgFloats; i += 256) lv.avg[(size_t)s * kLiveAvgFloats + i] = 0.0f;
    if (tid == 0) {
        lv.run_len[s] = 0;
        parity[s] = 0;
        est_parity[s] = 0;
        seen[s] = 0;
    }
}

// What both launchers below work out behind the noise pass: the blocks per wave (run_opt, or 0 = one round of resident
// waves, resident_run), the run kernel's grid (its waves rounded up to eight) and the FP64 pass's grid over a list
// of n_list entries at most.
struct ChunkLaunch { int run; dim3 grid, redo_grid; };
static ChunkLaunch chunk_launch(int run_opt, int n_cu, long n_blocks, long n_list)
{
    const long run = run_opt > 0 ? run_opt : resident_run(n_cu, n_blocks);
    return {(int)run, dim3((unsigned)(((n_blocks + run - 1) / run + 7) / 8 * 8)),
            dim3((unsigned)(n_list < kRedoGrid ? n_list : kRedoGrid))};
}

// flags / row_idx [n_blocks], rows [n_blocks / 10 + 1][1024] with row 0 zero, redo [n_blocks + 1]: the handle's batch
// workspace.  out and precast may be NULL (both: the run kernel is not launched); noise_last may be NULL.
int launch_denoise_batch(hipStream_t s, int mode, int run_opt, int n_cu, const short *pcm, const long long *sample_first,
                         const long long *block_first, long n_utts, long n_blocks, const double *w_hi,
                         const float2 *table, unsigned char *flags, int *row_idx, float *rows, int *redo, short *out,
                         float *precast, float *noise_last, int vad_only)
{
    if (n_blocks <= 0 || n_utts <= 0) return 0;
    hipLaunchKernelGGL(vad_flags_batch_kernel, dim3((unsigned)((n_blocks + kVadBlocksPerWave - 1) / kVadBlocksPerWave)),
                       dim3(64), 0, s, pcm, sample_first, block_first, n_utts, n_blocks, w_hi, flags);
    if (vad_only) return hipGetLastError() == hipSuccess ? 0 : -1;
    hipLaunchKernelGGL(noise_batch_kernel, dim3((unsigned)n_utts), dim3(64), 0, s, pcm, sample_first, block_first, flags,
                       table, rows, row_idx, noise_last);
    if (!out && !precast) return hipGetLastError() == hipSuccess ? 0 : -1;
    if (mode == 0 && hipMemsetAsync(redo, 0, sizeof(int), s) != hipSuccess) return -1;
    const ChunkLaunch g = chunk_launch(run_opt, n_cu, n_blocks, n_blocks);
    hipLaunchKernelGGL(mode == 0 ? denoise_batch_kernel<0> : denoise_batch_kernel<1>, g.grid, dim3(64), 0, s, pcm,
                       sample_first, block_first, n_utts, n_blocks, row_idx, rows, table, out, precast, g.run, redo);
    if (mode == 0)
        hipLaunchKernelGGL(denoise_redo_f64_batch_kernel, g.redo_grid, dim3(256), 0, s, pcm, sample_first, block_first,
                           n_utts, row_idx, rows, out, precast, redo, mode);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_denoise_live(hipStream_t s, int mode, int run_opt, int n_cu, const short *pcm, const long long *stream_id,
                        const long long *sample_first, const long long *block_first, long n_chunks, long n_blocks,
                        const double *w_hi, const float2 *table, unsigned char *flags, int *row_idx, int *redo,
                        const DenoiseLive &lv, int *parity, int *est_parity, long long *seen, short *out, float *precast,
                        long long *n_emitted)
{
    if (n_blocks <= 0 || n_chunks <= 0) return 0;
    hipLaunchKernelGGL(vad_flags_batch_kernel, dim3((unsigned)((n_blocks + kVadBlocksPerWave - 1) / kVadBlocksPerWave)),
                       dim3(64), 0, s, pcm, sample_first, block_first, n_chunks, n_blocks, w_hi, flags);
    hipLaunchKernelGGL(noise_live_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, pcm, stream_id, sample_first,
                       block_first, flags, table, row_idx, lv);
    if (mode == 0 && hipMemsetAsync(redo, 0, sizeof(int), s) != hipSuccess) return -1;
    const ChunkLaunch g = chunk_launch(run_opt, n_cu, n_blocks, n_blocks + n_chunks);
    hipLaunchKernelGGL(mode == 0 ? denoise_live_kernel<0> : denoise_live_kernel<1>, g.grid, dim3(64), 0, s, pcm, stream_id,
                       sample_first, block_first, lv.parity, lv.seen, n_chunks, n_blocks, row_idx, table, out, precast,
                       g.run, redo, lv);
    if (mode == 0 && (out || precast))
        hipLaunchKernelGGL(denoise_redo_f64_live_kernel, g.redo_grid, dim3(256), 0, s, pcm, stream_id, sample_first,
                           block_first, n_chunks, row_idx, lv, out, precast, redo, mode);
    hipLaunchKernelGGL(denoise_live_commit_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, s, stream_id,
                       block_first, n_chunks, lv.latched, parity, est_parity, seen, n_emitted);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_denoise_live_reset(hipStream_t s,const long long *stream_id, long n_ids, const DenoiseLive &lv, int *parity,
                              int *est_parity, long long *seen)
{
    if (n_ids <= 0) return 0;
    hipLaunchKernelGGL(denoise_live_reset_kernel, dim3((unsigned)n_ids), dim3(256), 0, s, stream_id, lv, parity, est_parity,
                       seen);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- launchers of both frame sizes --------------------------------------------------------------
// 512-point frames: the 512-point accumulate kernel, and the combine / fold / select kernels over bins 0..511 only (rows
// and summaries keep the 1024-float pitch of the 1024-point path; bins 512.. are never read)
int launch_denoise(hipStream_t s, DenoiseGeom g, int mode, int k_opt, int n_cu, const short *pcm, long n_blocks,
                   long calls_before, const DenoiseState *st_in, DenoiseState *st_out, const int *ver_base,
                   const unsigned long long *snap_mask, const float *noise_rows, const float2 *table, short *out,
                   float *precast, int *redo, const DenoiseShard *shard)
{
    // redo: [n_blocks + 1] ints, {count, frames...}: the spectral-subtraction frames FP32 could not hold (phase_unsafe),
    // left there by whichever kernel runs and computed again by denoise_redo_f64_kernel; the count stays for
    // jdsp_denoise_frames_recomputed.  1024-point Wiener lists nothing: no memset, no FP64 launch, the count is not read.
    if (n_blocks <= 0) return 0;
    const bool lists = mode == 0 || g.n_fft == 512;
    if (lists && hipMemsetAsync(redo, 0, sizeof(int), s) != hipSuccess) return -1;
    DenoiseShard sh;
    if (shard) sh = *shard;
    else {
        sh.ver_block_off = 0;
        sh.ver_row_off = nullptr;
        sh.emit_from = calls_before >= 2 ? 0 : 2 - calls_before;
        sh.emit_to = n_blocks;
    }
    const int rc = g.n_fft == 512
        ? launch_denoise512(s, mode, n_cu, pcm, n_blocks, calls_before, st_in, st_out, ver_base, snap_mask, noise_rows,
                            table, g.win512, out, precast, sh, redo)
        : launch_denoise1024(s, mode, k_opt, n_cu, pcm, n_blocks, calls_before, st_in, st_out, ver_base, snap_mask,
                             noise_rows, table, out, precast, sh, redo);
    if (rc || !lists) return rc;
    launch_denoise_redo(s, g.n_fft, pcm, n_blocks, calls_before, st_in, st_out, ver_base, snap_mask, noise_rows, out, precast,
                        sh, redo, mode);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// range / ext0: a shard's event range and the global index of its first block (NULL / 0 when not sharded)
static void launch_noise_accum(hipStream_t s, DenoiseGeom g, int grid, const short *pcm, long n_blocks,
                               const DenoiseState *st_in, const int *events, const int *ev_n, const DenoisePlan *plan,
                               const int *ver_base, const unsigned long long *snap_mask, const float2 *table,
                               const NoiseAccum &acc, float *rows, const int *range, long ext0)
{
    if (g.n_fft == 512)
        hipLaunchKernelGGL(noise_accum512_kernel, dim3((unsigned)grid), dim3(64), 0, s, pcm, n_blocks, st_in, events, ev_n,
                           plan, ver_base, snap_mask, table, g.win512, acc, rows, 10, range, ext0);
    else
        hipLaunchKernelGGL(noise_accum_kernel, dim3((unsigned)grid), dim3(64), 0, s, pcm, n_blocks, st_in, events, ev_n, plan,
                           ver_base, snap_mask, table, acc, rows, 10, range, ext0);
}

int launch_noise_estimate(hipStream_t s, DenoiseGeom g, const short *pcm, long n_blocks, const DenoiseState *st_in,
                          DenoiseState *st_out, const int *events, const int *ev_n, const DenoisePlan *plan,
                          const int *ver_base, const unsigned long long *snap_mask, const float2 *table,
                          const NoiseAccum &acc, float *noise_rows)
{
    const int grid = n_blocks < kNoiseChunks ? (int)(n_blocks > 0 ? n_blocks : 1) : kNoiseChunks;
    if (n_blocks > 0)
        launch_noise_accum(s, g, grid, pcm, n_blocks, st_in, events, ev_n, plan, ver_base, snap_mask, table, acc, noise_rows,
                           nullptr, 0L);
    hipLaunchKernelGGL(noise_combine_kernel, dim3(g.n_fft / kCombineBins), dim3(1024), 0, s, plan, st_in, st_out, acc,
                       noise_rows, grid, (const int *)nullptr, (const float *)nullptr, (float *)nullptr, (float *)nullptr, 1);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// A rank's events through the chunked average (noise_accum_kernel / noise_combine_kernel) in two passes: the first
// leaves the rank's composed map in `summary` (and every latched row as its partial map), the second -- once the
// maps of the ranks before it are known -- completes the rows from the average this rank starts from.
static int shard_accum_grid(long own) { return own < kNoiseChunks ? (int)(own > 0 ? own : 1) : kNoiseChunks; }

int launch_shard_summary(hipStream_t s, DenoiseGeom g, const short *pcm_ext, long n_ext, long ext0, long b0, long b1,
                         const int *events, const int *ev_n, const DenoisePlan *plan, const int *ver_base,
                         const unsigned long long *snap_mask, const float2 *table, int *range, const NoiseAccum &acc,
                         float *rows, float *summary)
{
    hipLaunchKernelGGL(event_range_kernel, dim3(1), dim3(64), 0, s, events, plan, ver_base, snap_mask, b0, b1, range);
    const int grid = shard_accum_grid(b1 - b0);
    launch_noise_accum(s, g, grid, pcm_ext, n_ext, nullptr, events, ev_n, plan, ver_base, snap_mask, table, acc, rows, range,
                       ext0);
    hipLaunchKernelGGL(noise_combine_kernel, dim3(g.n_fft / kCombineBins), dim3(1024), 0, s, plan,
                       (const DenoiseState *)nullptr, (DenoiseState *)nullptr, acc, rows, grid, (const int *)range,
                       (const float *)nullptr, summary, (float *)nullptr, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_shard_rows(hipStream_t s, DenoiseGeom g, const float *summaries_all, int rank, long b0, long b1,
                      const DenoisePlan *plan, const int *range, const NoiseAccum &acc, float *a_in, float *rows,
                      float *last)
{
    hipLaunchKernelGGL(fold_summaries_kernel, dim3(g.n_fft / 256), dim3(256), 0, s, summaries_all, rank, a_in);
    hipLaunchKernelGGL(noise_combine_kernel, dim3(g.n_fft / kCombineBins), dim3(1024), 0, s, plan,
                       (const DenoiseState *)nullptr, (DenoiseState *)nullptr, acc, rows, shard_accum_grid(b1 - b0), range,
                       (const float *)a_in, (float *)nullptr, last, 1);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_shard_row0(hipStream_t s, DenoiseGeom g, const float *last_all, int rank, float *rows)
{
    hipLaunchKernelGGL(select_row0_kernel, dim3(g.n_fft / 256), dim3(256), 0, s, last_all, rank, rows);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
