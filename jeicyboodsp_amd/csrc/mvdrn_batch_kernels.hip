// mvdrn_batch_kernels.hip -- the n-microphone MVDR beamformer (mvdrn_kernels.hip) over a batch of ragged utterances,
// each a fresh stream, in one launch sequence (include/jdsp.h, jdsp_mvdrn_batch_dev; the layout and the utterance walk:
// ragged_batch.h).  1024-point frames only.
//
// What makes a batch clean: block j of an utterance is an estimation frame ("event") iff it and the block before it
// are quiet and both lie in the utterance -- a local predicate, no run-length scan; the covariance is a running sum
// from zero; and the beamformed frame reads one block back, silence in front of an utterance's first block.  So:
//
//   mvnb_vad_kernel          the energy test on microphone 0 (BeamForming_MVDR_ver1.cpp:233, no zero-crossing term) per
//                            block of the concatenated axis, with a bit that marks an utterance's first block
//   mvnb_count / _tile_scan / _plan_kernel   ONE inclusive prefix sum of the event predicate over the concatenated axis,
//                            evpre[j], in tiles of 2,048 blocks: the global event list, and from it everything else --
//                            utterance u's events are [ev_first[u], ev_first[u + 1]), ev_first[u] = evpre[block_first[u] - 1]
//   mvnb_utt_kernel          ev_first per utterance and the chunk slots (below)
//   mvnb_event_spectra_kernel   X_m[k] of the frame [block j - 1, block j] of every event, both blocks inside the span
//   mvnb_chunk_sums / _prefix / mvnb_update_kernel   R_k and the weights after every event, per utterance from zero
//   mvnb_apply_kernel        one wave per block: the beamformed frame on span addresses
// The last four run the stream kernels' arithmetic, written once: the spectrum, the range sum and the emit are functions
// of mvdrn_common.h, the walk with its solve and the beamformed frame are the body fragments mvdrn_walk_body.h and
// mvdrn_frame_body.h, which mvdrn_kernels.hip includes too.  What is written here is what a batch has of its own: the
// VAD, the prefix sum, the slots and the span addresses.
//
// The weight table has row 0 for "no event yet" (the zero matrix, solved like any other: the non-finite weights of a
// fresh handle, the same for every utterance, so one row serves all) and row e + 1 for the e-th event of the GLOBAL
// list.  Block j of utterance u uses row evpre[j], or row 0 when evpre[j] == ev_first[u].
//
// Chunks.  Utterance u's E_u events are cut into chunks of kMvnBatchEvents = P events, ceil(E_u / P) of them: the cut
// depends on nothing but E_u, which is what makes an utterance's bits independent of its place in the batch.  Chunk
// counts are known on the device only, so chunk q of utterance u is given the SLOT u + ev_first[u] / P + q of a grid the
// host can size, n_utts + n_blocks / P + 1 slots: the slots of u end where those of u + 1 begin or before
// (floor(a + b) >= floor(a) + floor(b)), and a slot without a chunk exits.  Only an utterance of more than P events needs
// memory per chunk (the chunk's sum, then in place the matrix entering it): its chunk q has storage slot
// 2 ev_first[u] / P + q, which stays below 2 n_blocks / P + 1 because ceil(x) <= floor(2 x) for x > 1.
// P = 128: an utterance of real length (a hundred blocks) is one chunk, one walk of at most 128 solves (3.6 us each,
// mvdrn_kernels.hip) per eight bins, and the parallelism comes from the utterances; a long one gets a wave per 128
// events and eight bins; and the storage, 525 KB per slot, stays at 8.2 KB per reserved block beside the 65.7 KB of
// spectra and weights.  Not tuned against a measurement.
#include "frame_io.h"
#include "jdsp_internal.h"
#include "mvdrn_common.h"
#include "ragged_batch.h"

namespace jdsp {

typedef u32x4 u32x4_span __attribute__((aligned(4)));      // sample_first is even: a lane's 16 bytes are 4-byte aligned
constexpr int kMvnbVadBlocks = 4;                          // blocks per wave of the VAD, as kVadBlocksPerWave
constexpr int kMvnbTile = 2048;                            // blocks per workgroup of the prefix sum: 256 threads x 8
constexpr int P = kMvnBatchEvents;

// ---- 1. VAD: code[j] = voice | first-block-of-its-utterance << 1 -----------------------------------------------------
// vad_flags_kernel's energy decision (denoise_kernels.hip), statement for statement, without its zero-crossing count.
__global__ __launch_bounds__(64) void mvnb_vad_kernel(const short *__restrict__ pcm,
                                                      const long long *__restrict__ sample_first,
                                                      const long long *__restrict__ block_first, long n_utts,
                                                      long n_blocks, const double *__restrict__ w_vad,
                                                      unsigned char *__restrict__ code, unsigned char *__restrict__ flags)
{
    const int lane = threadIdx.x;
    const long b0 = (long)blockIdx.x * kMvnbVadBlocks;
    if (b0 >= n_blocks) return;
    double w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = w_vad[8 * lane + k];
    long u = ragged_find_utt(block_first, n_utts, b0);
    long ub = uniform_i64(block_first + u), ue = uniform_i64(block_first + u + 1);
    long base = uniform_i64(sample_first + u) - ub * 512;      // global block j starts at base + 512 j
    u32x4 img[kMvnbVadBlocks];
    unsigned int first_bits = 0, voice_bits = 0;               // wave-uniform
#pragma unroll
    for (int i = 0; i < kMvnbVadBlocks; i++) {
        const long b = b0 + i < n_blocks ? b0 + i : n_blocks - 1;
        if (b >= ue) {                                          // block b exists, so a non-empty utterance follows
            ub = ue;
            ragged_next_utt(block_first, n_utts, u, ue);
            base = uniform_i64(sample_first + u) - ub * 512;
        }
        if (b == ub) first_bits |= 1u << i;
        img[i] = reinterpret_cast<const u32x4_span *>(pcm + base + b * 512)[lane];
    }
#pragma unroll
    for (int i = 0; i < kMvnbVadBlocks; i++) {
        int x[8];
        x[0] = (short)(img[i].x & 0xffffu); x[1] = (int)img[i].x >> 16;
        x[2] = (short)(img[i].y & 0xffffu); x[3] = (int)img[i].y >> 16;
        x[4] = (short)(img[i].z & 0xffffu); x[5] = (int)img[i].z >> 16;
        x[6] = (short)(img[i].w & 0xffffu); x[7] = (int)img[i].w >> 16;
        unsigned int qa = 0, qb = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int sv = (int)((double)x[k] * w[k]);              // (short)(short * double), in range
            if (k < 4) qa += (unsigned int)__mul24(sv, sv); else qb += (unsigned int)__mul24(sv, sv);
        }
        const unsigned int cap = 1u << 20;
        const unsigned int e = wave_sum_u32((qa < cap ? qa : cap) + (qb < cap ? qb : cap));
        if (e > 700u * 128u * 8u) voice_bits |= 1u << i;
    }
    if (lane < kMvnbVadBlocks && b0 + lane < n_blocks) {
        const unsigned int v = (voice_bits >> lane) & 1u;
        code[b0 + lane] = (unsigned char)(v | (((first_bits >> lane) & 1u) << 1));
        if (flags) flags[b0 + lane] = (unsigned char)v;
    }
}

// ---- 2. the prefix sum of the event predicate ------------------------------------------------------------------------
// ev(j) = quiet(j), j not its utterance's first block, quiet(j - 1): code[j] == 0 and bit 0 of code[j - 1] clear (j is not
// a first block, so j >= 1).  Bit i of the result: block j0 + i, i < 8.
__device__ __forceinline__ unsigned int mvnb_events8(const unsigned char *__restrict__ code, long j0, long n_blocks)
{
    unsigned int bits = 0;
    if (j0 >= n_blocks) return 0;
    unsigned int before = j0 > 0 ? code[j0 - 1] : 1u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (j0 + i < n_blocks) {
            const unsigned int c = code[j0 + i];
            if (c == 0 && (before & 1u) == 0) bits |= 1u << i;
            before = c;
        }
    }
    return bits;
}

// the sum over a workgroup of 256 threads (four waves), in every thread; part: four words of LDS
__device__ __forceinline__ unsigned int mvnb_sum256(unsigned int v, unsigned int *part)
{
    const unsigned int ws = wave_sum_u32(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ws;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void mvnb_count_kernel(const unsigned char *__restrict__ code, long n_blocks,
                                                         int *__restrict__ tile_off)
{
    __shared__ unsigned int part[4];
    const long j0 = (long)blockIdx.x * kMvnbTile + 8 * (long)threadIdx.x;
    const unsigned int total = mvnb_sum256(__popc(mvnb_events8(code, j0, n_blocks)), part);
    if (threadIdx.x == 0) tile_off[blockIdx.x] = (int)total;
}

// tile_off[t] = events before tile t, tile_off[n_tiles] = all of them; one workgroup, 1,024 tiles a round
__global__ __launch_bounds__(1024) void mvnb_tile_scan_kernel(int *__restrict__ tile_off, long n_tiles)
{
    __shared__ int s[1024];
    __shared__ int carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (long t0 = 0; t0 < n_tiles; t0 += 1024) {
        const int mine = t0 + t < n_tiles ? tile_off[t0 + t] : 0;
        s[t] = mine;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int add = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        const int c = carry;
        if (t0 + t < n_tiles) tile_off[t0 + t] = c + s[t] - mine;
        __syncthreads();
        if (t == 1023) carry = c + s[1023];
        __syncthreads();
    }
    if (t == 0) tile_off[n_tiles] = carry;
}

// evpre[j] = events at or before block j; events[e] = the block of the e-th event
__global__ __launch_bounds__(256) void mvnb_plan_kernel(const unsigned char *__restrict__ code, long n_blocks,
                                                        const int *__restrict__ tile_off, int *__restrict__ evpre,
                                                        int *__restrict__ events)
{
    __shared__ unsigned int part[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long j0 = (long)blockIdx.x * kMvnbTile + 8 * (long)t;
    const unsigned int bits = mvnb_events8(code, j0, n_blocks);
    const unsigned int cnt = __popc(bits);
    unsigned int inc = cnt;                                     // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) part[wv] = inc;
    __syncthreads();
    unsigned int run = (unsigned int)tile_off[blockIdx.x] + inc - cnt;
    for (int i = 0; i < wv; i++) run += part[i];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (j0 + i < n_blocks) {
            if ((bits >> i) & 1u) events[run++] = (int)(j0 + i);
            evpre[j0 + i] = (int)run;
        }
    }
}

// ev_first[u], u <= n_utts, and the utterance of every chunk slot that can hold a chunk
__global__ __launch_bounds__(256) void mvnb_utt_kernel(const long long *__restrict__ block_first, long n_utts,
                                                       const int *__restrict__ evpre, int *__restrict__ ev_first,
                                                       int *__restrict__ slot_utt)
{
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    if (u > n_utts) return;
    const long b0 = block_first[u];
    const int e0 = b0 > 0 ? evpre[b0 - 1] : 0;
    ev_first[u] = e0;
    if (u == n_utts) return;
    const long b1 = block_first[u + 1];
    const int e1 = b1 > 0 ? evpre[b1 - 1] : 0;
    const long s0 = u + e0 / P, s1 = u + 1 + e1 / P;
    for (long s = s0; s < s1; s++) slot_utt[s] = (int)u;
}

// ---- 3. the spectra of the estimation frames -------------------------------------------------------------------------
// spec[(e * n_mics + m) * 513 + k] = X_m[k] of the frame [block j - 1, block j], j = events[e]: mvdrn_event_spectra_kernel
// with both blocks read from the span (an event is never an utterance's first block)
__global__ __launch_bounds__(64) void mvnb_event_spectra_kernel(const short *__restrict__ pcm, long chan_stride, int n_mics,
                                                                const long long *__restrict__ sample_first,
                                                                const long long *__restrict__ block_first, long n_utts,
                                                                const int *__restrict__ events,
                                                                const int *__restrict__ n_events_p,
                                                                const float2 *__restrict__ table, float2 *__restrict__ spec)
{
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    __shared__ __attribute__((aligned(16))) unsigned int stage[256];
    const int lane = threadIdx.x;
    const long total = (long)*n_events_p * n_mics;
    if ((long)blockIdx.x >= total) return;
    WaveTwiddles tw;
    load_wave_twiddles(tw, table, lane);
    const float2 wsp[2] = {table[kStftSplit + 2 * lane], table[kStftSplit + 2 * lane + 1]};
    for (long w = blockIdx.x; w < total; w += gridDim.x) {
        const int e = (int)(w / n_mics), m = (int)(w % n_mics);
        const long j = __builtin_amdgcn_readfirstlane(events[e]);
        const long u = ragged_find_utt(block_first, n_utts, j);
        const long at = uniform_i64(sample_first + u) + (j - uniform_i64(block_first + u)) * 512;   // block j's first sample
        const short *cur = pcm + (size_t)m * chan_stride + at;
        unsigned int raw[8];
        relayout_half(stage, lane, reinterpret_cast<const u32x4_span *>(cur - 512)[lane], raw);
        relayout_half(stage, lane, reinterpret_cast<const u32x4_span *>(cur)[lane], raw + 4);
        mvn_event_spectrum(raw, lds, lane, tw, wsp, spec + (size_t)w * kMvnBins);
    }
}

// ---- 4. covariance and weights, per utterance from zero --------------------------------------------------------------
// the chunk a slot holds (all of it wave-uniform): events [e0, e1) of the global list, chunk q of n_chunks of its
// utterance, whose storage slots start at store0.  n_chunks == 0: the slot holds nothing.
struct MvnbChunk { int e0, e1, q, n_chunks; long store0; };
__device__ __forceinline__ MvnbChunk mvnb_chunk_of(long slot, long n_utts, const int *__restrict__ ev_first,
                                                   const int *__restrict__ slot_utt)
{
    MvnbChunk c = {0, 0, 0, 0, 0};
    const int total = ev_first[n_utts];
    if (slot >= n_utts + total / P) return c;
    const long u = slot_utt[slot];
    const int ef = ev_first[u], n_ev = ev_first[u + 1] - ef;
    const int n_chunks = (n_ev + P - 1) / P;
    const long q = slot - (u + ef / P);
    if (q >= n_chunks) return c;
    c.q = (int)q;
    c.n_chunks = n_chunks;
    c.e0 = ef + (int)q * P;
    c.e1 = c.e0 + P < ef + n_ev ? c.e0 + P : ef + n_ev;
    c.store0 = 2 * (long)ef / P;
    return c;
}

// (8 bins, slot): the sum of X X^H / N over a chunk that another chunk of its utterance follows -- mvdrn_chunk_sums_kernel
__global__ __launch_bounds__(64) void mvnb_chunk_sums_kernel(const float2 *__restrict__ spec, int n_mics, long n_utts,
                                                             const int *__restrict__ ev_first,
                                                             const int *__restrict__ slot_utt, double2 *__restrict__ chunk_ws)
{
    const int lane = threadIdx.x, grp = lane >> 3, r = lane & 7;
    const MvnbChunk c = mvnb_chunk_of(blockIdx.x, n_utts, ev_first, slot_utt);
    if (c.n_chunks < 2 || c.q + 1 >= c.n_chunks) return;
    const int kb = blockIdx.y * 8 + grp;
    const int k = kb < kMvnBins ? kb : kMvnBins - 1;             // a group past the last bin repeats it and stores nothing
    cd S[8];
    mvn_range_sum(S, grp, r, spec, c.e0, c.e1, n_mics, kMvnBins, k, 1.0 / 1024.0);
    if (kb < kMvnBins) {
        double2 *dst = chunk_ws + ((size_t)(c.store0 + c.q) * kMvnBins + k) * 64 + 8 * r;
#pragma unroll
        for (int i = 0; i < 8; i++) dst[i] = d2_of(S[i]);
    }
}

// (8 bins, slot of an utterance's chunk 0): in place, chunk q's sum becomes the matrix entering chunk q -- the sums of
// the chunks before it, added in order from zero.  Elementwise: a lane takes 8 of the 512 values of its eight bins.
__global__ __launch_bounds__(64) void mvnb_chunk_prefix_kernel(long n_utts, const int *__restrict__ ev_first,
                                                               const int *__restrict__ slot_utt, double2 *__restrict__ chunk_ws)
{
    const int lane = threadIdx.x;
    const MvnbChunk c = mvnb_chunk_of(blockIdx.x, n_utts, ev_first, slot_utt);
    if (c.n_chunks < 2 || c.q != 0) return;
    const size_t per_slot = (size_t)kMvnBins * 64;
    double2 R[8];
#pragma unroll
    for (int i = 0; i < 8; i++) R[i] = make_double2(0.0, 0.0);
    for (int ch = 0; ch < c.n_chunks; ch++) {
        double2 *p = chunk_ws + (size_t)(c.store0 + ch) * per_slot;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const size_t at = (size_t)blockIdx.y * 512 + 64 * i + lane;
            if (at < per_slot) {
                const double2 s = ch + 1 < c.n_chunks ? p[at] : make_double2(0.0, 0.0);   // the last chunk has no sum
                p[at] = R[i];
                R[i].x += s.x;
                R[i].y += s.y;
            }
        }
    }
}

// (8 bins, slot): walks the chunk's events from the matrix entering it, one solve per event; the grid's LAST slot
// solves the zero matrix instead, row 0 of the weight table: a walk over no events that solves what it was given.  The
// walk and its solve are mvdrn_update_kernel's, the same text (mvdrn_walk_body.h): weights[(row * 8 + m) * 513 + k],
// row = event + 1 = the walk's version.
__global__ __launch_bounds__(64) void mvnb_update_kernel(const float2 *__restrict__ spec, int n_mics, long n_utts,
                                                         const int *__restrict__ ev_first, const int *__restrict__ slot_utt,
                                                         const double2 *__restrict__ chunk_ws,
                                                         const double2 *__restrict__ steer, double loading,
                                                         float2 *__restrict__ weights)
{
    const int lane = threadIdx.x, grp = lane >> 3, r = lane & 7;
    const bool row0 = blockIdx.x + 1 == gridDim.x;
    MvnbChunk c = {0, 0, 0, 0, 0};
    if (!row0) {
        c = mvnb_chunk_of(blockIdx.x, n_utts, ev_first, slot_utt);
        if (c.n_chunks == 0) return;
    }
    const int kb = blockIdx.y * 8 + grp;
    const int k = kb < kMvnBins ? kb : kMvnBins - 1;
    cd R[8];
#pragma unroll
    for (int i = 0; i < 8; i++) R[i] = {0.0, 0.0};
    if (c.q > 0) {                                                // chunk 0 starts from zero and has no storage
        const double2 *src = chunk_ws + ((size_t)(c.store0 + c.q) * kMvnBins + k) * 64 + 8 * r;
#pragma unroll
        for (int i = 0; i < 8; i++) R[i] = cd_of(src[i]);
    }
    constexpr int n_bins = kMvnBins;
    constexpr double inv_n = 1.0 / 1024.0;
    const int e0 = c.e0, e1 = c.e1;                               // the last slot: no events, and the leading version alone
    const bool lead = row0;
#include "mvdrn_walk_body.h"
}

// ---- 5. apply: one wave per block of the concatenated axis -----------------------------------------------------------
// The frame body of mvdrn_apply_pairs_kernel, the same text (mvdrn_frame_body.h).  The wave finds its utterance in scalar registers;
// an utterance's first block has silence in front of it and emits nothing, so its wave leaves at once; every other block
// reads the block before it from the span and writes time-aligned, at its own place in out and precast.
struct MvnbSpanSrc {
    const short *cur;                                              // block j of the next microphone asked for (they come in
    long chan_stride;                                              // order); block j - 1 lies before it
    __device__ __forceinline__ void load(int, int lane, u32x4 &prev, u32x4 &now)
    {
        prev = reinterpret_cast<const u32x4_span *>(cur - 512)[lane];
        now = reinterpret_cast<const u32x4_span *>(cur)[lane];
        cur += chan_stride;
    }
    __device__ __forceinline__ void done(int, int) const {}
};

__global__ __launch_bounds__(64) void mvnb_apply_kernel(const short *__restrict__ pcm, long chan_stride, int n_mics,
                                                        const long long *__restrict__ sample_first,
                                                        const long long *__restrict__ block_first, long n_utts,
                                                        long n_blocks, const int *__restrict__ evpre,
                                                        const int *__restrict__ ev_first,
                                                        const float2 *__restrict__ weights,
                                                        const float2 *__restrict__ table, short *__restrict__ out,
                                                        float *__restrict__ precast)
{
    const int lane = threadIdx.x;
    const long per_xcd = (gridDim.x + 7) >> 3;
    const long j = (long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (j >= n_blocks) return;
    const long u = ragged_find_utt(block_first, n_utts, j);
    const long ub = uniform_i64(block_first + u);
    if (j == ub) return;
    const long at = uniform_i64(sample_first + u) + (j - ub) * 512;     // block j's first sample; block j - 1 is in the span
    const int seen = __builtin_amdgcn_readfirstlane(evpre[j]);
    const int row = seen == __builtin_amdgcn_readfirstlane(ev_first[u]) ? 0 : seen;
    MvnbSpanSrc src = {pcm + at, chan_stride};
    const float2 *W = weights + (size_t)row * kMvnBins * 8;
#include "mvdrn_frame_body.h"
    mvn_emit_block<true>(y, lane, out ? out + at : nullptr, precast ? precast + at : nullptr);
}

int launch_mvdrn_batch(hipStream_t s, const short *pcm, long chan_stride, int n_mics, const long long *sample_first,
                       const long long *block_first, long n_utts, long n_blocks, const double *w_vad, const double2 *steer,
                       double loading, const float2 *table, const MvnBatchView &ws, unsigned char *flags, short *out,
                       float *precast)
{
    if (n_utts <= 0 || n_blocks <= 0) return 0;
    hipLaunchKernelGGL(mvnb_vad_kernel, dim3((unsigned)((n_blocks + kMvnbVadBlocks - 1) / kMvnbVadBlocks)), dim3(64), 0, s,
                       pcm, sample_first, block_first, n_utts, n_blocks, w_vad, ws.code, flags);
    if (!out && !precast) return hipGetLastError() == hipSuccess ? 0 : -1;      // the flags were all that was asked
    const long n_tiles = (n_blocks + kMvnbTile - 1) / kMvnbTile;
    hipLaunchKernelGGL(mvnb_count_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, ws.code, n_blocks, ws.tile_off);
    hipLaunchKernelGGL(mvnb_tile_scan_kernel, dim3(1), dim3(1024), 0, s, ws.tile_off, n_tiles);
    hipLaunchKernelGGL(mvnb_plan_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, ws.code, n_blocks, ws.tile_off, ws.evpre,
                       ws.events);
    hipLaunchKernelGGL(mvnb_utt_kernel, dim3((unsigned)(n_utts / 256 + 1)), dim3(256), 0, s, block_first, n_utts, ws.evpre,
                       ws.ev_first, ws.slot_utt);
    const long g1 = n_blocks * n_mics < 4096 ? n_blocks * n_mics : 4096;
    hipLaunchKernelGGL(mvnb_event_spectra_kernel, dim3((unsigned)g1), dim3(64), 0, s, pcm, chan_stride, n_mics, sample_first,
                       block_first, n_utts, ws.events, ws.ev_first + n_utts, table, ws.spec);
    const unsigned slots = (unsigned)(n_utts + n_blocks / P + 1), bin_groups = (kMvnBins + 7) / 8;
    hipLaunchKernelGGL(mvnb_chunk_sums_kernel, dim3(slots, bin_groups), dim3(64), 0, s, ws.spec, n_mics, n_utts, ws.ev_first,
                       ws.slot_utt, ws.chunk);
    hipLaunchKernelGGL(mvnb_chunk_prefix_kernel, dim3(slots, bin_groups), dim3(64), 0, s, n_utts, ws.ev_first, ws.slot_utt,
                       ws.chunk);
    hipLaunchKernelGGL(mvnb_update_kernel, dim3(slots + 1, bin_groups), dim3(64), 0, s, ws.spec, n_mics, n_utts, ws.ev_first,
                       ws.slot_utt, ws.chunk, steer, loading, ws.weights);
    const long grid = (n_blocks + 7) / 8 * 8;
    hipLaunchKernelGGL(mvnb_apply_kernel, dim3((unsigned)grid), dim3(64), 0, s, pcm, chan_stride, n_mics, sample_first,
                       block_first, n_utts, n_blocks, ws.evpre, ws.ev_first, ws.weights, table, out, precast);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
