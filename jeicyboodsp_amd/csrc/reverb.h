// reverb.h -- what reverb_api.hip and reverb_kernels.hip share: the handle of the batched reverberator (include/jdsp.h
// "batched reverberation") and the launcher of its three kernels; and what reverb_live_api.hip and
// reverb_live_kernels.hip share: the view of the live streams' state (include/jdsp.h "live reverberation streams") and
// the launchers of their kernels.
#pragma once
#include "jdsp_internal.h"

namespace jdsp {

constexpr int kReverbBlock = 512;          // samples per block, and taps per partition
constexpr int kReverbMaxPart = 15;         // partitions of one response: what one workgroup's LDS carries next to its waves
constexpr int kReverbMaxTaps = kReverbBlock * kReverbMaxPart;
constexpr int kReverbMaxIrs = 16384;
constexpr int kReverbGroup = 32;           // G: output blocks per workgroup of reverb_mac_kernel (16 waves x 2)

struct ReverbBatchArgs {
    const short *pcm;
    const long long *sample_first, *block_first;      // [n_utts], [n_utts + 1]
    const int *ir;                                    // [n_utts]
    const float *gain;                                // [n_utts] or nullptr: 1
    long n_utts, n_blocks_total;
    short *out_i16;                                   // either may be nullptr
    float *out_f32;
};

// plan (workgroups per utterance, prefixed), analysis (one spectrum row per block) and multiply-accumulate / inverse,
// enqueued on st; every grid comes from a.n_utts and a.n_blocks_total.  X: [n_blocks_total] rows, wg_first: [n_utts + 1].
int launch_reverb_batch(hipStream_t st, const ReverbBatchArgs &a, const float2 *bank, int n_part, int n_irs,
                        const float2 *rect_table, float2 *X, long long *wg_first);

// The live streams of a handle, as the kernels see them.  Per stream, each part once: blocks_seen, the last block's
// samples, and a ring of the last P - 1 spectrum rows (the row of stream block i at slot i mod (P - 1); none at P = 1).
// X is the call workspace: one row per block of a delivery.
struct ReverbLive {
    long long *seen;                                  // [n_streams]
    short *last;                                      // [n_streams][kReverbBlock]
    float2 *ring;                                     // [n_streams][n_part - 1][kUpolsRowPitch]
    float2 *X;                                        // [max_blocks_total][kUpolsRowPitch]
};

struct ReverbLiveArgs {
    const short *pcm;
    const long long *stream_id, *sample_first, *block_first;   // [n_chunks], [n_chunks], [n_chunks + 1]
    const int *ir;                                    // [n_chunks]
    const float *gain;                                // [n_chunks] or nullptr: 1
    long n_chunks, n_blocks_total;
    short *out_i16;                                   // either may be nullptr; with both only the state advances
    float *out_f32;
};

// analysis (rows of the new blocks), plan and multiply-accumulate / inverse (skipped without an output), commit (rows,
// samples and counts into the state): one linear chain on st, every grid from a.n_chunks and a.n_blocks_total.
// wave_first: [n_chunks + 1].
int launch_reverb_live(hipStream_t st, const ReverbLiveArgs &a, const float2 *bank, int n_part, int n_irs,
                       const float2 *rect_table, const ReverbLive &lv, long long *wave_first);
int launch_reverb_live_reset(hipStream_t st, const long long *stream_id, long n_ids, long n_streams, const ReverbLive &lv);

}  // namespace jdsp

struct jdsp_reverb {
    jdsp_ctx *ctx = nullptr;
    int n_irs = 0, n_taps = 0, n_part = 0;
    jdsp::DevBuf<float2> bank;             // [n_irs][n_part][kUpolsRowPitch]: bins 0..512 of every partition, FP32
    jdsp::DevBuf<float2> X;                // [cap_blocks][kUpolsRowPitch]: the batch's block spectra
    jdsp::DevBuf<long long> wg_first;      // [cap_utts + 1]: the plan
    long cap_blocks = -1, cap_utts = -1;   // -1: jdsp_reverb_batch_reserve has not been called
    // the live streams (jdsp_reverb_streams_reserve), kept apart from the batch workspace
    struct LiveWs {
        jdsp::DevBuf<long long> seen, wave_first;      // [n_streams], [n_streams + 1]
        jdsp::DevBuf<short> last;
        jdsp::DevBuf<float2> ring, X;
        jdsp::ReverbLive view = {};
        long n_streams = 0, cap_blocks = 0;            // n_streams 0: not reserved
    } lws;
};
