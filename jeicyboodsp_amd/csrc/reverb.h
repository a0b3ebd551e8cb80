// reverb.h -- what reverb_api.hip and reverb_kernels.hip share: the handle of the batched reverberator (include/jdsp.h
// "batched reverberation") and the launcher of its three kernels.
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

}  // namespace jdsp

struct jdsp_reverb {
    jdsp_ctx *ctx = nullptr;
    int n_irs = 0, n_taps = 0, n_part = 0;
    jdsp::DevBuf<float2> bank;             // [n_irs][n_part][kUpolsRowPitch]: bins 0..512 of every partition, FP32
    jdsp::DevBuf<float2> X;                // [cap_blocks][kUpolsRowPitch]: the batch's block spectra
    jdsp::DevBuf<long long> wg_first;      // [cap_utts + 1]: the plan
    long cap_blocks = -1, cap_utts = -1;   // -1: jdsp_reverb_batch_reserve has not been called
};
