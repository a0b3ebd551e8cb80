// reverb.h -- what reverb_api.hip and reverb_kernels.hip share: the handle of the batched reverberator (include/jdsp.h
// "batched reverberation") and the launcher of its three kernels; what reverb_live_api.hip and reverb_live_kernels.hip
// share: the view of the live streams' state (include/jdsp.h "live reverberation streams") and the launchers of their
// kernels; and what the two host entries share: their staging (reverb_host_call).  The kernels' shared text is
// reverb_body.h.
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

namespace jdsp {

// the scalar checks of the live entries (reverb_live_api.hip): streams reserved, counts inside what was reserved
int reverb_live_counts(jdsp_reverb *h, const char *entry, long n_chunks, long n_blocks_total);

// The host entries jdsp_reverb_batch (live false: n utterances) and jdsp_reverb_streams (live true: n chunks, their
// stream_id already checked) from the check of the offset arrays on, synchronous: the ir / gain scan, host outputs of
// n_samples zero outside what the call writes, the arrays and the samples to the device, the *_dev twin, the outputs
// back.  With no output to write the batch returns before it reserves anything; a live call goes on, since the streams'
// state still advances.
inline int reverb_host_call(jdsp_reverb *h, const char *entry, bool live, const int16_t *pcm, long n_samples,
                            const int64_t *stream_id, const int64_t *sample_first, const int64_t *block_first,
                            const int32_t *ir, const float *gain, long n, int16_t *out_i16, float *out_f32)
{
    jdsp_ctx *ctx = h->ctx;
    const auto reject = [&](const char *why) { return fail(ctx, JDSP_EINVAL, (std::string(entry) + ": " + why).c_str()); };
    RaggedOffsets offs;                                        // a span of b blocks is b hops: n = hop
    if (offs.check(ctx, entry, "block_first", sample_first, block_first, n, n_samples, kReverbBlock, kReverbBlock))
        return JDSP_EINVAL;
    for (long u = 0; u < n; u++) {
        if (ir[u] < 0 || ir[u] >= h->n_irs) return reject("an ir entry lies outside [0, n_irs)");
        if (gain && !std::isfinite(gain[u])) return reject("a gain is not finite");
    }
    const long n_total = offs.lay.n_total;
    const size_t end = (size_t)offs.lay.end;                   // nothing past the last span is read or written
    if (live)
        if (int rc = reverb_live_counts(h, entry, n, n_total)) return rc;
    // what no launch writes is zero: everything outside the spans
    if (out_i16 && n_samples) memset(out_i16, 0, (size_t)n_samples * sizeof(int16_t));
    if (out_f32 && n_samples) memset(out_f32, 0, (size_t)n_samples * sizeof(float));
    if (n_total == 0 || (!live && !out_i16 && !out_f32)) return JDSP_OK;         // nothing to launch
    if (!pcm) return reject("pcm is NULL");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (!live)
        if (int rc = jdsp_reverb_batch_reserve(h, n_total, n)) return rc;
    HostCall hc(ctx, entry);
    offs.upload(hc);
    const int64_t *d_id = live ? hc.upload(stream_id, (size_t)n * sizeof(int64_t)) : nullptr;
    const int16_t *d_pcm = hc.upload(pcm, end * sizeof(int16_t));
    const int32_t *d_ir = hc.upload(ir, (size_t)n * sizeof(int32_t));
    const float *d_gain = gain ? hc.upload(gain, (size_t)n * sizeof(float)) : nullptr;
    int16_t *d_out = out_i16 ? hc.alloc<int16_t>(end * sizeof(int16_t)) : nullptr;
    float *d_f32 = out_f32 ? hc.alloc<float>(end * sizeof(float)) : nullptr;
    if (d_out) hc.zero(d_out, end * sizeof(int16_t));
    if (d_f32) hc.zero(d_f32, end * sizeof(float));
    if (hc.ok())
        hc.result(live ? jdsp_reverb_streams_dev(h, d_pcm, d_id, offs.d_sample, offs.d_unit, d_ir, d_gain, n, n_total, d_out, d_f32)
                       : jdsp_reverb_batch_dev(h, d_pcm, offs.d_sample, offs.d_unit, d_ir, d_gain, n, n_total, d_out, d_f32));
    hc.download(out_i16, d_out, d_out ? end * sizeof(int16_t) : 0);
    hc.download(out_f32, d_f32, d_f32 ? end * sizeof(float) : 0);
    return hc.finish();
}

}  // namespace jdsp
