// mvdrn_batch_api.hip -- C ABI of the n-microphone MVDR beamformer over a batch of ragged utterances, each a fresh
// stream (include/jdsp.h "batched n-microphone MVDR"; the kernels: mvdrn_batch_kernels.hip).  The entries share the
// handle's configuration (n_mics, steering, loading, the VAD's window) and nothing of its stream.
#include "jdsp_internal.h"

using jdsp::fail;

static int batch_supported(jdsp_mvdrn *h, const char *what)
{
    if (h->n_fft == 1024) return JDSP_OK;
    return fail(h->ctx, JDSP_EINVAL, (std::string(what) + ": 1024-point handles only; a 512-point handle pairs two blocks "
                                      "in one inverse transform, which is not built across utterance boundaries").c_str());
}

static jdsp::MvnBatchView view(const jdsp_mvdrn *h)
{
    const jdsp_mvdrn::BatchWs &w = h->bws;
    return {w.code.get(), w.evpre.get(), w.events.get(), w.tile_off.get(), w.ev_first.get(), w.slot_utt.get(),
            w.spec.get(), w.weights.get(), w.chunk.get()};
}

extern "C" {

int jdsp_mvdrn_batch_reserve(jdsp_mvdrn *h, long max_blocks_total, long max_utts)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (max_blocks_total < 0 || max_utts < 0 || max_blocks_total > 0x7ffffff0L || max_utts > 0x7ffffff0L)
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_batch_reserve: max_blocks_total and max_utts must be 0 .. 2^31 - 16");
    int rc = batch_supported(h, "jdsp_mvdrn_batch_reserve");
    if (rc) return rc;
    jdsp_mvdrn::BatchWs &w = h->bws;
    if (max_blocks_total <= w.cap_blocks && max_utts <= w.cap_utts) return JDSP_OK;
    const long cap_b = max_blocks_total > w.cap_blocks ? max_blocks_total : w.cap_blocks;
    const long cap_u = max_utts > w.cap_utts ? max_utts : w.cap_utts;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));          // nothing enqueued still uses the old buffers
    w = {};                                                    // freed before anything is allocated
    const size_t n = (size_t)cap_b, nu = (size_t)cap_u, P = (size_t)jdsp::kMvnBatchEvents;
    hipError_t e = w.code.alloc(n + 1);
    if (e == hipSuccess) e = w.evpre.alloc(n + 1);
    if (e == hipSuccess) e = w.events.alloc(n + 1);
    if (e == hipSuccess) e = w.tile_off.alloc(n / 2048 + 2);
    if (e == hipSuccess) e = w.ev_first.alloc(nu + 1);
    if (e == hipSuccess) e = w.slot_utt.alloc(nu + n / P + 2);
    // worst case: every block is an estimation frame -- one spectrum set and one weight set per block, as mvdrn_reserve
    if (e == hipSuccess) e = w.spec.alloc((n + 1) * h->n_mics * (size_t)h->n_bins);
    if (e == hipSuccess) e = w.weights.alloc((n + 1) * (size_t)h->n_bins * 8);
    if (e == hipSuccess) e = w.chunk.alloc((2 * n / P + 2) * (size_t)h->n_bins * 64);
    if (e != hipSuccess) {
        w = {};
        return fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_mvdrn_batch_reserve", e);
    }
    w.cap_blocks = cap_b;
    w.cap_utts = cap_u;
    return JDSP_OK;
}

int jdsp_mvdrn_batch_dev(jdsp_mvdrn *h, const int16_t *pcm_dev, long chan_stride, const int64_t *sample_first_dev,
                         const int64_t *block_first_dev, long n_utts, long n_blocks_total, int16_t *out_dev,
                         float *precast_dev, uint8_t *flags_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_utts < 0 || n_blocks_total < 0) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_batch: n_utts or n_blocks_total < 0");
    int rc = batch_supported(h, "jdsp_mvdrn_batch");
    if (rc) return rc;
    if (!jdsp::aligned(pcm_dev, 16) || (chan_stride & 7) || !jdsp::aligned(out_dev, 4) || !jdsp::aligned(precast_dev, 4) ||
        !jdsp::aligned(sample_first_dev, 8) || !jdsp::aligned(block_first_dev, 8))
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_batch: pcm must be 16-byte aligned and chan_stride a multiple of 8; "
                                      "out and precast 4-byte, the offset arrays 8-byte aligned");
    if (n_utts == 0 || n_blocks_total == 0) return JDSP_OK;     // nothing to launch
    if (!out_dev && !precast_dev && !flags_dev) return JDSP_OK; // nothing to write
    if (!pcm_dev || !sample_first_dev || !block_first_dev)
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_batch: pcm, sample_first or block_first is NULL");
    if (chan_stride < 0) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_batch: chan_stride < 0");
    const jdsp_mvdrn::BatchWs &w = h->bws;
    if (n_blocks_total > w.cap_blocks || n_utts > w.cap_utts)
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_batch_dev: the batch exceeds what jdsp_mvdrn_batch_reserve sized "
                                      "(the device entry does not allocate)");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (jdsp::launch_mvdrn_batch(ctx->stream, pcm_dev, chan_stride, h->n_mics,
                                 reinterpret_cast<const long long *>(sample_first_dev),
                                 reinterpret_cast<const long long *>(block_first_dev), n_utts, n_blocks_total,
                                 h->w_vad.get(), h->steer.get(), h->loading, ctx->stft1024_table.get(), view(h), flags_dev,
                                 out_dev, precast_dev))
        return fail(ctx, JDSP_EHIP, "jdsp_mvdrn_batch: launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_mvdrn_batch(jdsp_mvdrn *h, const int16_t *pcm_host, long chan_stride, long n_samples,
                     const int64_t *sample_first_host, const int64_t *block_first_host, long n_utts, int16_t *out_host,
                     float *precast_host, uint8_t *flags_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_utts < 0 || n_samples < 0 || chan_stride < n_samples)
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_batch: n_utts or n_samples < 0, or chan_stride < n_samples");
    int rc = batch_supported(h, "jdsp_mvdrn_batch");
    if (rc) return rc;
    if (n_utts > 0 && (!sample_first_host || !block_first_host))
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_batch: sample_first or block_first is NULL");
    jdsp::RaggedOffsets offs;                                  // a span of b blocks is b hops: n = hop
    if (offs.check(ctx, "jdsp_mvdrn_batch", "block_first", sample_first_host, block_first_host, n_utts, n_samples, h->block,
                   h->block))
        return JDSP_EINVAL;
    const long n_total = offs.lay.n_total, end = offs.lay.end;
    // what no launch writes is zero: everything outside the spans and every span's first block
    if (out_host && n_samples) memset(out_host, 0, (size_t)n_samples * sizeof(int16_t));
    if (precast_host && n_samples) memset(precast_host, 0, (size_t)n_samples * sizeof(float));
    if (n_total == 0 || (!out_host && !precast_host && !flags_host)) return JDSP_OK;      // nothing to launch
    if (!pcm_host) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_batch: pcm is NULL");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    rc = jdsp_mvdrn_batch_reserve(h, n_total, n_utts);
    if (rc) return rc;
    const long stride_dev = (end + 7) & ~7L;                   // the planes repacked: nothing past the last span is read
    jdsp::HostCall hc(ctx, "jdsp_mvdrn_batch");
    offs.upload(hc);
    int16_t *d_pcm = hc.alloc<int16_t>((size_t)stride_dev * h->n_mics * sizeof(int16_t));
    for (int m = 0; m < h->n_mics; m++)
        hc.upload_to(d_pcm + (size_t)m * stride_dev, pcm_host + (size_t)m * chan_stride, (size_t)end * sizeof(int16_t));
    const bool run = offs.lay.longest >= 2;                    // otherwise nothing but the flags can come out
    int16_t *d_out = run && out_host ? hc.alloc<int16_t>((size_t)end * sizeof(int16_t)) : nullptr;
    float *d_pre = run && precast_host ? hc.alloc<float>((size_t)end * sizeof(float)) : nullptr;
    uint8_t *d_flags = flags_host ? hc.alloc<uint8_t>((size_t)n_total) : nullptr;
    if (d_out) hc.zero(d_out, (size_t)end * sizeof(int16_t));
    if (d_pre) hc.zero(d_pre, (size_t)end * sizeof(float));
    if (hc.ok())
        hc.result(jdsp_mvdrn_batch_dev(h, d_pcm, stride_dev, offs.d_sample, offs.d_unit, n_utts, n_total, d_out, d_pre,
                                       d_flags));
    hc.download(out_host, d_out, d_out ? (size_t)end * sizeof(int16_t) : 0);
    hc.download(precast_host, d_pre, d_pre ? (size_t)end * sizeof(float) : 0);
    hc.download(flags_host, d_flags, (size_t)n_total);
    return hc.finish();
}

}  // extern "C"
