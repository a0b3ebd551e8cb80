// reverb_api.hip -- C ABI of the batched reverberator (include/jdsp.h "batched reverberation"): a bank of long impulse
// responses and a stateless entry over a batch of ragged utterances, each with its own response and gain.
#include "reverb.h"

using jdsp::fail;

extern "C" {

int jdsp_reverb_create(jdsp_ctx *ctx, const double *taps, int n_irs, int n_taps, jdsp_reverb **out)
{
    if (!ctx || !out) return JDSP_EINVAL;
    *out = nullptr;
    if (!taps || n_taps < 1 || n_taps > jdsp::kReverbMaxTaps || n_irs < 1 || n_irs > jdsp::kReverbMaxIrs)
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_create: taps is NULL, or n_taps outside 1 .. 7680, or n_irs outside 1 .. 16384");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp::ensure_stft1024_table_rect(ctx);
    if (rc) return rc;
    jdsp_reverb *h = new (std::nothrow) jdsp_reverb();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_reverb_create");
    h->ctx = ctx;
    h->n_irs = n_irs;
    h->n_taps = n_taps;
    const int P = h->n_part = (n_taps + jdsp::kReverbBlock - 1) / jdsp::kReverbBlock;
    const size_t rows = (size_t)n_irs * P;
    const hipError_t e = h->bank.alloc(rows * jdsp::kUpolsRowPitch);
    if (e != hipSuccess) rc = fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_reverb_create: bank", e);
    // spectra of the 512-tap partitions, each zero-padded to 1024, in FP64 on the device as jdsp_fastconv_create's,
    // bins 0..512 kept as FP32 rows; a slice of the bank at a time, so that the FP64 staging stays at 2 x 64 MB
    const int irs_per_slice = 4096 / P;
    for (int i0 = 0; i0 < n_irs && !rc; i0 += irs_per_slice) {
        const int n = n_irs - i0 < irs_per_slice ? n_irs - i0 : irs_per_slice;
        const size_t srows = (size_t)n * P;
        std::vector<double> part(srows * 1024 * 2, 0.0);
        for (int f = 0; f < n; f++)
            for (int i = 0; i < n_taps; i++)
                part[2 * (((size_t)f * P + i / 512) * 1024 + i % 512)] = taps[(size_t)(i0 + f) * n_taps + i];
        jdsp::HostCall hc(ctx, "jdsp_reverb_create");
        const double *d_p = hc.upload(part.data(), srows * 1024 * 16);
        double *d_P = hc.alloc<double>(srows * 1024 * 16);
        if (hc.ok()) hc.result(jdsp_fft_process_f64_dev(ctx, d_p, d_P, 1024, (long)srows, 1));
        if (hc.ok() && jdsp::launch_spectrum_rows_to_f32(ctx->stream, (const double2 *)d_P,
                                                         h->bank.get() + (size_t)i0 * P * jdsp::kUpolsRowPitch, (long)srows))
            hc.result(fail(ctx, JDSP_EHIP, "jdsp_reverb_create: spectrum_rows_to_f32 launch", hipGetLastError()));
        rc = hc.finish();
    }
    if (rc) {
        jdsp_reverb_destroy(h);
        return rc;
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_reverb_destroy(jdsp_reverb *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_reverb_n_irs(const jdsp_reverb *h) { return h ? h->n_irs : 0; }
int jdsp_reverb_n_part(const jdsp_reverb *h) { return h ? h->n_part : 0; }
int jdsp_reverb_block_len(const jdsp_reverb *h) { return h ? jdsp::kReverbBlock : 0; }

int jdsp_reverb_batch_reserve(jdsp_reverb *h, long n_blocks, long n_utts)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0 || n_utts < 0 || n_blocks > 0x7ffffff0L)
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_batch_reserve: n_blocks must be 0 .. 2^31 - 16, n_utts >= 0");
    if (n_blocks <= h->cap_blocks && n_utts <= h->cap_utts) return JDSP_OK;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const long nb = n_blocks > h->cap_blocks ? n_blocks : h->cap_blocks, nu = n_utts > h->cap_utts ? n_utts : h->cap_utts;
    h->cap_blocks = h->cap_utts = -1;
    h->X.reset();                                               // freed before anything is allocated
    h->wg_first.reset();
    hipError_t e = h->X.alloc((size_t)(nb > 0 ? nb : 1) * jdsp::kUpolsRowPitch);
    if (e == hipSuccess) e = h->wg_first.alloc((size_t)nu + 1);
    if (e != hipSuccess) {
        h->X.reset();
        h->wg_first.reset();
        return fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_reverb_batch_reserve", e);
    }
    h->cap_blocks = nb;
    h->cap_utts = nu;
    return JDSP_OK;
}

int jdsp_reverb_batch_dev(jdsp_reverb *h, const int16_t *pcm_dev, const int64_t *sample_first_dev,
                          const int64_t *block_first_dev, const int32_t *ir_dev, const float *gain_dev, long n_utts,
                          long n_blocks_total, int16_t *out_i16_dev, float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_utts < 0 || n_blocks_total < 0) return fail(ctx, JDSP_EINVAL, "jdsp_reverb_batch: n_utts or n_blocks_total < 0");
    if (!jdsp::aligned(pcm_dev, 16) || !jdsp::aligned(out_i16_dev, 16) || !jdsp::aligned(out_f32_dev, 8) ||
        !jdsp::aligned(sample_first_dev, 8) || !jdsp::aligned(block_first_dev, 8) || !jdsp::aligned(ir_dev, 4) ||
        !jdsp::aligned(gain_dev, 4))
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_batch: pcm and out_i16 must be 16-byte, out_f32 and the offset arrays "
                                      "8-byte, ir and gain 4-byte aligned");
    if (n_utts == 0 || n_blocks_total == 0) return JDSP_OK;    // no utterance, or only empty ones: nothing to launch
    if (!out_i16_dev && !out_f32_dev) return JDSP_OK;           // nothing to write
    if (!pcm_dev || !sample_first_dev || !block_first_dev || !ir_dev)
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_batch: pcm, sample_first, block_first or ir is NULL");
    if (h->cap_blocks < 0)
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_batch_dev: call jdsp_reverb_batch_reserve first (the device entry does "
                                      "not allocate)");
    if (n_blocks_total > h->cap_blocks || n_utts > h->cap_utts)
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_batch_dev: the batch exceeds what jdsp_reverb_batch_reserve sized "
                                      "(the device entry does not allocate)");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const jdsp::ReverbBatchArgs a = {pcm_dev, reinterpret_cast<const long long *>(sample_first_dev),
                                     reinterpret_cast<const long long *>(block_first_dev), ir_dev, gain_dev, n_utts,
                                     n_blocks_total, out_i16_dev, out_f32_dev};
    if (jdsp::launch_reverb_batch(ctx->stream, a, h->bank.get(), h->n_part, h->n_irs, ctx->stft1024_table_rect.get(),
                                  h->X.get(), h->wg_first.get()))
        return fail(ctx, JDSP_EHIP, "jdsp_reverb_batch: launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_reverb_batch(jdsp_reverb *h, const int16_t *pcm_host, long n_samples, const int64_t *sample_first_host,
                      const int64_t *block_first_host, const int32_t *ir_host, const float *gain_host, long n_utts,
                      int16_t *out_i16_host, float *out_f32_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_utts < 0 || n_samples < 0) return fail(ctx, JDSP_EINVAL, "jdsp_reverb_batch: n_utts or n_samples < 0");
    if (n_utts > 0 && (!sample_first_host || !block_first_host || !ir_host))
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_batch: sample_first, block_first or ir is NULL");
    return jdsp::reverb_host_call(h, "jdsp_reverb_batch", false, pcm_host, n_samples, nullptr, sample_first_host, block_first_host,
                                  ir_host, gain_host, n_utts, out_i16_host, out_f32_host);
}

}  // extern "C"
