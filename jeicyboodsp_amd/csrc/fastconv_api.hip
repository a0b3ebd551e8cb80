// fastconv_api.hip -- C ABI of the overlap-save convolver (Fast_Convolution_Based_3DAudio_Impl.cpp).
#include "jdsp_internal.h"

using jdsp::fail;

#ifndef JDSP_STAMP
#define JDSP_STAMP 0
#endif
#if JDSP_STAMP
namespace jdsp { int read_wave_stamps(unsigned long long *host, int n); }
#endif
extern "C" {

int jdsp_fastconv_create(jdsp_ctx *ctx, const double *taps, int n_taps, int n_filters, int n_fft, jdsp_fastconv **out)
{
    if (!ctx || !out) return JDSP_EINVAL;
    *out = nullptr;
    if ((n_fft != 1024 && n_fft != 8192) || !taps || n_taps < 1 || n_taps > n_fft || n_filters < 1 || n_filters > 64)
        return fail(ctx, JDSP_EINVAL, "jdsp_fastconv_create: unsupported configuration (n_fft 1024 or 8192, 1 <= n_taps <= n_fft)");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp::ensure_stft1024_table(ctx);
    if (rc) return rc;
    jdsp_fastconv *h = new (std::nothrow) jdsp_fastconv();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_fastconv_create");
    h->ctx = ctx;
    h->n_fft = n_fft;
    h->n_taps = n_taps;
    h->n_filters = n_filters;
    h->block = n_fft - n_taps + 1;                                   // BLOCK_SIZE 1024 = 8192 - 7169 + 1
    h->n_hist = (n_taps - 1 + h->block - 1) / h->block;              // MAX_QUEUE_SIZE 7
    const size_t n = (size_t)n_filters * n_fft;
    // H = FFT(h zero-padded to n_fft) (:82-84,:140,:143), once, in double on the device
    std::vector<double> hpad(2 * n, 0.0);
    for (int f = 0; f < n_filters; f++)
        for (int i = 0; i < n_taps; i++) hpad[2 * ((size_t)f * n_fft + i)] = taps[(size_t)f * n_taps + i];
    hipError_t e = h->H.alloc(n);
    // Uniformly partitioned form of the same convolution (fastconv_kernels.hip).  JDSP_FASTCONV_PARTITIONED=0 keeps the
    // 8192-point kernel.  Its oldest frame starts 512 n_part samples back; the taps reach n_taps - 1 < 512 n_part back,
    // so the samples in between weigh nothing in the sum -- but they are in the frame the transform rounds.  The handle
    // carries all of them, and a stream gives the same bits however it is cut into calls.
    const char *env = getenv("JDSP_FASTCONV_PARTITIONED");
    const bool partitioned = n_fft == 8192 && h->block % 512 == 0 && !(env && env[0] == '0');
    h->hist_len = partitioned ? 512 * ((n_taps + 511) / 512) : n_taps - 1;
    const int hl = h->hist_len > 0 ? h->hist_len : 1;
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = h->hist[i].alloc((size_t)hl);
    if (e == hipSuccess && n_fft == 8192 && !ctx->conv_tw8192.get()) {
        std::vector<float2> a(4096), b(4096);
        jdsp::fill_conv_twiddles(a.data(), b.data());
        e = ctx->conv_tw4096.upload(a.data(), 4096);
        if (e == hipSuccess) e = ctx->conv_tw8192.upload(b.data(), 4096);
        if (e != hipSuccess) ctx->conv_tw4096.reset();       // both or neither
    }
    if (e != hipSuccess) rc = fail(ctx, JDSP_EHIP, "jdsp_fastconv_create: alloc", e);
    if (!rc) {
        jdsp::HostCall hc(ctx, "jdsp_fastconv_create");
        const double *d_h = hc.upload(hpad.data(), n * 16);
        double *d_H = hc.alloc<double>(n * 16);
        if (hc.ok()) hc.result(jdsp_fft_process_f64_dev(ctx, d_h, d_H, n_fft, n_filters, 1));
        if (hc.ok() && jdsp::launch_spectrum_to_f32(ctx->stream, (const double2 *)d_H, h->H.get(), (long)n,
                                                    n_fft == 1024 ? 1.0f / 2048.0f : 1.0f))   // 1024: the kernel's 1/2 and 1/1024
            hc.result(fail(ctx, JDSP_EHIP, "spectrum_to_f32 launch", hipGetLastError()));
        rc = hc.finish();
    }
    // spectra of the 512-tap partitions, each zero-padded to 1024, bins 0..512
    if (!rc && partitioned) {
        const int P = (n_taps + 511) / 512;
        const size_t rows = (size_t)n_filters * P;
        std::vector<double> part(rows * 1024 * 2, 0.0);
        for (int f = 0; f < n_filters; f++)
            for (int i = 0; i < n_taps; i++)
                part[2 * (((size_t)f * P + i / 512) * 1024 + i % 512)] = taps[(size_t)f * n_taps + i];
        if ((e = h->Hp.alloc(rows * jdsp::kUpolsRowPitch)) != hipSuccess)
            rc = fail(ctx, JDSP_EHIP, "jdsp_fastconv_create: partitions", e);
        if (!rc) rc = jdsp::ensure_stft1024_table_rect(ctx);
        if (!rc) {
            jdsp::HostCall hc(ctx, "jdsp_fastconv_create: partitions");
            const double *d_p = hc.upload(part.data(), rows * 1024 * 16);
            double *d_P = hc.alloc<double>(rows * 1024 * 16);
            if (hc.ok()) hc.result(jdsp_fft_process_f64_dev(ctx, d_p, d_P, 1024, (long)rows, 1));
            if (hc.ok() && jdsp::launch_spectrum_rows_to_f32(ctx->stream, (const double2 *)d_P, h->Hp.get(), (long)rows))
                hc.result(fail(ctx, JDSP_EHIP, "spectrum_rows_to_f32 launch", hipGetLastError()));
            rc = hc.finish();
        }
        if (!rc) h->n_part = P;
    }
    if (!rc) rc = jdsp_fastconv_reset(h);
    if (rc) {
        jdsp_fastconv_destroy(h);
        return rc;
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_fastconv_destroy(jdsp_fastconv *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_fastconv_reset(jdsp_fastconv *h)
{
    if (!h) return JDSP_EINVAL;
    const int hl = h->hist_len > 0 ? h->hist_len : 1;
    for (int i = 0; i < 2; i++) JDSP_HIP(h->ctx, hipMemsetAsync(h->hist[i].get(), 0, (size_t)hl * sizeof(short), h->ctx->stream));
    h->calls = 0;
    h->cur = 0;
    return JDSP_OK;
}

int jdsp_fastconv_set_position(jdsp_fastconv *h, long blocks_consumed)
{
    if (!h || blocks_consumed < 0) return JDSP_EINVAL;
    int rc = jdsp_fastconv_reset(h);                 // history = silence; the caller feeds the halo blocks itself
    if (rc) return rc;
    h->calls = blocks_consumed;
    return JDSP_OK;
}

int jdsp_fastconv_reserve(jdsp_fastconv *h, long n_blocks)
{
    if (!h || n_blocks < 0) return JDSP_EINVAL;
    if (!h->n_part) return JDSP_OK;                  // only the partitioned path has a workspace
    jdsp_ctx *ctx = h->ctx;
    const long samples = n_blocks * h->block;
    if (samples <= h->ws_samples) return JDSP_OK;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h->ws_samples = 0;
    h->staged.reset();
    h->X.reset();
    const long total = 512L * h->n_part + samples;
    JDSP_HIP(ctx, h->staged.alloc((size_t)total));
    JDSP_HIP(ctx, h->X.alloc((size_t)(total / 512) * jdsp::kUpolsRowPitch));
    h->ws_samples = samples;
    return JDSP_OK;
}

int jdsp_fastconv_block_len(const jdsp_fastconv *h) { return h ? h->block : 0; }
int jdsp_fastconv_hist_blocks(const jdsp_fastconv *h) { return h ? h->n_hist : 0; }

long jdsp_fastconv_blocks_out(const jdsp_fastconv *h, long n_blocks)
{
    if (!h || n_blocks < 0) return 0;
    const long first = h->calls >= h->n_hist ? 0 : h->n_hist - h->calls;      // :119-123
    return n_blocks > first ? n_blocks - first : 0;
}

int jdsp_fastconv_process_dev(jdsp_fastconv *h, const int16_t *pcm_dev, long n_blocks, int16_t *out_dev,
                              float *precast_dev, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0) return fail(ctx, JDSP_EINVAL, "jdsp_fastconv_process: n_blocks < 0");
    const long n_out = jdsp_fastconv_blocks_out(h, n_blocks);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (n_blocks == 0) return JDSP_OK;
    if (!pcm_dev || (n_out > 0 && !out_dev)) return fail(ctx, JDSP_EINVAL, "jdsp_fastconv_process: NULL buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    jdsp::ConvStream s;
    s.pcm = pcm_dev;
    s.hist = h->hist[h->cur].get();
    s.n_samples = n_blocks * h->block;
    s.global0 = h->calls * h->block;
    s.valid_from = (long)h->n_hist * h->block;
    s.hist_len = h->hist_len;
    const int first = (int)(n_blocks - n_out);
    if (h->n_part) {
        int rc = jdsp_fastconv_reserve(h, n_blocks);
        if (rc) return rc;
        if (jdsp::launch_fastconv_upols(ctx->stream, s, n_out, first, h->block, h->n_part, h->n_filters, h->Hp.get(),
                                        ctx->stft1024_table_rect.get(), h->staged.get(), h->X.get(), out_dev, precast_dev,
                                        n_out * h->block, h->hist[h->cur ^ 1].get()))
            return fail(ctx, JDSP_EHIP, "fastconv (partitioned) launch", hipGetLastError());
    } else if (jdsp::launch_fastconv(ctx->stream, h->n_fft, s, n_out, first, h->block, h->n_taps, h->n_filters, h->H.get(),
                              ctx->stft1024_table.get(), ctx->conv_tw4096.get(), ctx->conv_tw8192.get(), out_dev,
                              precast_dev, n_out * h->block, h->hist[h->cur ^ 1].get()))
        return fail(ctx, JDSP_EHIP, "fastconv launch", hipGetLastError());
    h->cur ^= 1;
    h->calls += n_blocks;
    return JDSP_OK;
}

int jdsp_fastconv_process(jdsp_fastconv *h, const int16_t *pcm_host, long n_blocks, int16_t *out_host,
                          float *precast_host, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0) return fail(ctx, JDSP_EINVAL, "jdsp_fastconv_process: n_blocks < 0");
    const long n_out = jdsp_fastconv_blocks_out(h, n_blocks);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (n_blocks == 0) return JDSP_OK;
    if (!pcm_host || (n_out > 0 && !out_host)) return fail(ctx, JDSP_EINVAL, "jdsp_fastconv_process: NULL buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t in_b = (size_t)n_blocks * h->block * 2;
    const size_t out_n = (size_t)(n_out > 0 ? n_out : 1) * h->block * h->n_filters;
    jdsp::HostCall hc(ctx, "jdsp_fastconv_process");
    const int16_t *d_in = hc.upload(pcm_host, in_b);
    int16_t *d_out = hc.alloc<int16_t>(out_n * 2);
    float *d_pre = precast_host ? hc.alloc<float>(out_n * 4) : nullptr;
    if (hc.ok()) hc.result(jdsp_fastconv_process_dev(h, d_in, n_blocks, d_out, d_pre, nullptr));
    const size_t got = (size_t)n_out * h->block * h->n_filters;
    hc.download(out_host, d_out, got * 2);
    hc.download(precast_host, d_pre, got * 4);
    return hc.finish();
}

#if JDSP_STAMP
/* diagnostic build only (tools/wave_timeline.py): (start, end, where) of the last convolver launch's first n waves */
int jdsp_debug_wave_stamps(unsigned long long *host, int n) { return jdsp::read_wave_stamps(host, n); }
#endif
}  // extern "C"
