// istft_api.hip -- C ABI of the STFT synthesis stream object (include/jdsp.h, jdsp_istft_*).
#include "jdsp_internal.h"

using jdsp::fail;

struct jdsp_istft {
    jdsp_ctx *ctx = nullptr;
    jdsp_istft_cfg cfg;
    jdsp::DevBuf<float> blob;             // ws[n_fft] (w_s / n_fft), g[hop], tail[2][n_fft]
    float *ws = nullptr, *g = nullptr, *tail[2] = {nullptr, nullptr};   // views into blob
    int cur = 0;                          // tail[cur] holds the partial sums the next call starts from
    int run_opt = 0;                      // "frames_per_wave": 0 = auto
    // host entry points' device buffers, grown on demand (those entries end with a synchronise: none is in use then)
    jdsp::DevBuf<jdsp_c32> h_spec;
    jdsp::DevBuf<int16_t> h_i16;
    jdsp::DevBuf<float> h_f32;
};

static int bins_of(const jdsp_istft_cfg &c) { return c.layout == JDSP_SPEC_HALF ? c.n_fft / 2 + 1 : c.n_fft; }

// "stft.window"'s formulas (fill_stft1024_table / fill_win512): PI 3.141592 as the reference writes it
static double window_at(int kind, int i, int n)
{
    if (kind == JDSP_WIN_NONE) return 1.0;
    const double a = kind == JDSP_WIN_HANN ? 0.5 : 0.54, b = kind == JDSP_WIN_HANN ? 0.5 : 0.46;
    return a - b * cos(2 * 3.141592 * i / (n - 1));
}

static bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" {

int jdsp_istft_create(jdsp_ctx *ctx, const jdsp_istft_cfg *cfg, jdsp_istft **out)
{
    if (!ctx || !cfg || !out) return JDSP_EINVAL;
    *out = nullptr;
    const jdsp_istft_cfg c = *cfg;
    if (c.n_fft != 1024 && c.n_fft != 512) return fail(ctx, JDSP_EINVAL, "jdsp_istft_create: n_fft must be 1024 or 512");
    if (c.hop != c.n_fft && c.hop != c.n_fft / 2 && c.hop != c.n_fft / 4)
        return fail(ctx, JDSP_EINVAL, "jdsp_istft_create: hop must be n_fft, n_fft/2 or n_fft/4");
    if (c.layout != JDSP_SPEC_FULL && c.layout != JDSP_SPEC_HALF) return fail(ctx, JDSP_EINVAL, "jdsp_istft_create: layout");
    for (int w : {c.synthesis_window, c.analysis_window})
        if (w != JDSP_WIN_NONE && w != JDSP_WIN_HAMMING && w != JDSP_WIN_HANN)
            return fail(ctx, JDSP_EINVAL, "jdsp_istft_create: window must be JDSP_WIN_NONE, _HAMMING or _HANN");
    const int n = c.n_fft, hop = c.hop, R = n / hop;
    std::vector<float> host((size_t)n + hop);
    for (int i = 0; i < n; i++) host[i] = (float)(window_at(c.synthesis_window, i, n) / n);
    // WOLA: g[i] = 1 / sum_r w_a[i + r hop] w_s[i + r hop]; 1 without an analysis window
    std::vector<double> den((size_t)hop, 1.0);
    if (c.analysis_window != JDSP_WIN_NONE) {
        double mx = 0;
        for (int i = 0; i < hop; i++) {
            double s = 0;
            for (int r = 0; r < R; r++)
                s += window_at(c.analysis_window, i + r * hop, n) * window_at(c.synthesis_window, i + r * hop, n);
            den[i] = s;
            mx = s > mx ? s : mx;
        }
        for (int i = 0; i < hop; i++)
            if (!(den[i] >= 1e-6 * mx))
                return fail(ctx, JDSP_EINVAL, "jdsp_istft_create: the windows' overlap-add vanishes (no WOLA inverse)");
    }
    for (int i = 0; i < hop; i++) host[(size_t)n + i] = (float)(1.0 / den[i]);
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp::ensure_stft1024_table(ctx);          // the transform's twiddles and the split's W^m
    if (rc) return rc;
    jdsp_istft *h = new (std::nothrow) jdsp_istft();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_istft_create");
    h->ctx = ctx;
    h->cfg = c;
    const size_t floats = (size_t)n + hop + 2 * (size_t)n;
    hipError_t e = h->blob.alloc(floats);
    if (e == hipSuccess) {
        h->ws = h->blob.get();
        h->g = h->ws + n;
        h->tail[0] = h->g + hop;
        h->tail[1] = h->tail[0] + n;
        e = hipMemcpy(h->ws, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        jdsp_istft_destroy(h);
        return fail(ctx, JDSP_EHIP, "jdsp_istft_create: alloc", e);
    }
    rc = jdsp_istft_reset(h);
    if (rc) {
        jdsp_istft_destroy(h);
        return rc;
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_istft_destroy(jdsp_istft *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_istft_reset(jdsp_istft *h)
{
    if (!h) return JDSP_EINVAL;
    JDSP_HIP(h->ctx, hipMemsetAsync(h->tail[0], 0, 2 * (size_t)h->cfg.n_fft * sizeof(float), h->ctx->stream));
    h->cur = 0;
    return JDSP_OK;
}

int jdsp_istft_set_option(jdsp_istft *h, const char *name, long value)
{
    if (!h || !name) return JDSP_EINVAL;
    if (!strcmp(name, "frames_per_wave")) {
        const long least = h->cfg.n_fft / h->cfg.hop > 1 ? h->cfg.n_fft / h->cfg.hop - 1 : 1;
        if (value != 0 && (value < least || value > (1L << 30)))
            return fail(h->ctx, JDSP_EINVAL, "jdsp_istft_set_option: frames_per_wave must be 0 (auto) or >= max(R - 1, 1)");
        h->run_opt = (int)value;
        return JDSP_OK;
    }
    return fail(h->ctx, JDSP_EINVAL, "jdsp_istft_set_option: unknown option");
}

long jdsp_istft_samples_out(const jdsp_istft *h, long n_frames)
{
    if (!h || n_frames < 0) return 0;
    return n_frames * h->cfg.hop;
}

int jdsp_istft_process_dev(jdsp_istft *h, const jdsp_c32 *spec_dev, long row_pitch, long n_frames, int16_t *out_i16_dev,
                           float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_frames < 0) return fail(ctx, JDSP_EINVAL, "jdsp_istft_process: n_frames < 0");
    if (row_pitch < bins_of(h->cfg)) return fail(ctx, JDSP_EINVAL, "jdsp_istft_process: row_pitch below the layout's bins");
    if (!aligned(spec_dev, 8) || !aligned(out_i16_dev, 4) || !aligned(out_f32_dev, 8))
        return fail(ctx, JDSP_EINVAL, "jdsp_istft_process: spec must be 8-byte, out_i16 4-byte, out_f32 8-byte aligned");
    if (n_frames == 0) return JDSP_OK;
    if (!spec_dev) return fail(ctx, JDSP_EINVAL, "jdsp_istft_process: spec is NULL");
    const int cur = h->cur;
    if (jdsp::launch_istft(ctx->stream, ctx->n_cu, h->cfg.n_fft, h->cfg.hop, h->cfg.layout == JDSP_SPEC_HALF,
                           reinterpret_cast<const float2 *>(spec_dev), row_pitch, n_frames, h->ws, h->g, h->tail[cur],
                           h->tail[cur ^ 1], out_i16_dev, out_f32_dev, ctx->stft1024_table.get(), h->run_opt))
        return fail(ctx, JDSP_EHIP, "jdsp_istft_process: launch", hipGetLastError());
    h->cur = cur ^ 1;
    return JDSP_OK;
}

int jdsp_istft_flush_dev(jdsp_istft *h, int16_t *out_i16_dev, float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (!aligned(out_i16_dev, 4) || !aligned(out_f32_dev, 8))
        return fail(ctx, JDSP_EINVAL, "jdsp_istft_flush: out_i16 must be 4-byte, out_f32 8-byte aligned");
    if (jdsp::launch_istft_flush(ctx->stream, h->tail[h->cur], h->g, h->cfg.n_fft - h->cfg.hop, h->cfg.hop, out_i16_dev,
                                 out_f32_dev))
        return fail(ctx, JDSP_EHIP, "jdsp_istft_flush: launch", hipGetLastError());
    return jdsp_istft_reset(h);
}

int jdsp_istft_process(jdsp_istft *h, const jdsp_c32 *spec_host, long row_pitch, long n_frames, int16_t *out_i16_host,
                       float *out_f32_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_frames < 0 || row_pitch < bins_of(h->cfg))
        return fail(ctx, JDSP_EINVAL, "jdsp_istft_process: n_frames < 0 or row_pitch below the layout's bins");
    if (n_frames == 0) return JDSP_OK;
    if (!spec_host) return fail(ctx, JDSP_EINVAL, "jdsp_istft_process: spec is NULL");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_in = (size_t)(n_frames - 1) * row_pitch + bins_of(h->cfg);
    const size_t n_out = (size_t)n_frames * h->cfg.hop;
    hipError_t e = h->h_spec.grow(n_in);
    if (e == hipSuccess && out_i16_host) e = h->h_i16.grow(n_out);
    if (e == hipSuccess && out_f32_host) e = h->h_f32.grow(n_out);
    if (e != hipSuccess) return fail(ctx, JDSP_EHIP, "jdsp_istft_process: buffers", e);
    int16_t *d_i16 = out_i16_host ? h->h_i16.get() : nullptr;
    float *d_f32 = out_f32_host ? h->h_f32.get() : nullptr;
    jdsp::HostCall hc(ctx, "jdsp_istft_process");                       // the buffers are the handle's
    hc.upload_to(h->h_spec.get(), spec_host, n_in * sizeof(jdsp_c32));
    if (hc.ok()) hc.result(jdsp_istft_process_dev(h, h->h_spec.get(), row_pitch, n_frames, d_i16, d_f32));
    hc.download(out_i16_host, d_i16, n_out * sizeof(int16_t));
    hc.download(out_f32_host, d_f32, n_out * sizeof(float));
    return hc.finish();
}

int jdsp_istft_flush(jdsp_istft *h, int16_t *out_i16_host, float *out_f32_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    const size_t n_tail = (size_t)(h->cfg.n_fft - h->cfg.hop);
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipSuccess;
    if (n_tail && out_i16_host) e = h->h_i16.grow(n_tail);
    if (e == hipSuccess && n_tail && out_f32_host) e = h->h_f32.grow(n_tail);
    if (e != hipSuccess) return fail(ctx, JDSP_EHIP, "jdsp_istft_flush: buffers", e);
    int16_t *d_i16 = n_tail && out_i16_host ? h->h_i16.get() : nullptr;
    float *d_f32 = n_tail && out_f32_host ? h->h_f32.get() : nullptr;
    jdsp::HostCall hc(ctx, "jdsp_istft_flush");
    hc.result(jdsp_istft_flush_dev(h, d_i16, d_f32));
    hc.download(out_i16_host, d_i16, n_tail * sizeof(int16_t));
    hc.download(out_f32_host, d_f32, n_tail * sizeof(float));
    return hc.finish();
}

}  // extern "C"
