// stftmask_api.hip -- C ABI of the fused STFT masking stream object (include/jdsp.h, jdsp_stftmask_*).
#include "jdsp_internal.h"

using jdsp::fail;

struct jdsp_stftmask {
    jdsp_ctx *ctx = nullptr;
    jdsp_stftmask_cfg cfg;
    jdsp::DevBuf<float> blob;             // wa[n] (w_a / 2), ws[n] (w_s), g[hop], tail[2][n]
    float *wa = nullptr, *ws = nullptr, *g = nullptr, *tail[2] = {nullptr, nullptr};   // views into blob
    int cur = 0;                          // tail[cur] holds the partial sums the next call starts from
    int run_opt = 0;                      // "frames_per_wave": 0 = auto
    // host entry points' device buffers, grown on demand (those entries end with a synchronise: none is in use then)
    jdsp::DevBuf<int16_t> h_pcm, h_i16;
    jdsp::DevBuf<char> h_mask;            // bytes: rows of float or jdsp_c32
    jdsp::DevBuf<float> h_f32;
};

static constexpr int kBins = 513;         // n/2 + 1 of the one supported n_fft

// "stft.window"'s formulas (fill_stft1024_table): PI 3.141592 as the reference writes it
static double window_at(int kind, int i, int n)
{
    if (kind == JDSP_WIN_NONE) return 1.0;
    const double a = kind == JDSP_WIN_HANN ? 0.5 : 0.54, b = kind == JDSP_WIN_HANN ? 0.5 : 0.46;
    return a - b * cos(2 * 3.141592 * i / (n - 1));
}

static bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static size_t mask_elem(const jdsp_stftmask *h) { return h->cfg.mask_kind == JDSP_MASK_COMPLEX ? sizeof(jdsp_c32) : sizeof(float); }

extern "C" {

int jdsp_stftmask_create(jdsp_ctx *ctx, const jdsp_stftmask_cfg *cfg, jdsp_stftmask **out)
{
    if (!ctx || !cfg || !out) return JDSP_EINVAL;
    *out = nullptr;
    const jdsp_stftmask_cfg c = *cfg;
    if (c.n_fft != 1024) return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_create: n_fft must be 1024");
    if (c.hop != 1024 && c.hop != 512 && c.hop != 256)
        return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_create: hop must be n_fft, n_fft/2 or n_fft/4");
    for (int w : {c.analysis_window, c.synthesis_window})
        if (w != JDSP_WIN_NONE && w != JDSP_WIN_HAMMING && w != JDSP_WIN_HANN)
            return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_create: window must be JDSP_WIN_NONE, _HAMMING or _HANN");
    if (c.mask_kind != JDSP_MASK_REAL && c.mask_kind != JDSP_MASK_COMPLEX)
        return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_create: mask_kind must be JDSP_MASK_REAL or JDSP_MASK_COMPLEX");
    if (c.normalise != 0 && c.normalise != 1) return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_create: normalise must be 0 or 1");
    const int n = c.n_fft, hop = c.hop, R = n / hop;
    std::vector<float> host(2 * (size_t)n + hop);
    for (int i = 0; i < n; i++) {
        host[i] = (float)(0.5 * window_at(c.analysis_window, i, n));      // the forward split's 1/2 (frame_io.h)
        host[(size_t)n + i] = (float)window_at(c.synthesis_window, i, n);
    }
    // WOLA: g[i] = 1 / sum_r w_a[i + r hop] w_s[i + r hop] (jdsp_istft_create's rule); 1 without normalisation
    std::vector<double> den((size_t)hop, 1.0);
    if (c.normalise) {
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
                return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_create: the windows' overlap-add vanishes (no WOLA inverse)");
    }
    for (int i = 0; i < hop; i++) host[2 * (size_t)n + i] = (float)(1.0 / den[i]);
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp::ensure_stft1024_table(ctx);          // the transform's twiddles and the split's W^m
    if (rc) return rc;
    jdsp_stftmask *h = new (std::nothrow) jdsp_stftmask();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_stftmask_create");
    h->ctx = ctx;
    h->cfg = c;
    const size_t floats = 2 * (size_t)n + hop + 2 * (size_t)n;
    hipError_t e = h->blob.alloc(floats);
    if (e == hipSuccess) {
        h->wa = h->blob.get();
        h->ws = h->wa + n;
        h->g = h->ws + n;
        h->tail[0] = h->g + hop;
        h->tail[1] = h->tail[0] + n;
        e = hipMemcpy(h->wa, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        jdsp_stftmask_destroy(h);
        return fail(ctx, JDSP_EHIP, "jdsp_stftmask_create: alloc", e);
    }
    rc = jdsp_stftmask_reset(h);
    if (rc) {
        jdsp_stftmask_destroy(h);
        return rc;
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_stftmask_destroy(jdsp_stftmask *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_stftmask_reset(jdsp_stftmask *h)
{
    if (!h) return JDSP_EINVAL;
    JDSP_HIP(h->ctx, hipMemsetAsync(h->tail[0], 0, 2 * (size_t)h->cfg.n_fft * sizeof(float), h->ctx->stream));
    h->cur = 0;
    return JDSP_OK;
}

int jdsp_stftmask_set_option(jdsp_stftmask *h, const char *name, long value)
{
    if (!h || !name) return JDSP_EINVAL;
    if (!strcmp(name, "frames_per_wave")) {
        const long least = h->cfg.n_fft / h->cfg.hop > 1 ? h->cfg.n_fft / h->cfg.hop - 1 : 1;
        if (value < 0 || value > (1L << 30))
            return fail(h->ctx, JDSP_EINVAL, "jdsp_stftmask_set_option: frames_per_wave must be 0 (auto) or positive");
        h->run_opt = (int)(value != 0 && value < least ? least : value);      // clamped to >= max(R - 1, 1)
        return JDSP_OK;
    }
    return fail(h->ctx, JDSP_EINVAL, "jdsp_stftmask_set_option: unknown option");
}

long jdsp_stftmask_samples_out(const jdsp_stftmask *h, long n_frames)
{
    if (!h || n_frames < 0) return 0;
    return n_frames * h->cfg.hop;
}

int jdsp_stftmask_process_dev(jdsp_stftmask *h, const int16_t *pcm_dev, const void *mask_dev, long mask_pitch,
                              long n_frames, int16_t *out_i16_dev, float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_frames < 0) return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_process: n_frames < 0");
    if (mask_pitch != 0 && mask_pitch < kBins)
        return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_process: mask_pitch must be 0 (one row) or >= n_fft/2 + 1");
    if (!aligned(pcm_dev, 4) || !aligned(out_i16_dev, 4) || !aligned(out_f32_dev, 8) || !aligned(mask_dev, mask_elem(h)))
        return fail(ctx, JDSP_EINVAL,
                    "jdsp_stftmask_process: pcm and out_i16 must be 4-byte, out_f32 8-byte aligned, the mask 4-byte "
                    "(REAL) or 8-byte (COMPLEX)");
    if (n_frames == 0) return JDSP_OK;
    if (!pcm_dev || !mask_dev) return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_process: pcm or mask is NULL");
    const int cur = h->cur;
    if (jdsp::launch_stftmask(ctx->stream, ctx->n_cu, h->cfg.hop, h->cfg.mask_kind == JDSP_MASK_COMPLEX, pcm_dev, mask_dev,
                              mask_pitch, n_frames, h->wa, h->ws, h->g, h->tail[cur], h->tail[cur ^ 1], out_i16_dev,
                              out_f32_dev, ctx->stft1024_table.get(), h->run_opt))
        return fail(ctx, JDSP_EHIP, "jdsp_stftmask_process: launch", hipGetLastError());
    h->cur = cur ^ 1;
    return JDSP_OK;
}

int jdsp_stftmask_flush_dev(jdsp_stftmask *h, int16_t *out_i16_dev, float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (!aligned(out_i16_dev, 4) || !aligned(out_f32_dev, 8))
        return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_flush: out_i16 must be 4-byte, out_f32 8-byte aligned");
    // the tail is jdsp_istft's: the same g[t mod hop] * s[t] and the same cast
    if (jdsp::launch_istft_flush(ctx->stream, h->tail[h->cur], h->g, h->cfg.n_fft - h->cfg.hop, h->cfg.hop, out_i16_dev,
                                 out_f32_dev))
        return fail(ctx, JDSP_EHIP, "jdsp_stftmask_flush: launch", hipGetLastError());
    return jdsp_stftmask_reset(h);
}

int jdsp_stftmask_process(jdsp_stftmask *h, const int16_t *pcm_host, const void *mask_host, long mask_pitch, long n_frames,
                          int16_t *out_i16_host, float *out_f32_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_frames < 0 || (mask_pitch != 0 && mask_pitch < kBins))
        return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_process: n_frames < 0, or mask_pitch neither 0 nor >= n_fft/2 + 1");
    if (n_frames == 0) return JDSP_OK;
    if (!pcm_host || !mask_host) return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_process: pcm or mask is NULL");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_pcm = (size_t)(n_frames - 1) * h->cfg.hop + h->cfg.n_fft;
    const size_t mask_bytes = ((size_t)(n_frames - 1) * mask_pitch + kBins) * mask_elem(h);
    const size_t n_out = (size_t)n_frames * h->cfg.hop;
    hipError_t e = h->h_pcm.grow(n_pcm);
    if (e == hipSuccess) e = h->h_mask.grow(mask_bytes);
    if (e == hipSuccess && out_i16_host) e = h->h_i16.grow(n_out);
    if (e == hipSuccess && out_f32_host) e = h->h_f32.grow(n_out);
    if (e != hipSuccess) return fail(ctx, JDSP_EHIP, "jdsp_stftmask_process: buffers", e);
    int16_t *d_i16 = out_i16_host ? h->h_i16.get() : nullptr;
    float *d_f32 = out_f32_host ? h->h_f32.get() : nullptr;
    jdsp::HostCall hc(ctx, "jdsp_stftmask_process");                    // the buffers are the handle's
    hc.upload_to(h->h_pcm.get(), pcm_host, n_pcm * sizeof(int16_t));
    hc.upload_to(h->h_mask.get(), mask_host, mask_bytes);
    if (hc.ok())
        hc.result(jdsp_stftmask_process_dev(h, h->h_pcm.get(), h->h_mask.get(), mask_pitch, n_frames, d_i16, d_f32));
    hc.download(out_i16_host, d_i16, n_out * sizeof(int16_t));
    hc.download(out_f32_host, d_f32, n_out * sizeof(float));
    return hc.finish();
}

int jdsp_stftmask_flush(jdsp_stftmask *h, int16_t *out_i16_host, float *out_f32_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    const size_t n_tail = (size_t)(h->cfg.n_fft - h->cfg.hop);
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipSuccess;
    if (n_tail && out_i16_host) e = h->h_i16.grow(n_tail);
    if (e == hipSuccess && n_tail && out_f32_host) e = h->h_f32.grow(n_tail);
    if (e != hipSuccess) return fail(ctx, JDSP_EHIP, "jdsp_stftmask_flush: buffers", e);
    int16_t *d_i16 = n_tail && out_i16_host ? h->h_i16.get() : nullptr;
    float *d_f32 = n_tail && out_f32_host ? h->h_f32.get() : nullptr;
    jdsp::HostCall hc(ctx, "jdsp_stftmask_flush");
    hc.result(jdsp_stftmask_flush_dev(h, d_i16, d_f32));
    hc.download(out_i16_host, d_i16, n_tail * sizeof(int16_t));
    hc.download(out_f32_host, d_f32, n_tail * sizeof(float));
    return hc.finish();
}

}  // extern "C"
