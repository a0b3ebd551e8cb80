// timedomain_api.hip -- C ABI of the time-domain pitch (AMDF, autocorrelation) and LPC entries (include/jdsp.h).
#include "jdsp_internal.h"

using jdsp::fail;

namespace {

// Hamming(2 block_len) of LPCEstimation.cpp:105 in FP64, made on the host once per context and frame length
int ensure_lpc_window(jdsp_ctx *ctx, int block_len, const double **w_out)
{
    const int bi = block_len == 256 ? 0 : 1, n = 2 * block_len;
    const int rc = jdsp::ensure_table(ctx, ctx->lpc_win[bi], (size_t)n, [n](double *w) {
        for (int i = 0; i < n; i++) w[i] = (double)(0.54 - 0.46 * cos(2 * 3.141592 * i / (double)(n - 1)));
    });
    *w_out = ctx->lpc_win[bi].get();
    return rc;
}

}  // namespace

extern "C" {

/* ---- PitchEstimation_method2 / _method3 ------------------------------------------------- */
int jdsp_pitch_lag_dev(jdsp_ctx *ctx, int method, const int16_t *pcm_dev, long n_blocks, const int16_t *prev_block_dev,
                       int32_t *arg_dev, double *value_dev, double *curve_dev)
{
    if (!ctx) return JDSP_EINVAL;
    if (method != JDSP_PITCH_AMDF && method != JDSP_PITCH_ACF)
        return fail(ctx, JDSP_EINVAL, "jdsp_pitch_lag: method must be JDSP_PITCH_AMDF (2) or JDSP_PITCH_ACF (3)");
    if (n_blocks < 0 || (n_blocks > 0 && !pcm_dev)) return fail(ctx, JDSP_EINVAL, "jdsp_pitch_lag: bad buffer");
    if (n_blocks == 0) return JDSP_OK;
    if (((uintptr_t)pcm_dev & 15u) || ((uintptr_t)prev_block_dev & 15u) || ((uintptr_t)curve_dev & 15u))
        return fail(ctx, JDSP_EINVAL, "jdsp_pitch_lag: pcm, prev_block and curve must be 16-byte aligned");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (jdsp::launch_pitch_lag(ctx->stream, method, pcm_dev, n_blocks, prev_block_dev, arg_dev, value_dev, curve_dev))
        return fail(ctx, JDSP_EHIP, "pitch_lag launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_pitch_lag(jdsp_ctx *ctx, int method, const int16_t *pcm_host, long n_blocks, const int16_t *prev_block_host,
                   int32_t *arg_host, double *value_host, double *curve_host)
{
    if (!ctx) return JDSP_EINVAL;
    if (method != JDSP_PITCH_AMDF && method != JDSP_PITCH_ACF)
        return fail(ctx, JDSP_EINVAL, "jdsp_pitch_lag: method must be JDSP_PITCH_AMDF (2) or JDSP_PITCH_ACF (3)");
    if (n_blocks < 0 || (n_blocks > 0 && !pcm_host)) return fail(ctx, JDSP_EINVAL, "jdsp_pitch_lag: bad buffer");
    if (n_blocks == 0) return JDSP_OK;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)n_blocks;
    jdsp::HostCall hc(ctx, "jdsp_pitch_lag");
    const int16_t *d_in = hc.upload(pcm_host, n * 1024);
    const int16_t *d_prev = prev_block_host ? hc.upload(prev_block_host, 1024) : nullptr;
    int32_t *d_arg = arg_host ? hc.alloc<int32_t>(n * 4) : nullptr;
    double *d_val = value_host ? hc.alloc<double>(n * 8) : nullptr;
    double *d_cv = curve_host ? hc.alloc<double>(n * 4096) : nullptr;
    if (hc.ok()) hc.result(jdsp_pitch_lag_dev(ctx, method, d_in, n_blocks, d_prev, d_arg, d_val, d_cv));
    hc.download(arg_host, d_arg, n * 4);
    hc.download(value_host, d_val, n * 8);
    hc.download(curve_host, d_cv, n * 4096);
    return hc.finish();
}

/* ---- LPCEstimation ------------------------------------------------------------------------ */
static int lpc_args(jdsp_ctx *ctx, const void *pcm, long n_blocks, int block_len, int order, const void *lpc)
{
    if ((block_len != 256 && block_len != 512) || order < 1 || order > 16)
        return fail(ctx, JDSP_EINVAL, "jdsp_lpc: block_len 256 | 512, order 1 .. 16");
    if (n_blocks < 0 || (n_blocks > 0 && (!pcm || !lpc))) return fail(ctx, JDSP_EINVAL, "jdsp_lpc: bad buffer");
    return JDSP_OK;
}

int jdsp_lpc_dev(jdsp_ctx *ctx, const int16_t *pcm_dev, long n_blocks, int block_len, int order,
                 const int16_t *prev_block_dev, double *autocorr_dev, double *lpc_dev)
{
    if (!ctx) return JDSP_EINVAL;
    int rc = lpc_args(ctx, pcm_dev, n_blocks, block_len, order, lpc_dev);
    if (rc || n_blocks == 0) return rc;
    if (((uintptr_t)pcm_dev & 15u) || ((uintptr_t)prev_block_dev & 15u))
        return fail(ctx, JDSP_EINVAL, "jdsp_lpc: pcm and prev_block must be 16-byte aligned");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const double *win = nullptr;
    if ((rc = ensure_lpc_window(ctx, block_len, &win))) return rc;
    if (jdsp::launch_lpc(ctx->stream, pcm_dev, n_blocks, block_len, order, prev_block_dev, win, autocorr_dev, lpc_dev))
        return fail(ctx, JDSP_EHIP, "lpc launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_lpc(jdsp_ctx *ctx, const int16_t *pcm_host, long n_blocks, int block_len, int order,
             const int16_t *prev_block_host, double *autocorr_host, double *lpc_host)
{
    if (!ctx) return JDSP_EINVAL;
    int rc = lpc_args(ctx, pcm_host, n_blocks, block_len, order, lpc_host);
    if (rc || n_blocks == 0) return rc;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)n_blocks, blk_b = (size_t)block_len * 2, ac_b = n * (size_t)(order + 1) * 8, lpc_b = n * (size_t)order * 8;
    jdsp::HostCall hc(ctx, "jdsp_lpc");
    const int16_t *d_in = hc.upload(pcm_host, n * blk_b);
    const int16_t *d_prev = prev_block_host ? hc.upload(prev_block_host, blk_b) : nullptr;
    double *d_ac = autocorr_host ? hc.alloc<double>(ac_b) : nullptr;
    double *d_lpc = hc.alloc<double>(lpc_b);
    if (hc.ok()) hc.result(jdsp_lpc_dev(ctx, d_in, n_blocks, block_len, order, d_prev, d_ac, d_lpc));
    hc.download(autocorr_host, d_ac, ac_b);
    hc.download(lpc_host, d_lpc, lpc_b);
    return hc.finish();
}

}  // extern "C"
