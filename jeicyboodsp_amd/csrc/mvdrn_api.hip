// mvdrn_api.hip -- C ABI of the generalised (n_mics <= 8, per-bin covariance) MVDR beamformer.
#include "jdsp_internal.h"

using jdsp::fail;

extern "C" {

int jdsp_mvdrn_create(jdsp_ctx *ctx, int n_mics, const double *delays_s, double loading, jdsp_mvdrn **out)
{
    return jdsp_mvdrn_create_cfg(ctx, n_mics, delays_s, loading, 1024, out);
}

int jdsp_mvdrn_block_len(const jdsp_mvdrn *h) { return h ? h->block : 0; }

int jdsp_mvdrn_create_cfg(jdsp_ctx *ctx, int n_mics, const double *delays_s, double loading, int n_fft, jdsp_mvdrn **out)
{
    if (!ctx || !out) return JDSP_EINVAL;
    *out = nullptr;
    if (n_mics < 2 || n_mics > 8 || !(loading >= 0)) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_create: 2 <= n_mics <= 8, loading >= 0");
    if (n_fft != 1024 && n_fft != 512) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_create_cfg: n_fft must be 1024 or 512");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp::ensure_stft1024_table(ctx);
    if (rc) return rc;
    jdsp_mvdrn *h = new (std::nothrow) jdsp_mvdrn();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_mvdrn_create");
    h->ctx = ctx;
    h->n_mics = n_mics;
    h->loading = loading;
    h->n_fft = n_fft;
    h->block = n_fft / 2;
    h->n_bins = n_fft / 2 + 1;
    const int nb = h->n_bins, keep = n_fft / 2 - 1;
    std::vector<double2> steer((size_t)513 * 8, make_double2(0.0, 0.0));
    for (int k = 0; k < nb; k++)
        for (int m = 0; m < n_mics; m++) {
            // the reference's steering phase (BeamForming_MVDR_ver1.cpp:164-165) per microphone delay
            const double ang = 2 * 3.141592 * k * (16000.0 / n_fft) * (delays_s ? delays_s[m] : 0.0);
            steer[(size_t)k * 8 + m] = make_double2(cos(ang), sin(ang));
        }
    double w[512] = {0};
    for (int i = 0; i < h->block; i++) w[i] = (0.54 - 0.46 * cos(2 * 3.141592 * (keep + i) / (n_fft - 1)));   // :217
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = h->cov[i].alloc(513 * 64);
        if (e == hipSuccess) e = h->prev[i].alloc(512 * 8);
        if (e == hipSuccess) e = h->run_len[i].alloc(1);
    }
    if (e == hipSuccess) e = h->plan.alloc(1);
    if (e == hipSuccess) e = h->steer.upload(steer.data(), steer.size());
    if (e == hipSuccess) e = h->w_vad.upload(w, 512);
    if (e != hipSuccess) {
        jdsp_mvdrn_destroy(h);
        return fail(ctx, JDSP_EHIP, "jdsp_mvdrn_create: alloc", e);
    }
    rc = jdsp_mvdrn_reset(h);
    if (rc) {
        jdsp_mvdrn_destroy(h);
        return rc;
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_mvdrn_destroy(jdsp_mvdrn *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_mvdrn_reset(jdsp_mvdrn *h)
{
    if (!h) return JDSP_EINVAL;
    hipStream_t s = h->ctx->stream;
    for (int i = 0; i < 2; i++) {
        JDSP_HIP(h->ctx, hipMemsetAsync(h->cov[i].get(), 0, sizeof(double2) * 513 * 64, s));
        JDSP_HIP(h->ctx, hipMemsetAsync(h->prev[i].get(), 0, sizeof(short) * 512 * 8, s));
        JDSP_HIP(h->ctx, hipMemsetAsync(h->run_len[i].get(), 0, sizeof(int), s));
    }
    h->calls = 0;
    h->cur = 0;
    return JDSP_OK;
}

long jdsp_mvdrn_blocks_out(const jdsp_mvdrn *h, long n_blocks)
{
    if (!h || n_blocks < 0) return 0;
    const long first = h->calls >= 1 ? 0 : 1;
    return n_blocks > first ? n_blocks - first : 0;
}

static int mvdrn_reserve(jdsp_mvdrn *h, long n_blocks)
{
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks <= h->ws.run.cap_blocks) return JDSP_OK;
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    jdsp_mvdrn::Workspace &w = h->ws;
    w = {};                                           // freed before anything is allocated
    const size_t n = (size_t)n_blocks;
    hipError_t e = w.run.reserve(n);
    // worst case: every block is an estimation frame -- one spectrum set and one weight set per block
    if (e == hipSuccess) e = w.spec.alloc(n * h->n_mics * (size_t)h->n_bins);
    if (e == hipSuccess) e = w.weights.alloc((n + 1) * (size_t)h->n_bins * 8);
    // the chunked covariance update's sums and entering matrices: a call of n blocks has at most min(n, kMvnChunks) chunks
    // (1 KB per bin and chunk: 134 MB at 128 chunks of 513 bins -- a per-block caller gets 1 MB)
    const int chunk_cap = (int)(n < (size_t)jdsp::kMvnChunks ? n : (size_t)jdsp::kMvnChunks);
    if (e == hipSuccess) e = w.chunk_ws.alloc(2 * (size_t)chunk_cap * (size_t)h->n_bins * 64);
    if (e != hipSuccess) {
        w = {};
        return fail(ctx, JDSP_ENOMEM, "jdsp_mvdrn: workspace", e);
    }
    w.chunk_cap = chunk_cap;
    return JDSP_OK;
}

int jdsp_mvdrn_process_dev(jdsp_mvdrn *h, const int16_t *pcm_dev, long chan_stride, long n_blocks, int16_t *out_dev,
                           float *precast_dev, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0 || chan_stride < n_blocks * h->block) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_process: bad sizes");
    const long n_out = jdsp_mvdrn_blocks_out(h, n_blocks);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (n_blocks == 0) return JDSP_OK;
    if (!pcm_dev || (n_out > 0 && !out_dev)) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_process: NULL buffer");
    if (((uintptr_t)pcm_dev & 15u) || (chan_stride & 7))
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_process: pcm must be 16-byte aligned and chan_stride a multiple of 8");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = mvdrn_reserve(h, n_blocks);
    if (rc) return rc;
    const int in = h->cur, ou = h->cur ^ 1;
    hipStream_t s = ctx->stream;
    const jdsp_mvdrn::Workspace &w = h->ws;
    const jdsp::RunPlanWs &r = w.run;
    const bool half = h->n_fft == 512;
    if (jdsp::launch_vad(s, h->block, pcm_dev, n_blocks, h->w_vad.get(), 0, r.flags.get(), nullptr, nullptr) ||
        jdsp::launch_run_plan(s, r.flags.get(), n_blocks, h->run_len[in].get(), h->run_len[ou].get(), 0, r.ver_base.get(),
                              r.snap_mask.get(), r.events.get(), r.ev_n.get(), h->plan.get()) ||
        (half ? jdsp::launch_mvdrn512 : jdsp::launch_mvdrn)(
            s, pcm_dev, chan_stride, h->n_mics, n_blocks, h->calls, h->prev[in].get(), h->prev[ou].get(), r.events.get(),
            h->plan.get(), r.ver_base.get(), r.snap_mask.get(), w.spec.get(), h->cov[in].get(), h->cov[ou].get(),
            h->steer.get(), h->loading, w.weights.get(), ctx->stft1024_table.get(), out_dev, precast_dev, w.chunk_ws.get(),
            w.chunk_cap))
        return fail(ctx, JDSP_EHIP, half ? "mvdrn512 launch" : "mvdrn launch", hipGetLastError());
    h->cur ^= 1;
    h->calls += n_blocks;
    return JDSP_OK;
}

int jdsp_mvdrn_process(jdsp_mvdrn *h, const int16_t *pcm_host, long chan_stride, long n_blocks, int16_t *out_host,
                       float *precast_host, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0 || chan_stride < n_blocks * h->block) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_process: bad sizes");
    const long n_out = jdsp_mvdrn_blocks_out(h, n_blocks);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (n_blocks == 0) return JDSP_OK;
    if (!pcm_host || (n_out > 0 && !out_host)) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_process: NULL buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const long stride_dev = n_blocks * h->block;               // repack the planes tightly (a multiple of 8)
    const size_t in_b = (size_t)stride_dev * h->n_mics * 2, out_b = (size_t)(n_out > 0 ? n_out : 1) * h->block * 2;
    jdsp::HostCall hc(ctx, "jdsp_mvdrn_process");
    int16_t *d_in = hc.alloc<int16_t>(in_b);
    int16_t *d_out = hc.alloc<int16_t>(out_b);
    float *d_pre = precast_host ? hc.alloc<float>(out_b * 2) : nullptr;
    for (int m = 0; m < h->n_mics; m++)
        hc.upload_to(d_in + (size_t)m * stride_dev, pcm_host + (size_t)m * chan_stride, (size_t)stride_dev * 2);
    if (hc.ok()) hc.result(jdsp_mvdrn_process_dev(h, d_in, stride_dev, n_blocks, d_out, d_pre, nullptr));
    hc.download(out_host, d_out, (size_t)n_out * h->block * 2);
    hc.download(precast_host, d_pre, (size_t)n_out * h->block * 4);
    return hc.finish();
}

}  // extern "C"
