// mvdr_api.hip -- C ABI of the two-microphone MVDR beamformer (BeamForming_MVDR_ver1.cpp).
#include "jdsp_internal.h"

using jdsp::fail;

extern "C" {

int jdsp_mvdr_create(jdsp_ctx *ctx, double d_time, jdsp_mvdr **out)
{
    if (!ctx || !out) return JDSP_EINVAL;
    *out = nullptr;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp::ensure_stft1024_table(ctx);
    if (rc) return rc;
    jdsp_mvdr *h = new (std::nothrow) jdsp_mvdr();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_mvdr_create");
    h->ctx = ctx;
    h->d_time = d_time;
    std::vector<double2> steer(1024);
    for (int i = 0; i < 1024; i++) {                                           // :164-165
        const double ang = 2 * 3.141592 * i * (16000.0 / 1024) * d_time;
        steer[i] = make_double2(cos(ang), sin(ang));
    }
    double w[512];
    for (int i = 0; i < 512; i++) w[i] = (0.54 - 0.46 * cos(2 * 3.141592 * (511 + i) / (1024 - 1)));   // :217, frame offset 511
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = h->st[i].alloc(1);
    if (e == hipSuccess) e = h->plan.alloc(1);
    if (e == hipSuccess) e = h->sh_range.alloc(4);
    if (e == hipSuccess) e = h->sh_zero_run.alloc(1);
    if (e == hipSuccess) e = hipMemset(h->sh_zero_run.get(), 0, sizeof(int));
    if (e == hipSuccess) e = h->steer.upload(steer.data(), 1024);
    if (e == hipSuccess) e = h->w_vad.upload(w, 512);
    if (e != hipSuccess) {
        jdsp_mvdr_destroy(h);
        return fail(ctx, JDSP_EHIP, "jdsp_mvdr_create: alloc", e);
    }
    rc = jdsp_mvdr_reset(h);
    if (rc) {
        jdsp_mvdr_destroy(h);
        return rc;
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_mvdr_destroy(jdsp_mvdr *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_mvdr_reset(jdsp_mvdr *h)
{
    if (!h) return JDSP_EINVAL;
    for (int i = 0; i < 2; i++) JDSP_HIP(h->ctx, hipMemsetAsync(h->st[i].get(), 0, sizeof(jdsp::MvdrState), h->ctx->stream));
    h->calls = 0;
    h->cur = 0;
    return JDSP_OK;
}

long jdsp_mvdr_blocks_out(const jdsp_mvdr *h, long n_blocks)
{
    if (!h || n_blocks < 0) return 0;
    const long first = h->calls >= 1 ? 0 : 1;                                  // :201-204
    return n_blocks > first ? n_blocks - first : 0;
}

static int mvdr_reserve(jdsp_mvdr *h, long n_blocks)
{
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks <= h->ws.run.cap_blocks) return JDSP_OK;
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    jdsp_mvdr::Workspace &w = h->ws;
    w = {};                                           // freed before anything is allocated
    const size_t n = (size_t)n_blocks;
    hipError_t e = w.run.reserve(n);
    if (e == hipSuccess) e = w.delta.alloc(n * 4);
    if (e == hipSuccess) e = w.rver.alloc((n + 1) * 4);
    if (e == hipSuccess) e = w.tile_sums.alloc((n / 1024 + 1) * 4);
    // a call has at most as many events as blocks: the weight table needs no more rows than that
    const size_t wrows = n + 1 < (size_t)jdsp::kMvdrTableVersions ? n + 1 : (size_t)jdsp::kMvdrTableVersions;
    if (e == hipSuccess) e = w.wtab.alloc(wrows * 1024);
    if (e != hipSuccess) {
        w = {};
        return fail(ctx, JDSP_ENOMEM, "jdsp_mvdr: workspace", e);
    }
    return JDSP_OK;
}

int jdsp_mvdr_process_dev(jdsp_mvdr *h, const int16_t *left_dev, const int16_t *right_dev, long n_blocks,
                          int16_t *out_dev, float *precast_dev, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0) return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_process: n_blocks < 0");
    const long n_out = jdsp_mvdr_blocks_out(h, n_blocks);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (n_blocks == 0) return JDSP_OK;
    if (!left_dev || !right_dev || (n_out > 0 && !out_dev)) return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_process: NULL buffer");
    if (((uintptr_t)left_dev & 15u) || ((uintptr_t)right_dev & 15u))
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_process: inputs must be 16-byte aligned");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = mvdr_reserve(h, n_blocks);
    if (rc) return rc;
    const jdsp::MvdrState *st_in = h->st[h->cur].get();
    jdsp::MvdrState *st_out = h->st[h->cur ^ 1].get();
    hipStream_t s = ctx->stream;
    const jdsp_mvdr::Workspace &w = h->ws;
    const jdsp::RunPlanWs &r = w.run;
    if (jdsp::launch_vad(s, 512, left_dev, n_blocks, h->w_vad.get(), 0, r.flags.get(), nullptr, nullptr) ||
        jdsp::launch_run_plan(s, r.flags.get(), n_blocks, &st_in->run_len, &st_out->run_len, 0, r.ver_base.get(),
                              r.snap_mask.get(), r.events.get(), r.ev_n.get(), h->plan.get()) ||
        jdsp::launch_mvdr(s, left_dev, right_dev, n_blocks, h->calls, st_in, st_out, r.events.get(), h->plan.get(),
                          r.ver_base.get(), r.snap_mask.get(), w.delta.get(), w.rver.get(), h->steer.get(),
                          ctx->stft1024_table.get(), out_dev, precast_dev, w.wtab.get(), w.tile_sums.get()))
        return fail(ctx, JDSP_EHIP, "mvdr launch", hipGetLastError());
    h->cur ^= 1;
    h->calls += n_blocks;
    return JDSP_OK;
}

int jdsp_mvdr_process(jdsp_mvdr *h, const int16_t *left_host, const int16_t *right_host, long n_blocks,
                      int16_t *out_host, float *precast_host, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0) return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_process: n_blocks < 0");
    const long n_out = jdsp_mvdr_blocks_out(h, n_blocks);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (n_blocks == 0) return JDSP_OK;
    if (!left_host || !right_host || (n_out > 0 && !out_host)) return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_process: NULL buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t in_b = (size_t)n_blocks * 1024, out_b = (size_t)(n_out > 0 ? n_out : 1) * 1024;
    jdsp::HostCall hc(ctx, "jdsp_mvdr_process");
    const int16_t *d_l = hc.upload(left_host, in_b);
    const int16_t *d_r = hc.upload(right_host, in_b);
    int16_t *d_out = hc.alloc<int16_t>(out_b);
    float *d_pre = precast_host ? hc.alloc<float>(out_b * 2) : nullptr;
    if (hc.ok()) hc.result(jdsp_mvdr_process_dev(h, d_l, d_r, n_blocks, d_out, d_pre, nullptr));
    hc.download(out_host, d_out, (size_t)n_out * 1024);
    hc.download(precast_host, d_pre, (size_t)n_out * 2048);
    return hc.finish();
}

/* ---- multi-GPU: one rank's share of one stereo stream ------------------------------------------ */
int jdsp_mvdr_shard_vad_dev(jdsp_mvdr *h, const int16_t *left_ext_dev, const int16_t *right_ext_dev, long ext0, long b0,
                            long b1, long n_total, uint8_t *flags_own_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (!(0 <= ext0 && ext0 <= b0 && b0 <= b1 && b1 <= n_total) || (b0 >= 1 ? ext0 != b0 - 1 : ext0 != 0))
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_shard_vad: need ext0 = max(b0-1, 0) <= b0 <= b1 <= n_total");
    if (b1 > b0 && (!left_ext_dev || !right_ext_dev || !flags_own_dev)) return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_shard_vad: NULL buffer");
    if (((uintptr_t)left_ext_dev & 15u) || ((uintptr_t)right_ext_dev & 15u))
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_shard_vad: inputs must be 16-byte aligned");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = mvdr_reserve(h, n_total);
    if (!rc) rc = jdsp_mvdr_reset(h);
    if (rc) return rc;
    h->sh_ext0 = ext0; h->sh_b0 = b0; h->sh_b1 = b1; h->sh_total = n_total;
    h->sh_left = left_ext_dev; h->sh_right = right_ext_dev;
    if (jdsp::launch_vad(ctx->stream, 512, left_ext_dev + (b0 - ext0) * 512, b1 - b0, h->w_vad.get(), 0, flags_own_dev, nullptr, nullptr))
        return fail(ctx, JDSP_EHIP, "vad launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_mvdr_shard_summary_dev(jdsp_mvdr *h, const uint8_t *flags_all_dev, double *sum4_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (!flags_all_dev || !sum4_dev) return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_shard_summary: NULL buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const jdsp::RunPlanWs &r = h->ws.run;
    if (jdsp::launch_run_plan(s, flags_all_dev, h->sh_total, h->sh_zero_run.get(), nullptr, 0, r.ver_base.get(),
                              r.snap_mask.get(), r.events.get(), r.ev_n.get(), h->plan.get()) ||
        jdsp::launch_mvdr_shard_summary(s, h->sh_left, h->sh_right, h->sh_b1 - h->sh_ext0, h->sh_ext0, h->sh_b0, h->sh_b1,
                                        h->st[h->cur].get(), r.events.get(), h->plan.get(), r.ver_base.get(),
                                        r.snap_mask.get(), ctx->stft1024_table.get(), h->sh_range.get(), h->ws.delta.get(),
                                        sum4_dev, h->ws.tile_sums.get()))
        return fail(ctx, JDSP_EHIP, "mvdr shard summary launch", hipGetLastError());
    return JDSP_OK;
}

long jdsp_mvdr_shard_blocks_out(const jdsp_mvdr *h)
{
    if (!h) return 0;
    const long lo = h->sh_b0 > 1 ? h->sh_b0 : 1;
    return h->sh_b1 > lo ? h->sh_b1 - lo : 0;
}

int jdsp_mvdr_shard_finish_dev(jdsp_mvdr *h, const double *sums_all_dev, int world, int rank, int16_t *out_dev,
                               float *precast_dev, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    const long n_out = jdsp_mvdr_shard_blocks_out(h);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (!sums_all_dev || world < 1 || rank < 0 || rank >= world || (n_out > 0 && !out_dev))
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_shard_finish: bad argument");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (jdsp::launch_mvdr_shard_finish(ctx->stream, h->sh_left, h->sh_right, h->sh_b1 - h->sh_ext0, h->sh_ext0, h->sh_b0,
                                       h->sh_b1, h->st[h->cur].get(), h->st[h->cur ^ 1].get(), h->plan.get(),
                                       h->ws.run.ver_base.get(), h->ws.run.snap_mask.get(), h->sh_range.get(),
                                       h->ws.delta.get(), sums_all_dev, rank, h->ws.rver.get(), h->steer.get(),
                                       ctx->stft1024_table.get(), out_dev, precast_dev, h->ws.tile_sums.get()))
        return fail(ctx, JDSP_EHIP, "mvdr shard finish launch", hipGetLastError());
    return JDSP_OK;
}

/* ---- the program's two helper functions on their own (compat: EstimateSpatialCorrMtx, ProcessMVDR) ---------- */
int jdsp_mvdr_estimate_corr(jdsp_mvdr *h, const int16_t *left_frames_host, const int16_t *right_frames_host, long n_frames,
                            double *corr4_inout_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_frames < 0 || n_frames > (1L << 28)) return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_estimate_corr: n_frames");
    if (n_frames == 0) return JDSP_OK;
    if (!left_frames_host || !right_frames_host || !corr4_inout_host) return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_estimate_corr: NULL buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = mvdr_reserve(h, 2 * n_frames);
    if (rc) return rc;
    // frame i = blocks (2i, 2i+1) of a 2 n_frames-block stream; "event" i = block 2i+1 with its predecessor (:250-253)
    std::vector<int> ev((size_t)n_frames);
    for (long i = 0; i < n_frames; i++) ev[(size_t)i] = (int)(2 * i + 1);
    const jdsp::DenoisePlan plan = {(int)n_frames, 0, 0, 0};
    const size_t in_b = (size_t)n_frames * 2048;
    hipStream_t s = ctx->stream;
    jdsp::HostCall hc(ctx, "jdsp_mvdr_estimate_corr");
    const int16_t *d_l = hc.upload(left_frames_host, in_b);
    const int16_t *d_r = hc.upload(right_frames_host, in_b);
    double *d_tot = hc.alloc<double>(4 * sizeof(double));
    hc.upload_to(h->ws.run.events.get(), ev.data(), sizeof(int) * (size_t)n_frames);
    hc.upload_to(h->plan.get(), &plan, sizeof(plan));
    double tot[4] = {0, 0, 0, 0};
    if (hc.ok() && jdsp::launch_mvdr_corr_total(s, d_l, d_r, 2 * n_frames, h->st[h->cur].get(), h->ws.run.events.get(),
                                                h->plan.get(), ctx->stft1024_table.get(), h->ws.delta.get(), d_tot,
                                                h->ws.tile_sums.get()))
        hc.result(fail(ctx, JDSP_EHIP, "mvdr corr launch", hipGetLastError()));
    hc.download(tot, d_tot, sizeof(tot));
    rc = hc.finish();
    if (!rc)
        for (int c = 0; c < 4; c++) corr4_inout_host[c] += tot[c];               // rgdSpatialCorr[..] += (:263-268)
    return rc;
}

int jdsp_mvdr_apply(jdsp_mvdr *h, const int16_t *left_host, const int16_t *right_host, long n_blocks,
                    const double *corr4_host, int16_t *out_host, float *precast_host, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0 || !corr4_host) return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_apply: bad argument");
    const long n_out = jdsp_mvdr_blocks_out(h, n_blocks);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (n_blocks == 0) return JDSP_OK;
    if (!left_host || !right_host || (n_out > 0 && !out_host)) return fail(ctx, JDSP_EINVAL, "jdsp_mvdr_apply: NULL buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = mvdr_reserve(h, n_blocks);
    if (rc) return rc;
    const size_t in_b = (size_t)n_blocks * 1024, out_b = (size_t)(n_out > 0 ? n_out : 1) * 1024;
    hipStream_t s = ctx->stream;
    jdsp::MvdrState *st_in = h->st[h->cur].get(), *st_out = h->st[h->cur ^ 1].get();
    double *rver = h->ws.rver.get();
    int *ver_base = h->ws.run.ver_base.get();
    unsigned long long *snap_mask = h->ws.run.snap_mask.get();
    jdsp::HostCall hc(ctx, "jdsp_mvdr_apply");
    const int16_t *d_l = hc.upload(left_host, in_b);
    const int16_t *d_r = hc.upload(right_host, in_b);
    int16_t *d_out = hc.alloc<int16_t>(out_b);
    float *d_pre = precast_host ? hc.alloc<float>(out_b * 2) : nullptr;
    // every block uses matrix version 0 = the caller's rgdSpatialCorr; the handle's own matrix and run length carry over
    hc.upload_to(rver, corr4_host, 4 * sizeof(double));
    hc.zero(ver_base, ((size_t)n_blocks / 64 + 1) * sizeof(int));
    hc.zero(snap_mask, ((size_t)n_blocks / 64 + 1) * sizeof(unsigned long long));
    hc.copy_dev(st_out, st_in, sizeof(jdsp::MvdrState));
    if (hc.ok() && jdsp::launch_mvdr_apply(s, d_l, d_r, n_blocks, h->calls, st_in, st_out, ver_base, snap_mask, rver,
                                           h->steer.get(), ctx->stft1024_table.get(), d_out, d_pre))
        hc.result(fail(ctx, JDSP_EHIP, "mvdr launch", hipGetLastError()));
    hc.download(out_host, d_out, (size_t)n_out * 1024);
    hc.download(precast_host, d_pre, (size_t)n_out * 2048);
    rc = hc.finish();
    if (!rc) {
        h->cur ^= 1;
        h->calls += n_blocks;
    }
    return rc;
}

int jdsp_mvdr_corr(jdsp_mvdr *h, double *corr4_host)
{
    if (!h || !corr4_host) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    JDSP_HIP(ctx, hipMemcpyAsync(corr4_host, h->st[h->cur].get()->corr, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JDSP_OK;
}

}  // extern "C"
