// gmm_train_api.hip -- C ABI of GMM training (GMMAlgorithm_Train_Auto_ver2.cpp) on MFCC vectors that are already in
// HBM, and the host-only conversion to the test program's PCA_LEN 4 record.
#include "jdsp_internal.h"

using jdsp::fail;

namespace {

int grow(jdsp_gmm_trainer *h, long frames)
{
    jdsp_ctx *ctx = h->ctx;
    const size_t n = (size_t)frames;
    if (n * 4 <= h->wbuf.count()) return JDSP_OK;       // wbuf is made last: it stands for both
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h->sel.reset();
    h->wbuf.reset();
    JDSP_HIP(ctx, h->sel.alloc(n));
    JDSP_HIP(ctx, h->wbuf.alloc(n * 4));
    return JDSP_OK;
}

}  // namespace

extern "C" {

int jdsp_gmm_train_create(jdsp_ctx *ctx, int n_classes, jdsp_gmm_trainer **out)
{
    if (!ctx || !out) return JDSP_EINVAL;
    *out = nullptr;
    if (n_classes < 1 || n_classes > jdsp::kGmmTrainMaxClasses)
        return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_create: 1..1024 classes");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    jdsp_gmm_trainer *h = new (std::nothrow) jdsp_gmm_trainer();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_gmm_train_create");
    h->ctx = ctx;
    h->n_classes = n_classes;
    hipError_t e = h->state.alloc((size_t)n_classes);
    if (e == hipSuccess) e = h->out.alloc((size_t)n_classes);
    if (e == hipSuccess) e = hipMemsetAsync(h->state.get(), 0, (size_t)n_classes * sizeof(jdsp::GmmTrainState), ctx->stream);
    if (e != hipSuccess) {
        jdsp_gmm_train_destroy(h);
        return fail(ctx, JDSP_EHIP, "jdsp_gmm_train_create: allocation", e);
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_gmm_train_destroy(jdsp_gmm_trainer *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_gmm_train_reset(jdsp_gmm_trainer *h)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipMemsetAsync(h->state.get(), 0, (size_t)h->n_classes * sizeof(jdsp::GmmTrainState), ctx->stream));
    return JDSP_OK;
}

int jdsp_gmm_train_set_option(jdsp_gmm_trainer *h, const char *name, long value)
{
    if (!h || !name) return JDSP_EINVAL;
    if (!strcmp(name, "kmeans_max_passes")) {
        if (value < 1 || value > 1000000000L) return fail(h->ctx, JDSP_EINVAL, "jdsp_gmm_train_set_option: kmeans_max_passes >= 1");
        h->kmeans_max_passes = (int)value;
        return JDSP_OK;
    }
    if (!strcmp(name, "threads_per_class")) {
        if (value != 256 && value != 512 && value != 1024)
            return fail(h->ctx, JDSP_EINVAL, "jdsp_gmm_train_set_option: threads_per_class is 256, 512 or 1024");
        h->threads = (int)value;
        return JDSP_OK;
    }
    return fail(h->ctx, JDSP_EINVAL, "jdsp_gmm_train_set_option: unknown option");
}

int jdsp_gmm_train_reserve(jdsp_gmm_trainer *h, long max_frames, long max_files)
{
    if (!h) return JDSP_EINVAL;
    if (max_frames < 0 || max_files < 0) return fail(h->ctx, JDSP_EINVAL, "jdsp_gmm_train_reserve: negative size");
    return grow(h, max_frames > 0 ? max_frames : 1);
}

int jdsp_gmm_train_files_dev(jdsp_gmm_trainer *h, const double *feats_dev, long n_frames, const int64_t *file_first_dev,
                             const int32_t *file_class_dev, long n_files)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_files < 0 || n_frames < 0) return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_files_dev: negative size");
    if (n_files > 0 && (!file_first_dev || !file_class_dev))
        return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_files_dev: bad buffer");
    if (n_frames > 0 && (!feats_dev || ((uintptr_t)feats_dev & 15u)))
        return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_files_dev: feats must be 16-byte aligned");
    if (n_files == 0) return JDSP_OK;
    int rc = grow(h, n_frames > 0 ? n_frames : 1);
    if (rc) return rc;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (jdsp::launch_gmm_train(ctx->stream, h->threads, h->n_classes, feats_dev, n_frames, (const long long *)file_first_dev,
                               (const int *)file_class_dev, n_files, h->kmeans_max_passes, h->state.get(), h->sel.get(), h->wbuf.get()))
        return fail(ctx, JDSP_EHIP, "gmm train launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_gmm_train_files(jdsp_gmm_trainer *h, const double *feats_host, const int64_t *file_first_host,
                         const int32_t *file_class_host, long n_files)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_files < 0 || (n_files > 0 && (!file_first_host || !file_class_host)))
        return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_files: bad buffer");
    if (n_files == 0) return JDSP_OK;
    if (file_first_host[0] != 0) return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_files: file_first[0] must be 0");
    for (long f = 0; f < n_files; f++) {
        if (file_class_host[f] < 0 || file_class_host[f] >= h->n_classes)
            return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_files: class out of range");
        if (file_first_host[f + 1] <= file_first_host[f])
            return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_files: offsets must increase (no empty file)");
    }
    const long n_frames = (long)file_first_host[n_files];
    if (!feats_host) return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_files: bad buffer");
    // a class's first file needs frames 0, 4, 8 and 12 (Train:120-124): is this call's first file of a class its
    // first file ever?
    std::vector<jdsp::GmmTrainState> st(h->n_classes);
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipMemcpyAsync(st.data(), h->state.get(), st.size() * sizeof(st[0]), hipMemcpyDeviceToHost, ctx->stream));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<char> seen(h->n_classes);
    for (int c = 0; c < h->n_classes; c++) seen[c] = st[c].i[jdsp::kTrSeen] != 0;
    for (long f = 0; f < n_files; f++) {
        const int c = file_class_host[f];
        if (!seen[c] && file_first_host[f + 1] - file_first_host[f] < 13)
            return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_files: a class's first file needs >= 13 vectors");
        seen[c] = 1;
    }
    jdsp::HostCall hc(ctx, "jdsp_gmm_train_files");
    const double *d_feats = hc.upload(feats_host, (size_t)n_frames * 12 * sizeof(double));
    const int64_t *d_first = hc.upload(file_first_host, (size_t)(n_files + 1) * sizeof(int64_t));
    const int32_t *d_class = hc.upload(file_class_host, (size_t)n_files * sizeof(int32_t));
    if (hc.ok()) hc.result(jdsp_gmm_train_files_dev(h, d_feats, n_frames, d_first, d_class, n_files));
    return hc.finish();
}

int jdsp_gmm_train_params_dev(jdsp_gmm_trainer *h, jdsp_gmm_train_param *out_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (!out_dev || ((uintptr_t)out_dev & 7u)) return fail(ctx, JDSP_EINVAL, "jdsp_gmm_train_params_dev: bad buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (jdsp::launch_gmm_train_params(ctx->stream, h->n_classes, h->state.get(), out_dev))
        return fail(ctx, JDSP_EHIP, "gmm train params launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_gmm_train_params(jdsp_gmm_trainer *h, jdsp_gmm_train_param *out_host, jdsp_gmm_train_stats *stats_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (out_host) {
        int rc = jdsp_gmm_train_params_dev(h, h->out.get());
        if (rc) return rc;
        JDSP_HIP(ctx, hipMemcpyAsync(out_host, h->out.get(), (size_t)h->n_classes * sizeof(jdsp_gmm_train_param),
                                     hipMemcpyDeviceToHost, ctx->stream));
    }
    std::vector<jdsp::GmmTrainState> st(stats_host ? h->n_classes : 0);
    if (stats_host)
        JDSP_HIP(ctx, hipMemcpyAsync(st.data(), h->state.get(), st.size() * sizeof(st[0]), hipMemcpyDeviceToHost, ctx->stream));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t c = 0; c < st.size(); c++) {
        jdsp_gmm_train_stats &o = stats_host[c];
        o.kmeans_passes = st[c].i[jdsp::kTrPasses];
        o.kmeans_capped = st[c].i[jdsp::kTrCapped];
        for (int k = 0; k < 4; k++) o.selected[k] = st[c].i[jdsp::kTrSelected + k];
        o.files = st[c].i[jdsp::kTrFiles];
        o.status = st[c].i[jdsp::kTrStatus];
        o.kmeans_cost = st[c].d[jdsp::kTrCost];
    }
    return JDSP_OK;
}

int jdsp_gmm_param_from_train(const jdsp_gmm_train_param *in, int n, jdsp_gmm_param *out)
{
    if (n < 0 || (n > 0 && (!in || !out))) return JDSP_EINVAL;
    for (int c = 0; c < n; c++) {
        memcpy(out[c].alpa, in[c].alpa, sizeof(out[c].alpa));
        memcpy(out[c].mean, in[c].mean, sizeof(out[c].mean));
        memcpy(out[c].covariance, in[c].covariance, sizeof(out[c].covariance));
        for (int k = 0; k < 4; k++)                                                  // GMMTest:216-235 reads [12][4]
            for (int i = 0; i < 12; i++)
                for (int j = 0; j < 4; j++) out[c].eigenVector[k][i][j] = in[c].eigenVector[k][i][j];
    }
    return JDSP_OK;
}

}  // extern "C"
