// streamfilter_api.hip -- C ABI of the multi-stream IIR equaliser and NLMS filter (include/jdsp.h).
// The coefficient design rounds every product and sum on its own, like the reference's build: no contraction.
#pragma clang fp contract(off)
#include "jdsp_internal.h"

using jdsp::fail;

namespace {

// 7Band_GEQ.cpp:32-59
constexpr double kGeqPi = 3.141592, kGeqRate = 48000.0, kGeqQ = 4.318, kGeqRoot2 = 1.0 / kGeqQ;
const double kGeqFreqs[7] = {44.0, 125.0, 250.0, 500.0, 2000.0, 6000.0, 11313.0};          // :47
const double kGeqGains[7] = {12.0, 12.0, 0.0, 0.0, 3.0, 0.0, -12.0};                        // :51-57

int stream_layout(jdsp_ctx *ctx, const char *who, long n_samples, long pitch)
{
    if (n_samples < 0 || pitch < n_samples || (pitch & 7))
        return fail(ctx, JDSP_EINVAL, (std::string(who) + ": n_samples >= 0, pitch >= n_samples and a multiple of 8").c_str());
    return JDSP_OK;
}

bool misaligned(const void *p) { return ((uintptr_t)p & 15u) != 0; }

// elements of a buffer of n_streams streams at that pitch: the last stream ends with its last sample
size_t extent(long n_streams, long n_samples, long pitch) { return (size_t)(n_streams - 1) * (size_t)pitch + (size_t)n_samples; }

}  // namespace

extern "C" {

/* ---- 7Band_GEQ.cpp ------------------------------------------------------------------------ */
int jdsp_geq_design(const double gain_db[7], double coeff[7][2][3])
{
    if (!coeff) return JDSP_EINVAL;
    const double *G = gain_db ? gain_db : kGeqGains;
    double K[7], V[7];
    for (int k = 0; k < 7; k++) {
        if (!std::isfinite(G[k])) return JDSP_EINVAL;
        K[k] = tan(kGeqPi * kGeqFreqs[k] / kGeqRate);                                       // :70-76
        V[k] = pow(10, G[k] / 20.0);                                                        // :61-67
        if (V[k] < 1) V[k] = 1.0 / V[k];                                                    // :139-142
    }
    double t;
    if (G[0] > 0) {                                                                         // :144-159 bass boost
        t = (1 + kGeqRoot2 * K[0] + pow(K[0], 2.0));
        coeff[0][0][0] = (1 + sqrt(V[0]) * kGeqRoot2 * K[0] + V[0] * pow(K[0], 2.0)) / t;
        coeff[0][0][1] = (2 * (V[0] * pow(K[0], 2.0) - 1)) / t;
        coeff[0][0][2] = (1 - sqrt(V[0]) * kGeqRoot2 * K[0] + V[0] * pow(K[0], 2.0)) / t;
        coeff[0][1][0] = 0.0;
        coeff[0][1][1] = (2 * (pow(K[0], 2.0) - 1)) / t;
        coeff[0][1][2] = (1 - kGeqRoot2 * K[0] + pow(K[0], 2.0)) / t;
    } else {                                                                                // :160-175 bass cut, as written
        t = (1 + kGeqRoot2 * sqrt(V[0]) * K[0] + V[0] * pow(K[0], 2.0));
        coeff[0][0][0] = (1 + kGeqRoot2 * K[0] + pow(K[0], 2.0)) / t;
        coeff[0][0][1] = (2 * (pow(K[0], 2.0) - 1)) / t;
        coeff[0][0][2] = (1 - kGeqRoot2 * K[0] + pow(K[0], 2.0)) / t;
        coeff[0][1][0] = 0.0;
        coeff[0][1][1] = (2 * (K[0] * pow(K[0], 2.0) - 1)) / t;
        coeff[0][1][2] = (1 - kGeqRoot2 * sqrt(K[0]) * K[0] + K[0] * pow(K[0], 2.0)) / t;
    }
    if (G[6] > 0) {                                                                         // :177-192 treble boost
        t = (1 + kGeqRoot2 * K[6] + pow(K[6], 2.0));
        coeff[6][0][0] = (V[6] + kGeqRoot2 * sqrt(V[6]) * K[6] + pow(K[6], 2.0)) / t;
        coeff[6][0][1] = (2 * (pow(K[6], 2.0) - V[6])) / t;
        coeff[6][0][2] = (V[6] - kGeqRoot2 * sqrt(V[6]) * K[6] + pow(K[6], 2.0)) / t;
        coeff[6][1][0] = 0.0;
        coeff[6][1][1] = (2 * (pow(K[6], 2.0) - 1)) / t;
        coeff[6][1][2] = (1 - kGeqRoot2 * K[6] + pow(K[6], 2.0)) / t;
    } else {                                                                                // :193-210 treble cut
        t = (V[6] + kGeqRoot2 * sqrt(V[6]) * K[6] + pow(K[6], 2.0));
        coeff[6][0][0] = (1 + kGeqRoot2 * K[6] + pow(K[6], 2.0)) / t;
        coeff[6][0][1] = (2 * (pow(K[6], 2.0) - 1)) / t;
        coeff[6][0][2] = (1 - kGeqRoot2 * K[6] + pow(K[6], 2.0)) / t;
        t = (1 + kGeqRoot2 / sqrt(V[6]) * K[6] + (pow(K[6], 2.0)) / V[6]);
        coeff[6][1][0] = 0.0;
        coeff[6][1][1] = (2 * ((pow(K[6], 2.0)) / V[6] - 1)) / t;
        coeff[6][1][2] = (1 - kGeqRoot2 / sqrt(V[6]) * K[6] + (pow(K[6], 2.0)) / V[6]) / t;
    }
    for (int k = 1; k < 6; k++) {                                                           // :212-249 peaking bands
        if (G[k] > 0) {
            t = (1 + ((1 / kGeqQ) * K[k]) + pow(K[k], 2.0));
            coeff[k][0][0] = (1 + ((V[k] / kGeqQ) * K[k]) + pow(K[k], 2.0)) / t;
            coeff[k][0][1] = (2 * (pow(K[k], 2.0) - 1)) / t;
            coeff[k][0][2] = (1 - ((V[k] / kGeqQ) * K[k]) + pow(K[k], 2.0)) / t;
            coeff[k][1][0] = 0.0;
            coeff[k][1][1] = coeff[k][0][1];
            coeff[k][1][2] = (1 - ((1 / kGeqQ) * K[k - 1]) + pow(K[k], 2.0)) / t;            // :231, K of the band below
        } else {
            t = (1 + ((V[k] / kGeqQ) * K[k]) + pow(K[k], 2.0));
            coeff[k][0][0] = (1 + ((1.0 / kGeqQ) * K[k]) + pow(K[k], 2.0)) / t;
            coeff[k][0][1] = (2 * (pow(K[k], 2.0) - 1)) / t;
            coeff[k][0][2] = (1 - ((1.0 / kGeqQ) * K[k]) + pow(K[k], 2.0)) / t;
            coeff[k][1][0] = 0.0;
            coeff[k][1][1] = coeff[k][0][1];
            coeff[k][1][2] = (1 - ((V[k] / kGeqQ) * K[k - 1]) + pow(K[k], 2.0)) / t;         // :247, likewise
        }
    }
    return JDSP_OK;
}

int jdsp_geq_create(jdsp_ctx *ctx, const double *coeff, int n_sections, long n_streams, jdsp_geq **out)
{
    if (!ctx || !out) return JDSP_EINVAL;
    *out = nullptr;
    if (n_sections < 1 || n_sections > 16) return fail(ctx, JDSP_EINVAL, "jdsp_geq_create: n_sections 1 .. 16");
    if (n_streams < 1) return fail(ctx, JDSP_EINVAL, "jdsp_geq_create: n_streams >= 1");
    double own[7][2][3];
    if (!coeff) {
        if (n_sections != 7) return fail(ctx, JDSP_EINVAL, "jdsp_geq_create: the default coefficients are 7 sections");
        (void)jdsp_geq_design(nullptr, own);
        coeff = &own[0][0][0];
    }
    for (int k = 0; k < n_sections; k++) {
        const double *c = coeff + 6 * k;
        double sum = 0;
        for (int i = 0; i < 6; i++) {
            if (!std::isfinite(c[i])) return fail(ctx, JDSP_EINVAL, "jdsp_geq_create: non-finite coefficient");
            if (i != 3) sum += fabs(c[i]);
        }
        // |pre-cast value| <= sum * 32768 must stay inside int32, where the cast is defined
        if (!(sum < 32768.0)) return fail(ctx, JDSP_EINVAL, "jdsp_geq_create: a section's |b0|+|b1|+|b2|+|a1|+|a2| must be below 2^15");
    }
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    jdsp_geq *h = new jdsp_geq;
    h->ctx = ctx;
    h->n_sections = n_sections;
    h->n_streams = n_streams;
    const size_t n_state = 2 * (size_t)(n_sections + 1) * (size_t)n_streams;
    hipError_t e = h->coeff.upload(coeff, 6 * (size_t)n_sections);
    if (e == hipSuccess) e = h->state.alloc(n_state);
    if (e == hipSuccess) e = hipMemsetAsync(h->state.get(), 0, sizeof(short) * n_state, ctx->stream);
    if (e != hipSuccess) {
        jdsp_geq_destroy(h);
        return fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_geq_create", e);
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_geq_destroy(jdsp_geq *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_geq_reset(jdsp_geq *h)
{
    if (!h) return JDSP_EINVAL;
    JDSP_HIP(h->ctx, hipMemsetAsync(h->state.get(), 0, sizeof(short) * h->state.count(), h->ctx->stream));
    return JDSP_OK;
}

int jdsp_geq_get_state(jdsp_geq *h, int16_t *state_host)
{
    if (!h || !state_host) return JDSP_EINVAL;
    jdsp::HostCall hc(h->ctx, "jdsp_geq_get_state");
    hc.download(state_host, h->state.get(), sizeof(short) * h->state.count());
    return hc.finish();
}

int jdsp_geq_set_state(jdsp_geq *h, const int16_t *state_host)
{
    if (!h || !state_host) return JDSP_EINVAL;
    jdsp::HostCall hc(h->ctx, "jdsp_geq_set_state");
    hc.upload_to(h->state.get(), state_host, sizeof(short) * h->state.count());
    return hc.finish();
}

int jdsp_geq_process_dev(jdsp_geq *h, const int16_t *pcm_dev, long n_samples, long pitch, int16_t *out_dev, double *precast_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = stream_layout(ctx, "jdsp_geq_process", n_samples, pitch);
    if (rc || n_samples == 0) return rc;
    if (!pcm_dev || !out_dev) return fail(ctx, JDSP_EINVAL, "jdsp_geq_process: bad buffer");
    if (misaligned(pcm_dev) || misaligned(out_dev) || misaligned(precast_dev))
        return fail(ctx, JDSP_EINVAL, "jdsp_geq_process: pcm, out and precast must be 16-byte aligned");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (jdsp::launch_geq(ctx->stream, pcm_dev, h->n_streams, n_samples, pitch, h->coeff.get(), h->n_sections, h->state.get(), out_dev, precast_dev))
        return fail(ctx, JDSP_EHIP, "geq launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_geq_process(jdsp_geq *h, const int16_t *pcm_host, long n_samples, long pitch, int16_t *out_host, double *precast_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = stream_layout(ctx, "jdsp_geq_process", n_samples, pitch);
    if (rc || n_samples == 0) return rc;
    if (!pcm_host || !out_host) return fail(ctx, JDSP_EINVAL, "jdsp_geq_process: bad buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = extent(h->n_streams, n_samples, pitch);
    jdsp::HostCall hc(ctx, "jdsp_geq_process");
    const int16_t *d_in = hc.upload(pcm_host, n * 2);
    int16_t *d_out = hc.alloc<int16_t>(n * 2);
    double *d_pc = precast_host ? hc.alloc<double>(n * 8) : nullptr;
    // what lies between the streams comes back as it went in
    if (pitch > n_samples) {
        hc.upload_to(d_out, out_host, n * 2);
        if (d_pc) hc.upload_to(d_pc, precast_host, n * 8);
    }
    if (hc.ok()) hc.result(jdsp_geq_process_dev(h, d_in, n_samples, pitch, d_out, d_pc));
    hc.download(out_host, d_out, n * 2);
    hc.download(precast_host, d_pc, n * 8);
    return hc.finish();
}

/* ---- NormalLMS.cpp ------------------------------------------------------------------------ */
int jdsp_nlms_create(jdsp_ctx *ctx, int filter_len, double mu, double compensation, long n_streams, jdsp_nlms **out)
{
    if (!ctx || !out) return JDSP_EINVAL;
    *out = nullptr;
    if (filter_len != 64 && filter_len != 128 && filter_len != 256)
        return fail(ctx, JDSP_EINVAL, "jdsp_nlms_create: filter_len 64 | 128 | 256");
    if (n_streams < 1) return fail(ctx, JDSP_EINVAL, "jdsp_nlms_create: n_streams >= 1");
    if (!std::isfinite(mu) || !std::isfinite(compensation))
        return fail(ctx, JDSP_EINVAL, "jdsp_nlms_create: non-finite coefficient");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    jdsp_nlms *h = new jdsp_nlms;
    h->ctx = ctx;
    h->filter_len = filter_len;
    h->n_streams = n_streams;
    h->mu = mu;
    h->compensation = compensation;
    hipError_t e = h->coef.alloc((size_t)filter_len * (size_t)n_streams);
    if (e == hipSuccess) e = h->keep.alloc((size_t)(filter_len - 1) * (size_t)n_streams);
    if (e != hipSuccess) {
        jdsp_nlms_destroy(h);
        return fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_nlms_create", e);
    }
    const int rc = jdsp_nlms_reset(h);
    if (rc) {
        jdsp_nlms_destroy(h);
        return rc;
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_nlms_destroy(jdsp_nlms *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_nlms_reset(jdsp_nlms *h)
{
    if (!h) return JDSP_EINVAL;
    JDSP_HIP(h->ctx, hipMemsetAsync(h->coef.get(), 0, sizeof(double) * h->coef.count(), h->ctx->stream));
    JDSP_HIP(h->ctx, hipMemsetAsync(h->keep.get(), 0, sizeof(short) * h->keep.count(), h->ctx->stream));
    return JDSP_OK;
}

int jdsp_nlms_get_state(jdsp_nlms *h, double *coef_host, int16_t *keep_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp::HostCall hc(h->ctx, "jdsp_nlms_get_state");
    hc.download(coef_host, h->coef.get(), sizeof(double) * h->coef.count());
    hc.download(keep_host, h->keep.get(), sizeof(short) * h->keep.count());
    return hc.finish();
}

int jdsp_nlms_set_state(jdsp_nlms *h, const double *coef_host, const int16_t *keep_host)
{
    if (!h || !coef_host || !keep_host) return JDSP_EINVAL;
    jdsp::HostCall hc(h->ctx, "jdsp_nlms_set_state");
    hc.upload_to(h->coef.get(), coef_host, sizeof(double) * h->coef.count());
    hc.upload_to(h->keep.get(), keep_host, sizeof(short) * h->keep.count());
    return hc.finish();
}

int jdsp_nlms_process_dev(jdsp_nlms *h, const int16_t *input_dev, const int16_t *reference_dev, long n_samples, long pitch,
                          int16_t *est_dev, int16_t *err_dev, double *precast_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = stream_layout(ctx, "jdsp_nlms_process", n_samples, pitch);
    if (rc || n_samples == 0) return rc;
    if (!input_dev || !reference_dev || !est_dev || !err_dev) return fail(ctx, JDSP_EINVAL, "jdsp_nlms_process: bad buffer");
    if (misaligned(input_dev) || misaligned(reference_dev) || misaligned(est_dev) || misaligned(err_dev) || misaligned(precast_dev))
        return fail(ctx, JDSP_EINVAL, "jdsp_nlms_process: input, reference, est, err and precast must be 16-byte aligned");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (jdsp::launch_nlms(ctx->stream, input_dev, reference_dev, h->n_streams, n_samples, pitch, h->filter_len, h->mu,
                          h->compensation, h->coef.get(), h->keep.get(), est_dev, err_dev, precast_dev))
        return fail(ctx, JDSP_EHIP, "nlms launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_nlms_process(jdsp_nlms *h, const int16_t *input_host, const int16_t *reference_host, long n_samples, long pitch,
                      int16_t *est_host, int16_t *err_host, double *precast_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = stream_layout(ctx, "jdsp_nlms_process", n_samples, pitch);
    if (rc || n_samples == 0) return rc;
    if (!input_host || !reference_host || !est_host || !err_host) return fail(ctx, JDSP_EINVAL, "jdsp_nlms_process: bad buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = extent(h->n_streams, n_samples, pitch);
    jdsp::HostCall hc(ctx, "jdsp_nlms_process");
    const int16_t *d_in = hc.upload(input_host, n * 2);
    const int16_t *d_ref = hc.upload(reference_host, n * 2);
    int16_t *d_est = hc.alloc<int16_t>(n * 2), *d_err = hc.alloc<int16_t>(n * 2);
    double *d_pc = precast_host ? hc.alloc<double>(n * 8) : nullptr;
    if (pitch > n_samples) {
        hc.upload_to(d_est, est_host, n * 2);
        hc.upload_to(d_err, err_host, n * 2);
        if (d_pc) hc.upload_to(d_pc, precast_host, n * 8);
    }
    if (hc.ok()) hc.result(jdsp_nlms_process_dev(h, d_in, d_ref, n_samples, pitch, d_est, d_err, d_pc));
    hc.download(est_host, d_est, n * 2);
    hc.download(err_host, d_err, n * 2);
    hc.download(precast_host, d_pc, n * 8);
    return hc.finish();
}

}  // extern "C"
