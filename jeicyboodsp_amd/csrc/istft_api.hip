// istft_api.hip -- C ABI of the STFT synthesis stream object (include/jdsp.h, jdsp_istft_*).
#include "ola_api.h"

using jdsp::fail;
using jdsp::OlaStream;

struct jdsp_istft {
    jdsp_ctx *ctx = nullptr;
    jdsp_istft_cfg cfg;
    jdsp::DevBuf<float> blob;             // ws[n_fft] (w_s / n_fft), then the stream's share
    float *ws = nullptr;                  // view into blob
    OlaStream ola;
    jdsp::OlaStreams live;                // the live streams (jdsp_istft_streams_*), none until _streams_reserve
    jdsp::DevBuf<jdsp_c32> h_spec;        // the host entry's device copy of the spectra, grown on demand
};

static int bins_of(const jdsp_istft_cfg &c) { return c.layout == JDSP_SPEC_HALF ? c.n_fft / 2 + 1 : c.n_fft; }

// what the handle checks of the input of a ragged call itself (jdsp::OwnRules, ola_api.h)
static jdsp::OwnRules own_rules(const jdsp_istft *h, const void *spec, long row_pitch)
{
    jdsp::OwnRules own;
    if (row_pitch < bins_of(h->cfg)) own.pitch = "row_pitch below the layout's bins";
    if (!jdsp::aligned(spec, 8)) own.align = "spec must be 8-byte aligned";
    if (!spec) own.null = "spec is NULL";
    return own;
}

// jdsp_istft_batch_dev (live == NULL) and jdsp_istft_streams_dev
static int ragged_dev(jdsp_istft *h, jdsp::OlaStreams *live, const jdsp_c32 *spec_dev, long row_pitch,
                      const int64_t *stream_id_dev, const int64_t *sample_first_dev, const int64_t *frame_first_dev, long n,
                      long n_frames_total, int16_t *out_i16_dev, float *out_f32_dev)
{
    jdsp_ctx *ctx = h->ctx;
    const char *entry = live ? "jdsp_istft_streams" : "jdsp_istft_batch";
    switch (jdsp::ragged_call_check(ctx, live, entry, own_rules(h, spec_dev, row_pitch), stream_id_dev, sample_first_dev,
                                    frame_first_dev, n, n_frames_total, out_i16_dev, out_f32_dev)) {
    case jdsp::RaggedCall::kRejected: return JDSP_EINVAL;
    case jdsp::RaggedCall::kNothing: return JDSP_OK;
    case jdsp::RaggedCall::kLaunch: break;
    }
    jdsp::LiveStreams view;
    if (live) view = live->view(stream_id_dev);
    if (jdsp::launch_istft_ragged(ctx->stream, ctx->n_cu, h->cfg.n_fft, h->cfg.hop, h->cfg.layout == JDSP_SPEC_HALF,
                                  reinterpret_cast<const float2 *>(spec_dev), row_pitch, n_frames_total,
                                  reinterpret_cast<const long long *>(sample_first_dev),
                                  reinterpret_cast<const long long *>(frame_first_dev), n, live ? &view : nullptr, h->ws,
                                  h->ola.g, out_i16_dev, out_f32_dev, ctx->stft1024_table.get(), h->ola.run_opt))
        return fail(ctx, JDSP_EHIP, (std::string(entry) + ": launch").c_str(), hipGetLastError());
    return live ? live->commit(entry, stream_id_dev, frame_first_dev, n) : JDSP_OK;
}

// jdsp_istft_batch (live == NULL: an utterance's span is its hop (F_u - 1) + n_fft samples) and jdsp_istft_streams (a
// chunk's span is its hop F_c output samples)
static int ragged_host(jdsp_istft *h, jdsp::OlaStreams *live, const jdsp_c32 *spec_host, long row_pitch,
                       const int64_t *stream_id_host, const int64_t *sample_first_host, const int64_t *frame_first_host,
                       long n, long n_samples, int16_t *out_i16_host, float *out_f32_host)
{
    return jdsp::ragged_host_call(
        h->ola, live, live ? "jdsp_istft_streams" : "jdsp_istft_batch", own_rules(h, spec_host, row_pitch), stream_id_host,
        sample_first_host, frame_first_host, n, n_samples, live ? h->cfg.hop : h->cfg.n_fft, out_i16_host, out_f32_host,
        [&](jdsp::HostCall &hc, long n_total, long) {
            const size_t n_in = (size_t)(n_total - 1) * row_pitch + bins_of(h->cfg);
            const hipError_t e = h->h_spec.grow(n_in);
            if (e == hipSuccess) hc.upload_to(h->h_spec.get(), spec_host, n_in * sizeof(jdsp_c32));
            return e;
        },
        [&](const int64_t *d_id, const int64_t *d_sample, const int64_t *d_frame, long n_total, int16_t *d_i16, float *d_f32) {
            return ragged_dev(h, live, h->h_spec.get(), row_pitch, d_id, d_sample, d_frame, n, n_total, d_i16, d_f32);
        });
}

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
    const int n = c.n_fft, hop = c.hop;
    std::vector<float> host((size_t)n + hop);
    for (int i = 0; i < n; i++) host[i] = (float)(OlaStream::window_at(c.synthesis_window, i, n) / n);
    // the WOLA gain; 1 without an analysis window
    if (!OlaStream::wola_gain(c.analysis_window, c.synthesis_window, n, hop, c.analysis_window != JDSP_WIN_NONE, &host[n]))
        return fail(ctx, JDSP_EINVAL, "jdsp_istft_create: the windows' overlap-add vanishes (no WOLA inverse)");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp::ensure_stft1024_table(ctx);          // the transform's twiddles and the split's W^m
    if (rc) return rc;
    jdsp_istft *h = new (std::nothrow) jdsp_istft();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_istft_create");
    h->ctx = ctx;
    h->cfg = c;
    hipError_t e = h->blob.alloc((size_t)n + OlaStream::floats(n, hop));
    if (e == hipSuccess) {
        h->ws = h->blob.get();
        h->ola.attach(ctx, n, hop, h->ws + n);
        h->live.ola = &h->ola;
        e = hipMemcpy(h->ws, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        delete h;                                       // nothing of it is enqueued yet
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
    if (h) h->ola.drain();
    delete h;
    return JDSP_OK;
}

int jdsp_istft_reset(jdsp_istft *h) { return h ? h->ola.reset() : JDSP_EINVAL; }

int jdsp_istft_set_option(jdsp_istft *h, const char *name, long value)
{
    if (!h || !name) return JDSP_EINVAL;
    if (!strcmp(name, "frames_per_wave")) {
        if (value != 0 && (value < h->ola.least_run() || value > (1L << 30)))
            return fail(h->ctx, JDSP_EINVAL, "jdsp_istft_set_option: frames_per_wave must be 0 (auto) or >= max(R - 1, 1)");
        h->ola.run_opt = (int)value;
        return JDSP_OK;
    }
    return fail(h->ctx, JDSP_EINVAL, "jdsp_istft_set_option: unknown option");
}

long jdsp_istft_samples_out(const jdsp_istft *h, long n_frames) { return h ? h->ola.samples_out(n_frames) : 0; }

int jdsp_istft_process_dev(jdsp_istft *h, const jdsp_c32 *spec_dev, long row_pitch, long n_frames, int16_t *out_i16_dev,
                           float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_frames < 0) return fail(ctx, JDSP_EINVAL, "jdsp_istft_process: n_frames < 0");
    if (row_pitch < bins_of(h->cfg)) return fail(ctx, JDSP_EINVAL, "jdsp_istft_process: row_pitch below the layout's bins");
    if (!jdsp::aligned(spec_dev, 8) || !jdsp::aligned(out_i16_dev, 4) || !jdsp::aligned(out_f32_dev, 8))
        return fail(ctx, JDSP_EINVAL, "jdsp_istft_process: spec must be 8-byte, out_i16 4-byte, out_f32 8-byte aligned");
    if (n_frames == 0) return JDSP_OK;
    if (!spec_dev) return fail(ctx, JDSP_EINVAL, "jdsp_istft_process: spec is NULL");
    OlaStream &o = h->ola;
    if (jdsp::launch_istft(ctx->stream, ctx->n_cu, h->cfg.n_fft, h->cfg.hop, h->cfg.layout == JDSP_SPEC_HALF,
                           reinterpret_cast<const float2 *>(spec_dev), row_pitch, n_frames, h->ws, o.g, o.tail[o.cur],
                           o.tail[o.cur ^ 1], out_i16_dev, out_f32_dev, ctx->stft1024_table.get(), o.run_opt))
        return fail(ctx, JDSP_EHIP, "jdsp_istft_process: launch", hipGetLastError());
    o.cur ^= 1;
    return JDSP_OK;
}

int jdsp_istft_flush_dev(jdsp_istft *h, int16_t *out_i16_dev, float *out_f32_dev)
{
    return h ? h->ola.flush_dev("jdsp_istft_flush", out_i16_dev, out_f32_dev) : JDSP_EINVAL;
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
    int16_t *d_i16 = nullptr;
    float *d_f32 = nullptr;
    hipError_t e = h->h_spec.grow(n_in);
    if (e == hipSuccess) e = h->ola.stage_out(n_out, out_i16_host, out_f32_host, d_i16, d_f32);
    if (e != hipSuccess) return fail(ctx, JDSP_EHIP, "jdsp_istft_process: buffers", e);
    jdsp::HostCall hc(ctx, "jdsp_istft_process");                       // the buffers are the handle's
    hc.upload_to(h->h_spec.get(), spec_host, n_in * sizeof(jdsp_c32));
    if (hc.ok()) hc.result(jdsp_istft_process_dev(h, h->h_spec.get(), row_pitch, n_frames, d_i16, d_f32));
    h->ola.download_out(hc, n_out, out_i16_host, out_f32_host);
    return hc.finish();
}

int jdsp_istft_flush(jdsp_istft *h, int16_t *out_i16_host, float *out_f32_host)
{
    return h ? h->ola.flush("jdsp_istft_flush", out_i16_host, out_f32_host) : JDSP_EINVAL;
}

int jdsp_istft_batch_dev(jdsp_istft *h, const jdsp_c32 *spec_dev, long row_pitch, const int64_t *sample_first_dev,
                         const int64_t *frame_first_dev, long n_utts, long n_frames_total, int16_t *out_i16_dev,
                         float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    return ragged_dev(h, nullptr, spec_dev, row_pitch, nullptr, sample_first_dev, frame_first_dev, n_utts, n_frames_total,
                      out_i16_dev, out_f32_dev);
}

int jdsp_istft_batch(jdsp_istft *h, const jdsp_c32 *spec_host, long row_pitch, const int64_t *sample_first_host,
                     const int64_t *frame_first_host, long n_utts, long n_samples, int16_t *out_i16_host,
                     float *out_f32_host)
{
    if (!h) return JDSP_EINVAL;
    return ragged_host(h, nullptr, spec_host, row_pitch, nullptr, sample_first_host, frame_first_host, n_utts, n_samples,
                       out_i16_host, out_f32_host);
}

// ---- live streams ---------------------------------------------------------------------------------------------------

int jdsp_istft_streams_reserve(jdsp_istft *h, long n_streams)
{
    return h ? h->live.reserve("jdsp_istft_streams_reserve", n_streams) : JDSP_EINVAL;
}

int jdsp_istft_streams_reset_dev(jdsp_istft *h, const int64_t *stream_id_dev, long n_ids)
{
    return h ? h->live.reset_dev("jdsp_istft_streams_reset", stream_id_dev, n_ids) : JDSP_EINVAL;
}

int jdsp_istft_streams_dev(jdsp_istft *h, const jdsp_c32 *spec_dev, long row_pitch, const int64_t *stream_id_dev,
                           const int64_t *sample_first_dev, const int64_t *frame_first_dev, long n_chunks,
                           long n_frames_total, int16_t *out_i16_dev, float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    return ragged_dev(h, &h->live, spec_dev, row_pitch, stream_id_dev, sample_first_dev, frame_first_dev, n_chunks,
                      n_frames_total, out_i16_dev, out_f32_dev);
}

int jdsp_istft_streams_flush_dev(jdsp_istft *h, const int64_t *stream_id_dev, const int64_t *sample_first_dev, long n_ids,
                                 int16_t *out_i16_dev, float *out_f32_dev)
{
    return h ? h->live.flush_dev("jdsp_istft_streams_flush", stream_id_dev, sample_first_dev, n_ids, out_i16_dev, out_f32_dev)
             : JDSP_EINVAL;
}

int jdsp_istft_streams(jdsp_istft *h, const jdsp_c32 *spec_host, long row_pitch, const int64_t *stream_id_host,
                       const int64_t *sample_first_host, const int64_t *frame_first_host, long n_chunks, long n_samples,
                       int16_t *out_i16_host, float *out_f32_host)
{
    if (!h) return JDSP_EINVAL;
    return ragged_host(h, &h->live, spec_host, row_pitch, stream_id_host, sample_first_host, frame_first_host, n_chunks,
                       n_samples, out_i16_host, out_f32_host);
}

int jdsp_istft_streams_flush(jdsp_istft *h, const int64_t *stream_id_host, const int64_t *sample_first_host, long n_ids,
                             long n_samples, int16_t *out_i16_host, float *out_f32_host)
{
    return h ? h->live.flush("jdsp_istft_streams_flush", stream_id_host, sample_first_host, n_ids, n_samples, out_i16_host,
                             out_f32_host)
             : JDSP_EINVAL;
}

}  // extern "C"
