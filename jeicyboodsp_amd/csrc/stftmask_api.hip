// stftmask_api.hip -- C ABI of the fused STFT masking stream object (include/jdsp.h, jdsp_stftmask_*).
#include "ola_api.h"

using jdsp::fail;
using jdsp::OlaStream;

struct jdsp_stftmask {
    jdsp_ctx *ctx = nullptr;
    jdsp_stftmask_cfg cfg;
    jdsp::DevBuf<float> blob;             // wa[n] (w_a / 2), ws[n] (w_s), then the stream's share
    float *wa = nullptr, *ws = nullptr;   // views into blob
    OlaStream ola;
    jdsp::OlaStreams live;                // the live streams (jdsp_stftmask_streams_*), none until _streams_reserve
    // the host entry's device copies of its inputs, grown on demand
    jdsp::DevBuf<int16_t> h_pcm;
    jdsp::DevBuf<char> h_mask;            // bytes: rows of float or jdsp_c32
    // the FP64 pass over the frames FP32 cannot hold (stftmask_kernels.hip, stftmask_frame_f64), sized at create
    jdsp::DevBuf<double> f64;             // w_a[n], w_s[n], exp(-2 pi i t / n) for t < n/2 as (re, im)
    // count[epoch & 1]: the recomputed frames of the call with that number (jdsp_stftmask_frames_recomputed); every
    // call's kernel zeroes the other word for the call after it, so nothing is enqueued to zero one
    jdsp::DevBuf<unsigned int> count;
    unsigned int epoch = 0;
    int count_valid = 0;                  // the last call launched (under `epoch`) since create / reset

    unsigned int next_epoch()
    {
        ++epoch;
        count_valid = 1;
        return epoch;
    }
};

static constexpr int kBins = 513;         // n/2 + 1 of the one supported n_fft

static size_t mask_elem(const jdsp_stftmask *h) { return h->cfg.mask_kind == JDSP_MASK_COMPLEX ? sizeof(jdsp_c32) : sizeof(float); }

// what the handle checks of the inputs of a ragged call itself (jdsp::OwnRules, ola_api.h)
static jdsp::OwnRules own_rules(const jdsp_stftmask *h, const void *pcm, const void *mask, long mask_pitch)
{
    jdsp::OwnRules own;
    if (mask_pitch != 0 && mask_pitch < kBins) own.pitch = "mask_pitch must be 0 (one row) or >= n_fft/2 + 1";
    if (!jdsp::aligned(pcm, 4) || !jdsp::aligned(mask, mask_elem(h)))
        own.align = "pcm must be 4-byte aligned, the mask 4-byte (REAL) or 8-byte (COMPLEX)";
    if (!pcm || !mask) own.null = "pcm or mask is NULL";
    return own;
}

// jdsp_stftmask_batch_dev (live == NULL) and jdsp_stftmask_streams_dev
static int ragged_dev(jdsp_stftmask *h, jdsp::OlaStreams *live, const int16_t *pcm_dev, const void *mask_dev,
                      long mask_pitch, const int64_t *stream_id_dev, const int64_t *sample_first_dev,
                      const int64_t *frame_first_dev, long n, long n_frames_total, int16_t *out_i16_dev, float *out_f32_dev)
{
    jdsp_ctx *ctx = h->ctx;
    const char *entry = live ? "jdsp_stftmask_streams" : "jdsp_stftmask_batch";
    switch (jdsp::ragged_call_check(ctx, live, entry, own_rules(h, pcm_dev, mask_dev, mask_pitch), stream_id_dev,
                                    sample_first_dev, frame_first_dev, n, n_frames_total, out_i16_dev, out_f32_dev)) {
    case jdsp::RaggedCall::kRejected: return JDSP_EINVAL;
    case jdsp::RaggedCall::kNothing: h->count_valid = 0; return JDSP_OK;   // a call of no frames recomputed none
    case jdsp::RaggedCall::kLaunch: break;
    }
    jdsp::LiveStreams view;
    if (live) view = live->view(stream_id_dev);
    if (jdsp::launch_stftmask_ragged(ctx->stream, ctx->n_cu, h->cfg.hop, h->cfg.mask_kind == JDSP_MASK_COMPLEX, pcm_dev,
                                     mask_dev, mask_pitch, n_frames_total,
                                     reinterpret_cast<const long long *>(sample_first_dev),
                                     reinterpret_cast<const long long *>(frame_first_dev), n, live ? &view : nullptr, h->wa,
                                     h->ws, h->ola.g, out_i16_dev, out_f32_dev, ctx->stft1024_table.get(), h->ola.run_opt,
                                     h->f64.get(), h->count.get(), h->next_epoch()))
        return fail(ctx, JDSP_EHIP, (std::string(entry) + ": launch").c_str(), hipGetLastError());
    return live ? live->commit(entry, stream_id_dev, frame_first_dev, n) : JDSP_OK;
}

// jdsp_stftmask_batch (live == NULL) and jdsp_stftmask_streams
static int ragged_host(jdsp_stftmask *h, jdsp::OlaStreams *live, const int16_t *pcm_host, long n_samples,
                       const void *mask_host, long mask_pitch, const int64_t *stream_id_host,
                       const int64_t *sample_first_host, const int64_t *frame_first_host, long n, int16_t *out_i16_host,
                       float *out_f32_host)
{
    return jdsp::ragged_host_call(
        h->ola, live, live ? "jdsp_stftmask_streams" : "jdsp_stftmask_batch", own_rules(h, pcm_host, mask_host, mask_pitch),
        stream_id_host, sample_first_host, frame_first_host, n, n_samples, h->cfg.n_fft, out_i16_host, out_f32_host,
        [&](jdsp::HostCall &hc, long n_total, long end) {
            const size_t mask_bytes = ((size_t)(n_total - 1) * mask_pitch + kBins) * mask_elem(h);
            hipError_t e = h->h_pcm.grow((size_t)n_samples);
            if (e == hipSuccess) e = h->h_mask.grow(mask_bytes);
            if (e != hipSuccess) return e;
            hc.upload_to(h->h_pcm.get(), pcm_host, (size_t)end * sizeof(int16_t));   // nothing past the last span is read
            hc.upload_to(h->h_mask.get(), mask_host, mask_bytes);
            return hipSuccess;
        },
        [&](const int64_t *d_id, const int64_t *d_sample, const int64_t *d_frame, long n_total, int16_t *d_i16, float *d_f32) {
            return ragged_dev(h, live, h->h_pcm.get(), h->h_mask.get(), mask_pitch, d_id, d_sample, d_frame, n, n_total,
                              d_i16, d_f32);
        });
}

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
    const int n = c.n_fft, hop = c.hop;
    std::vector<float> host(2 * (size_t)n + hop);
    for (int i = 0; i < n; i++) {
        host[i] = (float)(0.5 * OlaStream::window_at(c.analysis_window, i, n));   // the forward split's 1/2 (frame_io.h)
        host[(size_t)n + i] = (float)OlaStream::window_at(c.synthesis_window, i, n);
    }
    // the WOLA gain; 1 without normalisation
    if (!OlaStream::wola_gain(c.analysis_window, c.synthesis_window, n, hop, c.normalise != 0, &host[2 * (size_t)n]))
        return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_create: the windows' overlap-add vanishes (no WOLA inverse)");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp::ensure_stft1024_table(ctx);          // the transform's twiddles and the split's W^m
    if (rc) return rc;
    jdsp_stftmask *h = new (std::nothrow) jdsp_stftmask();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_stftmask_create");
    h->ctx = ctx;
    h->cfg = c;
    std::vector<double> host64(3 * (size_t)n);
    for (int i = 0; i < n; i++) {
        host64[i] = OlaStream::window_at(c.analysis_window, i, n);
        host64[(size_t)n + i] = OlaStream::window_at(c.synthesis_window, i, n);
    }
    for (int t = 0; t < n / 2; t++) {
        const double a = -2.0 * 3.14159265358979323846 * t / n;
        host64[2 * (size_t)n + 2 * t] = cos(a);
        host64[2 * (size_t)n + 2 * t + 1] = sin(a);
    }
    hipError_t e = h->blob.alloc(2 * (size_t)n + OlaStream::floats(n, hop));
    if (e == hipSuccess) e = h->f64.upload(host64.data(), host64.size());
    const unsigned int zero[2] = {0, 0};
    if (e == hipSuccess) e = h->count.upload(zero, 2);
    if (e == hipSuccess) {
        h->wa = h->blob.get();
        h->ws = h->wa + n;
        h->ola.attach(ctx, n, hop, h->ws + n);
        h->live.ola = &h->ola;
        e = hipMemcpy(h->wa, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        delete h;                                       // nothing of it is enqueued yet
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
    if (h) h->ola.drain();
    delete h;
    return JDSP_OK;
}

int jdsp_stftmask_reset(jdsp_stftmask *h)
{
    if (!h) return JDSP_EINVAL;
    h->count_valid = 0;
    return h->ola.reset();
}

long jdsp_stftmask_frames_recomputed(const jdsp_stftmask *h)
{
    if (!h) return JDSP_EINVAL;
    if (!h->count_valid) return 0;
    jdsp_ctx *ctx = h->ctx;
    unsigned int n = 0;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipMemcpyAsync(&n, h->count.get() + (h->epoch & 1), sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return (long)n;
}

int jdsp_stftmask_set_option(jdsp_stftmask *h, const char *name, long value)
{
    if (!h || !name) return JDSP_EINVAL;
    if (!strcmp(name, "frames_per_wave")) {
        const long least = h->ola.least_run();
        if (value < 0 || value > (1L << 30))
            return fail(h->ctx, JDSP_EINVAL, "jdsp_stftmask_set_option: frames_per_wave must be 0 (auto) or positive");
        h->ola.run_opt = (int)(value != 0 && value < least ? least : value);      // clamped to >= max(R - 1, 1)
        return JDSP_OK;
    }
    return fail(h->ctx, JDSP_EINVAL, "jdsp_stftmask_set_option: unknown option");
}

long jdsp_stftmask_samples_out(const jdsp_stftmask *h, long n_frames) { return h ? h->ola.samples_out(n_frames) : 0; }

int jdsp_stftmask_process_dev(jdsp_stftmask *h, const int16_t *pcm_dev, const void *mask_dev, long mask_pitch,
                              long n_frames, int16_t *out_i16_dev, float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_frames < 0) return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_process: n_frames < 0");
    if (mask_pitch != 0 && mask_pitch < kBins)
        return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_process: mask_pitch must be 0 (one row) or >= n_fft/2 + 1");
    if (!jdsp::aligned(pcm_dev, 4) || !jdsp::aligned(out_i16_dev, 4) || !jdsp::aligned(out_f32_dev, 8) ||
        !jdsp::aligned(mask_dev, mask_elem(h)))
        return fail(ctx, JDSP_EINVAL,
                    "jdsp_stftmask_process: pcm and out_i16 must be 4-byte, out_f32 8-byte aligned, the mask 4-byte "
                    "(REAL) or 8-byte (COMPLEX)");
    if (n_frames == 0) {
        h->count_valid = 0;                                    // a call of no frames recomputed none
        return JDSP_OK;
    }
    if (!pcm_dev || !mask_dev) return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_process: pcm or mask is NULL");
    OlaStream &o = h->ola;
    if (jdsp::launch_stftmask(ctx->stream, ctx->n_cu, h->cfg.hop, h->cfg.mask_kind == JDSP_MASK_COMPLEX, pcm_dev, mask_dev,
                              mask_pitch, n_frames, h->wa, h->ws, o.g, o.tail[o.cur], o.tail[o.cur ^ 1], out_i16_dev,
                              out_f32_dev, ctx->stft1024_table.get(), o.run_opt, h->f64.get(), h->count.get(),
                              h->next_epoch()))
        return fail(ctx, JDSP_EHIP, "jdsp_stftmask_process: launch", hipGetLastError());
    o.cur ^= 1;
    return JDSP_OK;
}

int jdsp_stftmask_flush_dev(jdsp_stftmask *h, int16_t *out_i16_dev, float *out_f32_dev)
{
    return h ? h->ola.flush_dev("jdsp_stftmask_flush", out_i16_dev, out_f32_dev) : JDSP_EINVAL;
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
    int16_t *d_i16 = nullptr;
    float *d_f32 = nullptr;
    hipError_t e = h->h_pcm.grow(n_pcm);
    if (e == hipSuccess) e = h->h_mask.grow(mask_bytes);
    if (e == hipSuccess) e = h->ola.stage_out(n_out, out_i16_host, out_f32_host, d_i16, d_f32);
    if (e != hipSuccess) return fail(ctx, JDSP_EHIP, "jdsp_stftmask_process: buffers", e);
    jdsp::HostCall hc(ctx, "jdsp_stftmask_process");                    // the buffers are the handle's
    hc.upload_to(h->h_pcm.get(), pcm_host, n_pcm * sizeof(int16_t));
    hc.upload_to(h->h_mask.get(), mask_host, mask_bytes);
    if (hc.ok())
        hc.result(jdsp_stftmask_process_dev(h, h->h_pcm.get(), h->h_mask.get(), mask_pitch, n_frames, d_i16, d_f32));
    h->ola.download_out(hc, n_out, out_i16_host, out_f32_host);
    return hc.finish();
}

int jdsp_stftmask_flush(jdsp_stftmask *h, int16_t *out_i16_host, float *out_f32_host)
{
    return h ? h->ola.flush("jdsp_stftmask_flush", out_i16_host, out_f32_host) : JDSP_EINVAL;
}

int jdsp_stftmask_batch_dev(jdsp_stftmask *h, const int16_t *pcm_dev, const void *mask_dev, long mask_pitch,
                            const int64_t *sample_first_dev, const int64_t *frame_first_dev, long n_utts,
                            long n_frames_total, int16_t *out_i16_dev, float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    return ragged_dev(h, nullptr, pcm_dev, mask_dev, mask_pitch, nullptr, sample_first_dev, frame_first_dev, n_utts,
                      n_frames_total, out_i16_dev, out_f32_dev);
}

int jdsp_stftmask_batch(jdsp_stftmask *h, const int16_t *pcm_host, long n_samples, const void *mask_host, long mask_pitch,
                        const int64_t *sample_first_host, const int64_t *frame_first_host, long n_utts,
                        int16_t *out_i16_host, float *out_f32_host)
{
    if (!h) return JDSP_EINVAL;
    return ragged_host(h, nullptr, pcm_host, n_samples, mask_host, mask_pitch, nullptr, sample_first_host, frame_first_host,
                       n_utts, out_i16_host, out_f32_host);
}

// ---- live streams ---------------------------------------------------------------------------------------------------

int jdsp_stftmask_streams_reserve(jdsp_stftmask *h, long n_streams)
{
    return h ? h->live.reserve("jdsp_stftmask_streams_reserve", n_streams) : JDSP_EINVAL;
}

int jdsp_stftmask_streams_reset_dev(jdsp_stftmask *h, const int64_t *stream_id_dev, long n_ids)
{
    return h ? h->live.reset_dev("jdsp_stftmask_streams_reset", stream_id_dev, n_ids) : JDSP_EINVAL;
}

int jdsp_stftmask_streams_dev(jdsp_stftmask *h, const int16_t *pcm_dev, const void *mask_dev, long mask_pitch,
                              const int64_t *stream_id_dev, const int64_t *sample_first_dev,
                              const int64_t *frame_first_dev, long n_chunks, long n_frames_total, int16_t *out_i16_dev,
                              float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    return ragged_dev(h, &h->live, pcm_dev, mask_dev, mask_pitch, stream_id_dev, sample_first_dev, frame_first_dev, n_chunks,
                      n_frames_total, out_i16_dev, out_f32_dev);
}

int jdsp_stftmask_streams_flush_dev(jdsp_stftmask *h, const int64_t *stream_id_dev, const int64_t *sample_first_dev,
                                    long n_ids, int16_t *out_i16_dev, float *out_f32_dev)
{
    return h ? h->live.flush_dev("jdsp_stftmask_streams_flush", stream_id_dev, sample_first_dev, n_ids, out_i16_dev,
                                 out_f32_dev)
             : JDSP_EINVAL;
}

int jdsp_stftmask_streams(jdsp_stftmask *h, const int16_t *pcm_host, long n_samples, const void *mask_host,
                          long mask_pitch, const int64_t *stream_id_host, const int64_t *sample_first_host,
                          const int64_t *frame_first_host, long n_chunks, int16_t *out_i16_host, float *out_f32_host)
{
    if (!h) return JDSP_EINVAL;
    return ragged_host(h, &h->live, pcm_host, n_samples, mask_host, mask_pitch, stream_id_host, sample_first_host,
                       frame_first_host, n_chunks, out_i16_host, out_f32_host);
}

int jdsp_stftmask_streams_flush(jdsp_stftmask *h, const int64_t *stream_id_host, const int64_t *sample_first_host,
                                long n_ids, long n_samples, int16_t *out_i16_host, float *out_f32_host)
{
    return h ? h->live.flush("jdsp_stftmask_streams_flush", stream_id_host, sample_first_host, n_ids, n_samples,
                             out_i16_host, out_f32_host)
             : JDSP_EINVAL;
}

}  // extern "C"
