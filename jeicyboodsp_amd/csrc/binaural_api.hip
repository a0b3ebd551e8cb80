// binaural_api.hip -- C ABI of live binaural rendering (include/jdsp.h, "binaural rendering"; NOT a reference
// function: the reference's overlap-save convolver generalised to mixes of moving sources).
#include "binaural_layout.h"
#include "jdsp_internal.h"

using jdsp::fail;

static int bin_open(jdsp_binaural *h, const char *what)
{
    if (h->n_streams) return JDSP_OK;
    return fail(h->ctx, JDSP_EINVAL, (std::string(what) + ": no live streams (call jdsp_binaural_streams_reserve first)").c_str());
}

extern "C" {

int jdsp_binaural_create(jdsp_ctx *ctx, const double *hrir_taps, int n_dirs, int n_taps, jdsp_binaural **out)
{
    if (!ctx || !out) return JDSP_EINVAL;
    *out = nullptr;
    if (!hrir_taps || n_dirs < 1 || n_dirs > 16384 || n_taps < 1 || n_taps > 513)
        return fail(ctx, JDSP_EINVAL, "jdsp_binaural_create: 1 <= n_dirs <= 16384 directions of 2 x n_taps taps, 1 <= n_taps <= 513");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp::ensure_stft1024_table(ctx);
    if (rc) return rc;
    jdsp_binaural *h = new (std::nothrow) jdsp_binaural();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_binaural_create");
    h->ctx = ctx;
    h->n_dirs = n_dirs;
    h->n_taps = n_taps;
    const size_t rows = (size_t)n_dirs * 2;
    // H = FFT(h zero-padded to 1024), once, in double on the device (as jdsp_fastconv_create)
    std::vector<double> hpad(rows * 1024 * 2, 0.0);
    for (size_t r = 0; r < rows; r++)
        for (int i = 0; i < n_taps; i++) hpad[2 * (r * 1024 + i)] = hrir_taps[r * n_taps + i];
    const hipError_t e = h->bank.alloc(rows * 640);
    if (e != hipSuccess) rc = fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_binaural_create: alloc", e);
    if (!rc) {
        jdsp::HostCall hc(ctx, "jdsp_binaural_create");
        const double *d_h = hc.upload(hpad.data(), rows * 1024 * 16);
        double *d_H = hc.alloc<double>(rows * 1024 * 16);
        if (hc.ok()) hc.result(jdsp_fft_process_f64_dev(ctx, d_h, d_H, 1024, (long)rows, 1));
        if (hc.ok() && jdsp::launch_binaural_bank(ctx->stream, (const double2 *)d_H, h->bank.get(), (long)rows))
            hc.result(fail(ctx, JDSP_EHIP, "jdsp_binaural_create: bank launch", hipGetLastError()));
        rc = hc.finish();
    }
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_binaural_destroy(jdsp_binaural *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_binaural_n_dirs(const jdsp_binaural *h) { return h ? h->n_dirs : 0; }
int jdsp_binaural_block_len(const jdsp_binaural *h) { return h ? (int)jdsp::kBinauralBlock : 0; }

int jdsp_binaural_streams_reserve(jdsp_binaural *h, long n_streams)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_streams < 1 || n_streams > 0x3fffffffL)
        return fail(ctx, JDSP_EINVAL, "jdsp_binaural_streams_reserve: n_streams must be 1 .. 2^30 - 1");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));          // nothing enqueued still uses the old buffers
    h->n_streams = 0, h->parity = nullptr, h->view = {};
    const size_t n = (size_t)n_streams;
    // the state's parts in one allocation: histories, then the four kinds of words
    const size_t b_hist = 2 * n * 512 * sizeof(short), b_word = n * sizeof(int);
    hipError_t e = h->state.alloc(b_hist + 7 * b_word);
    // every stream fresh: zeros everywhere (both parities 0)
    if (e == hipSuccess) e = hipMemsetAsync(h->state.get(), 0, h->state.count(), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        h->state.reset();
        return fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_binaural_streams_reserve", e);
    }
    char *p = h->state.get();
    int *word = reinterpret_cast<int *>(p + b_hist);
    h->view = {reinterpret_cast<short *>(p), word, reinterpret_cast<float *>(word + 2 * n), word + 4 * n, n_streams};
    h->parity = word + 6 * n;
    h->n_streams = n_streams;
    return JDSP_OK;
}

int jdsp_binaural_streams_reset_dev(jdsp_binaural *h, const int64_t *stream_id_dev, long n_ids)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = bin_open(h, "jdsp_binaural_streams_reset_dev");
    if (rc) return rc;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (!stream_id_dev) {
        JDSP_HIP(ctx, hipMemsetAsync(h->state.get(), 0, h->state.count(), ctx->stream));
        return JDSP_OK;
    }
    if (n_ids < 0 || n_ids > h->n_streams)
        return fail(ctx, JDSP_EINVAL, "jdsp_binaural_streams_reset_dev: n_ids must be 0 .. n_streams (ids are distinct within a call)");
    if (!jdsp::aligned(stream_id_dev, 8)) return fail(ctx, JDSP_EINVAL, "jdsp_binaural_streams_reset_dev: stream_id must be 8-byte aligned");
    if (jdsp::launch_binaural_reset(ctx->stream, reinterpret_cast<const long long *>(stream_id_dev), n_ids, h->view))
        return fail(ctx, JDSP_EHIP, "jdsp_binaural_streams_reset_dev: launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_binaural_render_dev(jdsp_binaural *h, const int16_t *pcm_dev, const int64_t *stream_id_dev,
                             const int64_t *sample_first_dev, const int32_t *dir_dev, const float *gain_dev,
                             const int64_t *chunk_first_dev, const int64_t *block_first_dev, long n_mixes, long n_chunks,
                             long n_blocks_total, int16_t *out_i16_dev, float *out_f32_dev, long plane)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    const char *me = "jdsp_binaural_render_dev";
    int rc = bin_open(h, me);
    if (rc) return rc;
    if (n_mixes < 0 || n_chunks < 0 || n_blocks_total < 0)
        return fail(ctx, JDSP_EINVAL, "jdsp_binaural_render_dev: n_mixes, n_chunks or n_blocks_total < 0");
    if (n_chunks > h->n_streams)
        return fail(ctx, JDSP_EINVAL, "jdsp_binaural_render_dev: more chunks than live streams (ids are distinct within a call)");
    if (n_blocks_total > jdsp::kBinauralMaxBlocks)
        return fail(ctx, JDSP_EINVAL, "jdsp_binaural_render_dev: more than 2^30 - 16 blocks in one delivery");
    if (plane < 0 || (plane & 1)) return fail(ctx, JDSP_EINVAL, "jdsp_binaural_render_dev: plane must be even and >= 0");
    if ((out_i16_dev || out_f32_dev) && n_blocks_total > plane / jdsp::kBinauralBlock)
        return fail(ctx, JDSP_EINVAL, "jdsp_binaural_render_dev: the output blocks do not fit in plane");
    if (!jdsp::aligned(pcm_dev, 4) || !jdsp::aligned(out_i16_dev, 4) || !jdsp::aligned(out_f32_dev, 8) ||
        !jdsp::aligned(dir_dev, 4) || !jdsp::aligned(gain_dev, 4) || !jdsp::aligned(stream_id_dev, 8) ||
        !jdsp::aligned(sample_first_dev, 8) || !jdsp::aligned(chunk_first_dev, 8) || !jdsp::aligned(block_first_dev, 8))
        return fail(ctx, JDSP_EINVAL, "jdsp_binaural_render_dev: pcm, out_i16, dir and gain must be 4-byte, out_f32, the "
                                      "stream ids and the offset arrays 8-byte aligned");
    if (n_mixes == 0 || n_blocks_total == 0) return JDSP_OK;     // nothing launched, nothing changed
    if (!chunk_first_dev || !block_first_dev)
        return fail(ctx, JDSP_EINVAL, "jdsp_binaural_render_dev: chunk_first or block_first is NULL");
    if (n_chunks > 0 && (!pcm_dev || !stream_id_dev || !sample_first_dev || !dir_dev || !gain_dev))
        return fail(ctx, JDSP_EINVAL, "jdsp_binaural_render_dev: pcm, stream_id, sample_first, dir or gain is NULL");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (jdsp::launch_binaural_render(ctx->stream, pcm_dev, reinterpret_cast<const long long *>(stream_id_dev),
                                     reinterpret_cast<const long long *>(sample_first_dev), dir_dev, gain_dev,
                                     reinterpret_cast<const long long *>(chunk_first_dev),
                                     reinterpret_cast<const long long *>(block_first_dev), n_mixes, n_chunks,
                                     n_blocks_total, h->bank.get(), h->n_dirs, ctx->stft1024_table.get(), h->view,
                                     h->parity, out_i16_dev, out_f32_dev, plane))
        return fail(ctx, JDSP_EHIP, "jdsp_binaural_render_dev: launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_binaural_render(jdsp_binaural *h, const int16_t *pcm_host, long n_samples, const int64_t *stream_id_host,
                         const int64_t *sample_first_host, const int32_t *dir_host, const float *gain_host,
                         const int64_t *chunk_first_host, const int64_t *block_first_host, long n_mixes, long n_chunks,
                         int16_t *out_i16_host, float *out_f32_host, long plane)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    const char *me = "jdsp_binaural_render";
    int rc = bin_open(h, me);
    if (rc) return rc;
    const jdsp::BinauralDelivery d = {stream_id_host, sample_first_host, dir_host, gain_host, chunk_first_host,
                                      block_first_host, n_mixes, n_chunks, n_samples, plane,
                                      out_i16_host != nullptr || out_f32_host != nullptr};
    int64_t n_total = 0;
    const std::string bad = jdsp::binaural_delivery_check(d, h->n_streams, h->n_dirs, &n_total);
    if (!bad.empty()) return fail(ctx, JDSP_EINVAL, (std::string(me) + ": " + bad).c_str());
    if (n_chunks > 0 && n_total > 0 && !pcm_host) return fail(ctx, JDSP_EINVAL, "jdsp_binaural_render: pcm is NULL");
    // what no launch writes is zero
    if (out_i16_host && plane) memset(out_i16_host, 0, (size_t)plane * 2 * sizeof(int16_t));
    if (out_f32_host && plane) memset(out_f32_host, 0, (size_t)plane * 2 * sizeof(float));
    if (n_total == 0) return JDSP_OK;                          // nothing to launch
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    jdsp::HostCall hc(ctx, me);
    const size_t nm = (size_t)n_mixes + 1, nc = (size_t)n_chunks;
    const int64_t *d_cf = hc.upload(chunk_first_host, nm * sizeof(int64_t));
    const int64_t *d_bf = hc.upload(block_first_host, nm * sizeof(int64_t));
    // the four per-chunk arrays in one buffer (HostCall owns eight): ids, sample_first, dir, gain
    char *d_chunk = hc.alloc<char>(nc * 24);
    hc.upload_to(d_chunk, stream_id_host, nc * 8);
    hc.upload_to(d_chunk + nc * 8, sample_first_host, nc * 8);
    hc.upload_to(d_chunk + nc * 16, dir_host, nc * 4);
    hc.upload_to(d_chunk + nc * 20, gain_host, nc * 4);
    const int16_t *d_pcm = nc ? hc.upload(pcm_host, (size_t)n_samples * sizeof(int16_t)) : nullptr;
    const size_t out_n = (size_t)plane * 2;
    int16_t *d_o16 = out_i16_host ? hc.alloc<int16_t>(out_n * sizeof(int16_t)) : nullptr;
    float *d_o32 = out_f32_host ? hc.alloc<float>(out_n * sizeof(float)) : nullptr;
    if (d_o16) hc.zero(d_o16, out_n * sizeof(int16_t));
    if (d_o32) hc.zero(d_o32, out_n * sizeof(float));
    if (hc.ok())
        hc.result(jdsp_binaural_render_dev(h, d_pcm, reinterpret_cast<const int64_t *>(d_chunk),
                                           reinterpret_cast<const int64_t *>(d_chunk + nc * 8),
                                           reinterpret_cast<const int32_t *>(d_chunk + nc * 16),
                                           reinterpret_cast<const float *>(d_chunk + nc * 20), d_cf, d_bf, n_mixes, n_chunks,
                                           (long)n_total, d_o16, d_o32, plane));
    hc.download(out_i16_host, d_o16, d_o16 ? out_n * sizeof(int16_t) : 0);
    hc.download(out_f32_host, d_o32, d_o32 ? out_n * sizeof(float) : 0);
    return hc.finish();
}

int jdsp_binaural_streams_state(jdsp_binaural *h, const int64_t *stream_id_host, long n_ids, int16_t *hist_host,
                                int32_t *dir_host, float *gain_host, int32_t *started_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = bin_open(h, "jdsp_binaural_streams_state");
    if (rc) return rc;
    if (n_ids < 0 || (n_ids > 0 && !stream_id_host)) return fail(ctx, JDSP_EINVAL, "jdsp_binaural_streams_state: bad argument");
    for (long i = 0; i < n_ids; i++)
        if (stream_id_host[i] < 0 || stream_id_host[i] >= h->n_streams)
            return fail(ctx, JDSP_EINVAL, "jdsp_binaural_streams_state: a stream id lies outside [0, n_streams)");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const jdsp::BinauralStreams &v = h->view;
    for (long i = 0; i < n_ids; i++) {
        const int64_t id = stream_id_host[i];
        int p = 0;
        JDSP_HIP(ctx, hipMemcpyAsync(&p, h->parity + id, sizeof(int), hipMemcpyDeviceToHost, s));
        JDSP_HIP(ctx, hipStreamSynchronize(s));
        const size_t at = (size_t)(p & 1) * h->n_streams + id;
        if (hist_host)
            JDSP_HIP(ctx, hipMemcpyAsync(hist_host + (size_t)i * 512, v.hist + at * 512, 512 * sizeof(int16_t), hipMemcpyDeviceToHost, s));
        if (dir_host) JDSP_HIP(ctx, hipMemcpyAsync(dir_host + i, v.dir + at, sizeof(int), hipMemcpyDeviceToHost, s));
        if (gain_host) JDSP_HIP(ctx, hipMemcpyAsync(gain_host + i, v.gain + at, sizeof(float), hipMemcpyDeviceToHost, s));
        if (started_host) JDSP_HIP(ctx, hipMemcpyAsync(started_host + i, v.started + at, sizeof(int), hipMemcpyDeviceToHost, s));
    }
    JDSP_HIP(ctx, hipStreamSynchronize(s));
    return JDSP_OK;
}

}  // extern "C"
