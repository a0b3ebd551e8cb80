// reverb_live_api.hip -- C ABI of the live reverberation streams (include/jdsp.h "live reverberation streams"; the
// kernels: reverb_live_kernels.hip).  The entries share the handle's bank and nothing of its batch workspace.
#include "reverb.h"

using jdsp::fail;

static int live_open(jdsp_reverb *h, const char *what)
{
    if (h->lws.n_streams) return JDSP_OK;
    return fail(h->ctx, JDSP_EINVAL, (std::string(what) + ": no live streams (call jdsp_reverb_streams_reserve first)").c_str());
}

// every stream fresh: no block seen, a silent last block.  The ring needs nothing: a row is written before the walk
// of a later block reaches it.
static hipError_t live_zero(jdsp_reverb *h)
{
    jdsp_reverb::LiveWs &w = h->lws;
    hipError_t e = hipMemsetAsync(w.seen.get(), 0, w.seen.count() * sizeof(long long), h->ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(w.last.get(), 0, w.last.count() * sizeof(short), h->ctx->stream);
    return e;
}

// the scalar checks both entries make before anything else
int jdsp::reverb_live_counts(jdsp_reverb *h, const char *what, long n_chunks, long n_blocks_total)
{
    jdsp_ctx *ctx = h->ctx;
    int rc = live_open(h, what);
    if (rc) return rc;
    const std::string e(what);
    if (n_chunks < 0 || n_blocks_total < 0) return fail(ctx, JDSP_EINVAL, (e + ": n_chunks or the number of blocks < 0").c_str());
    if (n_chunks > h->lws.n_streams)
        return fail(ctx, JDSP_EINVAL, (e + ": more chunks than live streams (ids are distinct within a call)").c_str());
    if (n_blocks_total > h->lws.cap_blocks)
        return fail(ctx, JDSP_EINVAL, (e + ": more blocks than jdsp_reverb_streams_reserve sized the workspace for").c_str());
    return JDSP_OK;
}

extern "C" {

int jdsp_reverb_streams_reserve(jdsp_reverb *h, long n_streams, long max_blocks_total)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_streams < 1 || n_streams > 0x3fffffffL || max_blocks_total < 0 || max_blocks_total > 0x3ffffff0L)
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_streams_reserve: n_streams must be 1 .. 2^30 - 1, max_blocks_total 0 .. 2^30 - 16");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));          // nothing enqueued still uses the old buffers
    jdsp_reverb::LiveWs &w = h->lws;
    w = {};
    const size_t n = (size_t)n_streams, nb = (size_t)max_blocks_total, ring_rows = n * (size_t)(h->n_part - 1);
    hipError_t e = w.seen.alloc(n);
    if (e == hipSuccess) e = w.wave_first.alloc(n + 1);
    if (e == hipSuccess) e = w.last.alloc(n * jdsp::kReverbBlock);
    if (e == hipSuccess) e = w.ring.alloc((ring_rows ? ring_rows : 1) * jdsp::kUpolsRowPitch);
    if (e == hipSuccess) e = w.X.alloc((nb ? nb : 1) * jdsp::kUpolsRowPitch);
    if (e == hipSuccess) {
        w.view = {w.seen.get(), w.last.get(), w.ring.get(), w.X.get()};
        w.n_streams = n_streams;
        e = live_zero(h);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) {
        w = {};
        return fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_reverb_streams_reserve", e);
    }
    w.cap_blocks = max_blocks_total;
    return JDSP_OK;
}

int jdsp_reverb_streams_reset_dev(jdsp_reverb *h, const int64_t *stream_id_dev, long n_ids)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = live_open(h, "jdsp_reverb_streams_reset_dev");
    if (rc) return rc;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const jdsp_reverb::LiveWs &w = h->lws;
    if (!stream_id_dev) {
        JDSP_HIP(ctx, live_zero(h));
        return JDSP_OK;
    }
    if (n_ids < 0 || n_ids > w.n_streams)
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_streams_reset_dev: n_ids must be 0 .. n_streams (ids are distinct within a call)");
    if (!jdsp::aligned(stream_id_dev, 8)) return fail(ctx, JDSP_EINVAL, "jdsp_reverb_streams_reset_dev: stream_id must be 8-byte aligned");
    if (jdsp::launch_reverb_live_reset(ctx->stream, reinterpret_cast<const long long *>(stream_id_dev), n_ids, w.n_streams, w.view))
        return fail(ctx, JDSP_EHIP, "jdsp_reverb_streams_reset_dev: launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_reverb_streams_dev(jdsp_reverb *h, const int16_t *pcm_dev, const int64_t *stream_id_dev,
                            const int64_t *sample_first_dev, const int64_t *block_first_dev, const int32_t *ir_dev,
                            const float *gain_dev, long n_chunks, long n_blocks_total, int16_t *out_i16_dev, float *out_f32_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = jdsp::reverb_live_counts(h, "jdsp_reverb_streams_dev", n_chunks, n_blocks_total);
    if (rc) return rc;
    if (!jdsp::aligned(pcm_dev, 16) || !jdsp::aligned(out_i16_dev, 16) || !jdsp::aligned(out_f32_dev, 8) ||
        !jdsp::aligned(stream_id_dev, 8) || !jdsp::aligned(sample_first_dev, 8) || !jdsp::aligned(block_first_dev, 8) ||
        !jdsp::aligned(ir_dev, 4) || !jdsp::aligned(gain_dev, 4))
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_streams_dev: pcm and out_i16 must be 16-byte, out_f32, the stream ids and "
                                      "the offset arrays 8-byte, ir and gain 4-byte aligned");
    if (n_chunks == 0 || n_blocks_total == 0) return JDSP_OK;   // nothing launched, nothing changed
    if (!pcm_dev || !stream_id_dev || !sample_first_dev || !block_first_dev || !ir_dev)
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_streams_dev: pcm, stream_id, sample_first, block_first or ir is NULL");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const jdsp::ReverbLiveArgs a = {pcm_dev,
                                    reinterpret_cast<const long long *>(stream_id_dev),
                                    reinterpret_cast<const long long *>(sample_first_dev),
                                    reinterpret_cast<const long long *>(block_first_dev),
                                    ir_dev, gain_dev, n_chunks, n_blocks_total, out_i16_dev, out_f32_dev};
    if (jdsp::launch_reverb_live(ctx->stream, a, h->bank.get(), h->n_part, h->n_irs, ctx->stft1024_table_rect.get(),
                                 h->lws.view, h->lws.wave_first.get()))
        return fail(ctx, JDSP_EHIP, "jdsp_reverb_streams_dev: launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_reverb_streams(jdsp_reverb *h, const int16_t *pcm_host, long n_samples, const int64_t *stream_id_host,
                        const int64_t *sample_first_host, const int64_t *block_first_host, const int32_t *ir_host,
                        const float *gain_host, long n_chunks, int16_t *out_i16_host, float *out_f32_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    const char *me = "jdsp_reverb_streams";
    int rc = jdsp::reverb_live_counts(h, me, n_chunks, 0);
    if (rc) return rc;
    if (n_samples < 0) return fail(ctx, JDSP_EINVAL, "jdsp_reverb_streams: n_samples < 0");
    if (n_chunks > 0 && (!stream_id_host || !sample_first_host || !block_first_host || !ir_host))
        return fail(ctx, JDSP_EINVAL, "jdsp_reverb_streams: stream_id, sample_first, block_first or ir is NULL");
    const jdsp::StreamIdVerdict v = jdsp::stream_ids_check(stream_id_host, n_chunks, h->lws.n_streams);
    if (v != jdsp::StreamIdVerdict::kOk) return fail(ctx, JDSP_EINVAL, jdsp::stream_ids_message(v, me).c_str());
    return jdsp::reverb_host_call(h, me, true, pcm_host, n_samples, stream_id_host, sample_first_host, block_first_host, ir_host,
                                  gain_host, n_chunks, out_i16_host, out_f32_host);
}

int jdsp_reverb_streams_state(jdsp_reverb *h, const int64_t *stream_id_host, long n_ids, int64_t *blocks_seen_host,
                              int16_t *last_block_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = live_open(h, "jdsp_reverb_streams_state");
    if (rc) return rc;
    const jdsp_reverb::LiveWs &w = h->lws;
    if (n_ids < 0 || (n_ids > 0 && !stream_id_host)) return fail(ctx, JDSP_EINVAL, "jdsp_reverb_streams_state: bad argument");
    for (long i = 0; i < n_ids; i++)
        if (stream_id_host[i] < 0 || stream_id_host[i] >= w.n_streams)
            return fail(ctx, JDSP_EINVAL, "jdsp_reverb_streams_state: a stream id lies outside [0, n_streams)");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t B = jdsp::kReverbBlock;
    for (long i = 0; i < n_ids; i++) {
        const int64_t id = stream_id_host[i];
        if (blocks_seen_host)
            JDSP_HIP(ctx, hipMemcpyAsync(blocks_seen_host + i, w.view.seen + id, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        if (last_block_host)
            JDSP_HIP(ctx, hipMemcpyAsync(last_block_host + (size_t)i * B, w.view.last + (size_t)id * B, B * sizeof(int16_t),
                                         hipMemcpyDeviceToHost, s));
    }
    JDSP_HIP(ctx, hipStreamSynchronize(s));
    return JDSP_OK;
}

}  // extern "C"
