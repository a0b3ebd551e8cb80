// mvdrn_live_api.hip -- C ABI of the live streams of the n-microphone MVDR beamformer (include/jdsp.h "live n-microphone
// MVDR streams"; the kernels: mvdrn_live_kernels.hip).  The entries share the handle's configuration (n_mics, steering,
// loading, the VAD's window) and nothing of its own stream or of its batch workspace.
#include "jdsp_internal.h"

using jdsp::fail;

static int live_supported(jdsp_mvdrn *h, const char *what)
{
    if (h->n_fft == 1024) return JDSP_OK;
    return fail(h->ctx, JDSP_EINVAL, (std::string(what) + ": 1024-point handles only; a 512-point handle pairs two blocks "
                                      "in one inverse transform, which is not built across chunk boundaries").c_str());
}

static int live_open(jdsp_mvdrn *h, const char *what)
{
    int rc = live_supported(h, what);
    if (rc) return rc;
    if (h->lws.n_streams) return JDSP_OK;
    return fail(h->ctx, JDSP_EINVAL, (std::string(what) + ": no live streams (call jdsp_mvdrn_streams_reserve first)").c_str());
}

// every stream fresh: zeros everywhere
static hipError_t live_zero(jdsp_mvdrn *h)
{
    return hipMemsetAsync(h->lws.state.get(), 0, h->lws.state.count(), h->ctx->stream);
}

// the scalar checks both entries make before anything else
static int live_counts(jdsp_mvdrn *h, const char *what, long n_chunks, long n_blocks_total)
{
    jdsp_ctx *ctx = h->ctx;
    int rc = live_open(h, what);
    if (rc) return rc;
    const std::string e(what);
    if (n_chunks < 0 || n_blocks_total < 0) return fail(ctx, JDSP_EINVAL, (e + ": n_chunks or the number of blocks < 0").c_str());
    if (n_chunks > h->lws.n_streams)
        return fail(ctx, JDSP_EINVAL, (e + ": more chunks than live streams (ids are distinct within a call)").c_str());
    if (n_blocks_total > h->lws.cap_blocks)
        return fail(ctx, JDSP_EINVAL, (e + ": more blocks than jdsp_mvdrn_streams_reserve sized the workspace for").c_str());
    return JDSP_OK;
}

extern "C" {

int jdsp_mvdrn_streams_reserve(jdsp_mvdrn *h, long n_streams, long max_blocks_total)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = live_supported(h, "jdsp_mvdrn_streams_reserve");
    if (rc) return rc;
    if (n_streams < 1 || n_streams > 0x3fffffffL || max_blocks_total < 0 || max_blocks_total > 0x3ffffff0L)
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams_reserve: n_streams must be 1 .. 2^30 - 1, max_blocks_total 0 .. 2^30 - 16");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));          // nothing enqueued still uses the old buffers
    jdsp_mvdrn::LiveWs &w = h->lws;
    w = {};
    const size_t n = (size_t)n_streams, nb = (size_t)max_blocks_total, bins = (size_t)h->n_bins;
    // the state's parts in one allocation, the widest alignment first
    const size_t b_cov = n * bins * 64 * sizeof(double2), b_prev = n * 8 * 512 * sizeof(short),
                 b_seen = n * sizeof(long long), b_quiet = n * sizeof(int);
    hipError_t e = w.state.alloc(b_cov + b_prev + b_seen + b_quiet);
    if (e == hipSuccess) e = w.code.alloc(nb + 1);
    if (e == hipSuccess) e = w.row.alloc(nb + 1);
    if (e == hipSuccess) e = w.events.alloc(nb + 1);
    if (e == hipSuccess) e = w.ev_n.alloc(n);
    // worst case: every block is an estimation frame -- one spectrum set and one weight set per block, as
    // jdsp_mvdrn_batch_reserve, and one weight set per chunk on top: the row that solves the matrix carried in
    if (e == hipSuccess) e = w.spec.alloc((nb + 1) * h->n_mics * bins);
    if (e == hipSuccess) e = w.weights.alloc((nb + n + 1) * bins * 8);
    if (e == hipSuccess) {
        char *p = w.state.get();
        double2 *cov = reinterpret_cast<double2 *>(p);
        p += b_cov;
        short *prev = reinterpret_cast<short *>(p);
        p += b_prev;
        long long *seen = reinterpret_cast<long long *>(p);
        p += b_seen;
        w.view = {cov, prev, seen, reinterpret_cast<int *>(p), n_streams, w.code.get(), w.row.get(), w.events.get(),
                  w.ev_n.get(), w.spec.get(), w.weights.get()};
        w.n_streams = n_streams;
        e = live_zero(h);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) {
        w = {};
        return fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_mvdrn_streams_reserve", e);
    }
    w.cap_blocks = max_blocks_total;
    return JDSP_OK;
}

int jdsp_mvdrn_streams_reset_dev(jdsp_mvdrn *h, const int64_t *stream_id_dev, long n_ids)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = live_open(h, "jdsp_mvdrn_streams_reset_dev");
    if (rc) return rc;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const jdsp_mvdrn::LiveWs &w = h->lws;
    if (!stream_id_dev) {
        JDSP_HIP(ctx, live_zero(h));
        return JDSP_OK;
    }
    if (n_ids < 0 || n_ids > w.n_streams)
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams_reset_dev: n_ids must be 0 .. n_streams (ids are distinct within a call)");
    if (!jdsp::aligned(stream_id_dev, 8)) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams_reset_dev: stream_id must be 8-byte aligned");
    if (jdsp::launch_mvdrn_live_reset(ctx->stream, reinterpret_cast<const long long *>(stream_id_dev), n_ids, w.view))
        return fail(ctx, JDSP_EHIP, "jdsp_mvdrn_streams_reset_dev: launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_mvdrn_streams_dev(jdsp_mvdrn *h, const int16_t *pcm_dev, long chan_stride, const int64_t *stream_id_dev,
                           const int64_t *sample_first_dev, const int64_t *block_first_dev, long n_chunks,
                           long n_blocks_total, int16_t *out_dev, float *precast_dev, uint8_t *flags_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = live_counts(h, "jdsp_mvdrn_streams_dev", n_chunks, n_blocks_total);
    if (rc) return rc;
    if (!jdsp::aligned(pcm_dev, 16) || (chan_stride & 7) || !jdsp::aligned(out_dev, 4) || !jdsp::aligned(precast_dev, 4) ||
        !jdsp::aligned(stream_id_dev, 8) || !jdsp::aligned(sample_first_dev, 8) || !jdsp::aligned(block_first_dev, 8))
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams_dev: pcm must be 16-byte aligned and chan_stride a multiple of 8; "
                                      "out and precast 4-byte, the stream ids and the offset arrays 8-byte aligned");
    if (n_chunks == 0 || n_blocks_total == 0) return JDSP_OK;   // nothing launched, nothing changed
    if (!pcm_dev || !stream_id_dev || !sample_first_dev || !block_first_dev)
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams_dev: pcm, stream_id, sample_first or block_first is NULL");
    if (chan_stride < 0) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams_dev: chan_stride < 0");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (jdsp::launch_mvdrn_live(ctx->stream, pcm_dev, chan_stride, h->n_mics,
                                reinterpret_cast<const long long *>(stream_id_dev),
                                reinterpret_cast<const long long *>(sample_first_dev),
                                reinterpret_cast<const long long *>(block_first_dev), n_chunks, n_blocks_total,
                                h->w_vad.get(), h->steer.get(), h->loading, ctx->stft1024_table.get(), h->lws.view,
                                flags_dev, out_dev, precast_dev))
        return fail(ctx, JDSP_EHIP, "jdsp_mvdrn_streams_dev: launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_mvdrn_streams(jdsp_mvdrn *h, const int16_t *pcm_host, long chan_stride, long n_samples,
                       const int64_t *stream_id_host, const int64_t *sample_first_host, const int64_t *block_first_host,
                       long n_chunks, int16_t *out_host, float *precast_host, uint8_t *flags_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    const char *me = "jdsp_mvdrn_streams";
    int rc = live_counts(h, me, n_chunks, 0);
    if (rc) return rc;
    if (n_samples < 0 || chan_stride < n_samples)
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams: n_samples < 0 or chan_stride < n_samples");
    if (n_chunks > 0 && (!stream_id_host || !sample_first_host || !block_first_host))
        return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams: stream_id, sample_first or block_first is NULL");
    const jdsp::StreamIdVerdict v = jdsp::stream_ids_check(stream_id_host, n_chunks, h->lws.n_streams);
    if (v != jdsp::StreamIdVerdict::kOk) return fail(ctx, JDSP_EINVAL, jdsp::stream_ids_message(v, me).c_str());
    jdsp::RaggedOffsets offs;                                  // a span of b blocks is b hops: n = hop
    if (offs.check(ctx, me, "block_first", sample_first_host, block_first_host, n_chunks, n_samples, h->block, h->block))
        return JDSP_EINVAL;
    const long n_total = offs.lay.n_total, end = offs.lay.end;
    rc = live_counts(h, me, n_chunks, n_total);
    if (rc) return rc;
    // what no launch writes is zero
    if (out_host && n_samples) memset(out_host, 0, (size_t)n_samples * sizeof(int16_t));
    if (precast_host && n_samples) memset(precast_host, 0, (size_t)n_samples * sizeof(float));
    if (n_total == 0) return JDSP_OK;                          // nothing to launch
    if (!pcm_host) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams: pcm is NULL");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const long stride_dev = (end + 7) & ~7L;                   // the planes repacked: nothing past the last span is read
    jdsp::HostCall hc(ctx, me);
    offs.upload(hc);
    const int64_t *d_id = hc.upload(stream_id_host, (size_t)n_chunks * sizeof(int64_t));
    int16_t *d_pcm = hc.alloc<int16_t>((size_t)stride_dev * h->n_mics * sizeof(int16_t));
    for (int m = 0; m < h->n_mics; m++)
        hc.upload_to(d_pcm + (size_t)m * stride_dev, pcm_host + (size_t)m * chan_stride, (size_t)end * sizeof(int16_t));
    int16_t *d_out = out_host ? hc.alloc<int16_t>((size_t)end * sizeof(int16_t)) : nullptr;
    float *d_pre = precast_host ? hc.alloc<float>((size_t)end * sizeof(float)) : nullptr;
    uint8_t *d_flags = flags_host ? hc.alloc<uint8_t>((size_t)n_total) : nullptr;
    if (d_out) hc.zero(d_out, (size_t)end * sizeof(int16_t));
    if (d_pre) hc.zero(d_pre, (size_t)end * sizeof(float));
    if (hc.ok())
        hc.result(jdsp_mvdrn_streams_dev(h, d_pcm, stride_dev, d_id, offs.d_sample, offs.d_unit, n_chunks, n_total, d_out,
                                         d_pre, d_flags));
    hc.download(out_host, d_out, d_out ? (size_t)end * sizeof(int16_t) : 0);
    hc.download(precast_host, d_pre, d_pre ? (size_t)end * sizeof(float) : 0);
    hc.download(flags_host, d_flags, (size_t)n_total);
    return hc.finish();
}

int jdsp_mvdrn_streams_state(jdsp_mvdrn *h, const int64_t *stream_id_host, long n_ids, int64_t *blocks_seen_host,
                             double *cov_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = live_open(h, "jdsp_mvdrn_streams_state");
    if (rc) return rc;
    const jdsp_mvdrn::LiveWs &w = h->lws;
    if (n_ids < 0 || (n_ids > 0 && !stream_id_host)) return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams_state: bad argument");
    for (long i = 0; i < n_ids; i++)
        if (stream_id_host[i] < 0 || stream_id_host[i] >= w.n_streams)
            return fail(ctx, JDSP_EINVAL, "jdsp_mvdrn_streams_state: a stream id lies outside [0, n_streams)");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t per = (size_t)h->n_bins * 64;                    // double2 per stream
    for (long i = 0; i < n_ids; i++) {
        const int64_t id = stream_id_host[i];
        if (blocks_seen_host)
            JDSP_HIP(ctx, hipMemcpyAsync(blocks_seen_host + i, w.view.seen + id, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        if (cov_host)
            JDSP_HIP(ctx, hipMemcpyAsync(cov_host + (size_t)i * per * 2, w.view.cov + (size_t)id * per, per * sizeof(double2),
                                         hipMemcpyDeviceToHost, s));
    }
    JDSP_HIP(ctx, hipStreamSynchronize(s));
    return JDSP_OK;
}

}  // extern "C"
