// ola_api.h -- the host side of the two handles with an overlap-add output stream, jdsp_istft (istft_api.hip) and
// jdsp_stftmask (stftmask_api.hip), and of nobody else: the stream a handle carries between calls (OlaStream), its live
// streams (OlaStreams) and the one layer under the four ragged entries of each handle, jdsp_*_batch[_dev] and
// jdsp_*_streams[_dev] (ragged_call_check, ragged_host_call).  The kernels' side of the stream is ola_stream.h, the
// kernels' walk over ragged spans ragged_batch.h; the launchers and LiveStreams, which kernels and API both see, are in
// jdsp_internal.h.
#pragma once

#include "jdsp_internal.h"

namespace jdsp {

// What a jdsp_istft or jdsp_stftmask handle carries of its overlap-add output stream between calls (the kernels' side
// and the stream's rules: ola_stream.h): the emission gain, the ping-pong tail, the "frames_per_wave" option and the
// host entries' output staging.  `entry` is the calling entry's name, the prefix of its messages.
struct OlaStream {
    jdsp_ctx *ctx = nullptr;
    int n = 0, hop = 0;
    float *g = nullptr, *tail[2] = {nullptr, nullptr};   // views into the handle's blob: g[hop], tail[2][n]
    int cur = 0;                          // tail[cur] holds the partial sums the next call starts from
    int run_opt = 0;                      // "frames_per_wave": 0 = auto
    // host entry points' device buffers, grown on demand (those entries end with a synchronise: none is in use then)
    DevBuf<int16_t> h_i16;
    DevBuf<float> h_f32;

    // "stft.window"'s formulas (fill_stft1024_table / fill_win512): PI 3.141592 as the reference writes it
    static double window_at(int kind, int i, int n)
    {
        if (kind == JDSP_WIN_NONE) return 1.0;
        const double a = kind == JDSP_WIN_HANN ? 0.5 : 0.54, b = kind == JDSP_WIN_HANN ? 0.5 : 0.46;
        return a - b * cos(2 * 3.141592 * i / (n - 1));
    }
    // WOLA: gain[i] = 1 / sum_r w_a[i + r hop] w_s[i + r hop], i < hop; 1 when not normalising.  false: the windows'
    // overlap-add vanishes somewhere (no WOLA inverse), for the caller to report
    static bool wola_gain(int wa_kind, int ws_kind, int n, int hop, bool normalise, float *gain)
    {
        std::vector<double> den((size_t)hop, 1.0);
        if (normalise) {
            double mx = 0;
            for (int i = 0; i < hop; i++) {
                double s = 0;
                for (int r = 0; r < n / hop; r++)
                    s += window_at(wa_kind, i + r * hop, n) * window_at(ws_kind, i + r * hop, n);
                den[i] = s;
                mx = s > mx ? s : mx;
            }
            for (int i = 0; i < hop; i++)
                if (!(den[i] >= 1e-6 * mx)) return false;
        }
        for (int i = 0; i < hop; i++) gain[i] = (float)(1.0 / den[i]);
        return true;
    }
    // the stream's share of the handle's blob, the gain first
    static size_t floats(int n, int hop) { return (size_t)hop + 2 * (size_t)n; }
    void attach(jdsp_ctx *c, int n_fft, int hop_len, float *base)
    {
        ctx = c, n = n_fft, hop = hop_len;
        g = base, tail[0] = g + hop, tail[1] = tail[0] + n;
    }
    long least_run() const { return n / hop > 1 ? n / hop - 1 : 1; }     // max(R - 1, 1): the halo stays above frame 0
    long samples_out(long n_frames) const { return n_frames < 0 ? 0 : n_frames * hop; }
    int reset()
    {
        JDSP_HIP(ctx, hipMemsetAsync(tail[0], 0, 2 * (size_t)n * sizeof(float), ctx->stream));
        cur = 0;
        return JDSP_OK;
    }
    // before the handle is deleted: the stream's work on its memory is done
    void drain() const
    {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    // the n - hop samples still in the tail (g[t mod hop] * s[t], the same cast), then the reset
    int flush_dev(const char *entry, int16_t *out_i16_dev, float *out_f32_dev)
    {
        const std::string e(entry);
        if (!aligned(out_i16_dev, 4) || !aligned(out_f32_dev, 8))
            return fail(ctx, JDSP_EINVAL, (e + ": out_i16 must be 4-byte, out_f32 8-byte aligned").c_str());
        if (launch_istft_flush(ctx->stream, tail[cur], g, n - hop, hop, out_i16_dev, out_f32_dev))
            return fail(ctx, JDSP_EHIP, (e + ": launch").c_str(), hipGetLastError());
        return reset();
    }
    // The output half of a host entry: device staging for n_samples of each output the caller wants (d_* NULL where
    // it wants none, or for no samples), and after the *_dev call the copies back.
    hipError_t stage_out(size_t n_samples, const void *want_i16, const void *want_f32, int16_t *&d_i16, float *&d_f32)
    {
        hipError_t e = hipSuccess;
        if (n_samples && want_i16) e = h_i16.grow(n_samples);
        if (e == hipSuccess && n_samples && want_f32) e = h_f32.grow(n_samples);
        d_i16 = n_samples && want_i16 ? h_i16.get() : nullptr;
        d_f32 = n_samples && want_f32 ? h_f32.get() : nullptr;
        return e;
    }
    void download_out(HostCall &hc, size_t n_samples, int16_t *out_i16_host, float *out_f32_host) const
    {
        hc.download(out_i16_host, h_i16.get(), n_samples * sizeof(int16_t));
        hc.download(out_f32_host, h_f32.get(), n_samples * sizeof(float));
    }
    int flush(const char *entry, int16_t *out_i16_host, float *out_f32_host)
    {
        const size_t n_tail = (size_t)(n - hop);
        JDSP_HIP(ctx, hipSetDevice(ctx->device));
        int16_t *d_i16;
        float *d_f32;
        const hipError_t e = stage_out(n_tail, out_i16_host, out_f32_host, d_i16, d_f32);
        if (e != hipSuccess) return fail(ctx, JDSP_EHIP, (std::string(entry) + ": buffers").c_str(), e);
        HostCall hc(ctx, entry);
        hc.result(flush_dev(entry, d_i16, d_f32));
        download_out(hc, n_tail, out_i16_host, out_f32_host);
        return hc.finish();
    }
};

// The live streams of a jdsp_istft or jdsp_stftmask handle (jdsp_*_streams_*), next to its own OlaStream: n_streams
// tails carried from call to call, of which one call advances any subset by a chunk of frames each in one launch
// (LiveStreams in jdsp_internal.h, LiveSpan in ragged_batch.h).  Nothing here is read or written by the handle's own stream or by
// the stateless batch entries.  `entry` is the calling entry's name, the prefix of its messages.
struct OlaStreams {
    OlaStream *ola = nullptr;             // the handle's own: the context, n, hop, the gain and the output staging
    long n_streams = 0;                   // 0: not reserved
    DevBuf<float> tails;                  // [2][n_streams][n - hop]
    DevBuf<int> parity;                   // [n_streams]

    int n_tail() const { return ola->n - ola->hop; }
    LiveStreams view(const int64_t *stream_id_dev) const
    {
        return {reinterpret_cast<const long long *>(stream_id_dev), parity.get(), tails.get(), n_streams, n_tail()};
    }
    int closed(const char *entry) const
    {
        return fail(ola->ctx, JDSP_EINVAL, (std::string(entry) + ": no live streams (call _streams_reserve first)").c_str());
    }
    // the only call that allocates; every stream is fresh afterwards
    int reserve(const char *entry, long n)
    {
        jdsp_ctx *ctx = ola->ctx;
        const std::string e(entry);
        if (n < 1) return fail(ctx, JDSP_EINVAL, (e + ": n_streams must be >= 1").c_str());
        JDSP_HIP(ctx, hipSetDevice(ctx->device));
        JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // nothing enqueued still uses the old buffers
        n_streams = 0;
        const size_t n_floats = 2 * (size_t)n * (size_t)n_tail();
        hipError_t err = tails.alloc(n_floats ? n_floats : 1);
        if (err == hipSuccess) err = parity.alloc((size_t)n);
        if (err == hipSuccess) err = hipMemsetAsync(tails.get(), 0, tails.count() * sizeof(float), ctx->stream);
        if (err == hipSuccess) err = hipMemsetAsync(parity.get(), 0, (size_t)n * sizeof(int), ctx->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
        if (err != hipSuccess) {
            tails.reset();
            parity.reset();
            return fail(ctx, err == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, (e + ": buffers").c_str(), err);
        }
        n_streams = n;
        return JDSP_OK;
    }
    // the checks every entry over a list of ids makes before anything else: reserved, 0 <= n_ids <= n_streams
    int check_count(const char *entry, long n_ids) const
    {
        if (!n_streams) return closed(entry);
        const std::string e(entry);
        if (n_ids < 0) return fail(ola->ctx, JDSP_EINVAL, (e + ": a count is < 0").c_str());
        if (n_ids > n_streams)
            return fail(ola->ctx, JDSP_EINVAL, (e + ": more ids than live streams (ids are distinct within a call)").c_str());
        return JDSP_OK;
    }
    // host arrays only: every id in range, none twice
    int check_ids(const char *entry, const int64_t *stream_id_host, long n_ids) const
    {
        const StreamIdVerdict v = stream_ids_check(stream_id_host, n_ids, n_streams);
        return v == StreamIdVerdict::kOk ? JDSP_OK : fail(ola->ctx, JDSP_EINVAL, stream_ids_message(v, entry).c_str());
    }
    // the listed streams fresh again; stream_id_dev NULL: all of them
    int reset_dev(const char *entry, const int64_t *stream_id_dev, long n_ids)
    {
        jdsp_ctx *ctx = ola->ctx;
        if (!n_streams) return closed(entry);
        const std::string e(entry);
        if (!stream_id_dev) {
            JDSP_HIP(ctx, hipMemsetAsync(tails.get(), 0, tails.count() * sizeof(float), ctx->stream));
            JDSP_HIP(ctx, hipMemsetAsync(parity.get(), 0, (size_t)n_streams * sizeof(int), ctx->stream));
            return JDSP_OK;
        }
        if (int rc = check_count(entry, n_ids)) return rc;
        if (!aligned(stream_id_dev, 8)) return fail(ctx, JDSP_EINVAL, (e + ": stream_id must be 8-byte aligned").c_str());
        if (launch_ola_streams_flush(ctx->stream, view(stream_id_dev), n_ids, nullptr, ola->g, ola->hop, nullptr, nullptr))
            return fail(ctx, JDSP_EHIP, (e + ": launch").c_str(), hipGetLastError());
        return JDSP_OK;
    }
    // the n - hop samples still in each listed stream's tail, at sample_first[i] onwards, then its reset
    int flush_dev(const char *entry, const int64_t *stream_id_dev, const int64_t *sample_first_dev, long n_ids,
                  int16_t *out_i16_dev, float *out_f32_dev)
    {
        jdsp_ctx *ctx = ola->ctx;
        if (int rc = check_count(entry, n_ids)) return rc;
        const std::string e(entry);
        if (!aligned(stream_id_dev, 8) || !aligned(sample_first_dev, 8) || !aligned(out_i16_dev, 4) || !aligned(out_f32_dev, 8))
            return fail(ctx, JDSP_EINVAL,
                        (e + ": stream_id, sample_first and out_f32 must be 8-byte, out_i16 4-byte aligned").c_str());
        if (n_ids == 0) return JDSP_OK;
        if (!stream_id_dev || ((out_i16_dev || out_f32_dev) && !sample_first_dev))
            return fail(ctx, JDSP_EINVAL, (e + ": stream_id or sample_first is NULL").c_str());
        if (launch_ola_streams_flush(ctx->stream, view(stream_id_dev), n_ids,
                                     reinterpret_cast<const long long *>(sample_first_dev), ola->g, ola->hop, out_i16_dev,
                                     out_f32_dev))
            return fail(ctx, JDSP_EHIP, (e + ": launch").c_str(), hipGetLastError());
        return JDSP_OK;
    }
    // behind the transform launch over the chunks: the streams that were given frames carry their new tails
    int commit(const char *entry, const int64_t *stream_id_dev, const int64_t *frame_first_dev, long n_chunks)
    {
        if (launch_ola_streams_commit(ola->ctx->stream, reinterpret_cast<const long long *>(stream_id_dev),
                                      reinterpret_cast<const long long *>(frame_first_dev), n_chunks, parity.get()))
            return fail(ola->ctx, JDSP_EHIP, (std::string(entry) + ": commit launch").c_str(), hipGetLastError());
        return JDSP_OK;
    }
    // host pointers, synchronous: checks the ids and the n - hop long spans (even, ascending, disjoint, inside
    // n_samples); the outputs are n_samples long and zero outside the spans
    int flush(const char *entry, const int64_t *stream_id_host, const int64_t *sample_first_host, long n_ids,
              long n_samples, int16_t *out_i16_host, float *out_f32_host)
    {
        jdsp_ctx *ctx = ola->ctx;
        if (int rc = check_count(entry, n_ids)) return rc;
        const std::string e(entry);
        if (n_samples < 0) return fail(ctx, JDSP_EINVAL, (e + ": n_samples < 0").c_str());
        if (n_ids > 0 && (!stream_id_host || !sample_first_host))
            return fail(ctx, JDSP_EINVAL, (e + ": stream_id or sample_first is NULL").c_str());
        if (int rc = check_ids(entry, stream_id_host, n_ids)) return rc;
        std::vector<int64_t> unit((size_t)n_ids + 1);
        for (long i = 0; i <= n_ids; i++) unit[(size_t)i] = i;
        const int nt = n_tail();
        const RaggedLayout lay = ragged_layout_check(sample_first_host, unit.data(), n_ids, n_samples, nt, nt ? nt : 1);
        if (lay.verdict != RaggedVerdict::kOk)
            return fail(ctx, JDSP_EINVAL, ragged_layout_message(lay.verdict, entry, "stream_id").c_str());
        JDSP_HIP(ctx, hipSetDevice(ctx->device));
        int16_t *d_i16 = nullptr;
        float *d_f32 = nullptr;
        const hipError_t err = ola->stage_out((size_t)n_samples, out_i16_host, out_f32_host, d_i16, d_f32);
        if (err != hipSuccess) return fail(ctx, JDSP_EHIP, (e + ": buffers").c_str(), err);
        HostCall hc(ctx, entry);
        const int64_t *d_id = hc.upload(stream_id_host, (size_t)n_ids * sizeof(int64_t));
        const int64_t *d_sf = hc.upload(sample_first_host, (size_t)n_ids * sizeof(int64_t));
        if (d_i16) hc.zero(d_i16, (size_t)n_samples * sizeof(int16_t));
        if (d_f32) hc.zero(d_f32, (size_t)n_samples * sizeof(float));
        if (hc.ok()) hc.result(flush_dev(entry, d_id, d_sf, n_ids, d_i16, d_f32));
        ola->download_out(hc, (size_t)n_samples, out_i16_host, out_f32_host);
        return hc.finish();
    }
};

// ---- the ragged call layer ------------------------------------------------------------------------------------------
// A ragged call is a batch of utterances (live == NULL) or the chunks of live streams: n spans at sample_first[i] with
// the frames frame_first[i] .. frame_first[i + 1] - 1, for the live streams stream_id[i] as well.  The two handles
// differ in their inputs alone, so what they check of those travels as text: the reason a rule of the handle's own is
// broken, NULL where it is kept.  The layer reports it as `<entry>: <reason>` at the rule's place in the order of checks.
struct OwnRules {
    const char *pitch = nullptr;          // mask_pitch / row_pitch out of range
    const char *align = nullptr;          // a misaligned input (device entries)
    const char *null = nullptr;           // a NULL input, asked only of a call with frames
};

enum class RaggedCall { kRejected, kNothing, kLaunch };

// JDSP_EINVAL with the message `<entry>: <why>`
inline int ragged_einval(jdsp_ctx *ctx, const char *entry, const char *why)
{
    return fail(ctx, JDSP_EINVAL, (std::string(entry) + ": " + why).c_str());
}
inline RaggedCall ragged_reject(jdsp_ctx *ctx, const char *entry, const char *why)
{
    ragged_einval(ctx, entry, why);
    return RaggedCall::kRejected;
}

// The checks of a device entry in front of its launch.  kRejected: JDSP_EINVAL, the message is set.  kNothing: no spans,
// no frames or no output to write -- the call succeeds, launches nothing and advances no stream.  kLaunch: go on.
inline RaggedCall ragged_call_check(jdsp_ctx *ctx, const OlaStreams *live, const char *entry, const OwnRules &own,
                                    const int64_t *stream_id_dev, const int64_t *sample_first_dev,
                                    const int64_t *frame_first_dev, long n, long n_frames_total, const void *out_i16_dev,
                                    const void *out_f32_dev)
{
    if (live) {
        if (live->check_count(entry, n)) return RaggedCall::kRejected;
        if (n_frames_total < 0) return ragged_reject(ctx, entry, "n_frames_total < 0");
    } else if (n < 0 || n_frames_total < 0) {
        return ragged_reject(ctx, entry, "n_utts or n_frames_total < 0");
    }
    if (own.pitch) return ragged_reject(ctx, entry, own.pitch);
    if (own.align) return ragged_reject(ctx, entry, own.align);
    if (!aligned(out_i16_dev, 4) || !aligned(out_f32_dev, 8) || !aligned(stream_id_dev, 8) ||
        !aligned(sample_first_dev, 8) || !aligned(frame_first_dev, 8))
        return ragged_reject(ctx, entry,
                             live ? "out_i16 must be 4-byte, out_f32, the stream ids and the offset arrays 8-byte aligned"
                                  : "out_i16 must be 4-byte, out_f32 and the offset arrays 8-byte aligned");
    if (n == 0 || n_frames_total == 0) return RaggedCall::kNothing;
    if (own.null) return ragged_reject(ctx, entry, own.null);
    if ((live && !stream_id_dev) || !sample_first_dev || !frame_first_dev)
        return ragged_reject(ctx, entry, live ? "stream_id, sample_first or frame_first is NULL"
                                              : "sample_first or frame_first is NULL");
    if (!out_i16_dev && !out_f32_dev) return RaggedCall::kNothing;     // no stream to advance
    return RaggedCall::kLaunch;
}

// A host entry, synchronous: checks the arrays (the ids; the spans of span_n + hop (F - 1) samples even, ascending,
// disjoint and inside n_samples), brings them and the inputs to the device, runs the *_dev twin and copies back outputs
// of n_samples that are zero outside what the call wrote.
//   inputs(hc, n_total, end) -> hipError_t: grows the handle's device copies of its inputs for n_total frames whose
//       spans end at sample `end`, and enqueues their upload on hc;
//   dev(d_stream_id, d_sample_first, d_frame_first, n_total, d_i16, d_f32) -> the *_dev twin's return code.
// A call with nothing to launch reaches the twin as well, as a call of no frames: what a handle does about one (its
// count of recomputed frames) it does there.
template <class Inputs, class Dev>
int ragged_host_call(OlaStream &ola, const OlaStreams *live, const char *entry, const OwnRules &own,
                     const int64_t *stream_id, const int64_t *sample_first, const int64_t *frame_first, long n,
                     long n_samples, long span_n, int16_t *out_i16, float *out_f32, Inputs inputs, Dev dev)
{
    jdsp_ctx *ctx = ola.ctx;
    const auto reject = [&](const char *why) { return ragged_einval(ctx, entry, why); };
    if (live) {
        if (int rc = live->check_count(entry, n)) return rc;
        if (n_samples < 0) return reject("n_samples < 0");
    } else if (n < 0 || n_samples < 0) {
        return reject("n_utts or n_samples < 0");
    }
    if (own.pitch) return reject(own.pitch);
    if (n > 0 && ((live && !stream_id) || !sample_first || !frame_first))
        return reject(live ? "stream_id, sample_first or frame_first is NULL" : "sample_first or frame_first is NULL");
    if (live)
        if (int rc = live->check_ids(entry, stream_id, n)) return rc;
    RaggedOffsets offs;
    if (offs.check(ctx, entry, "frame_first", sample_first, frame_first, n, n_samples, span_n, ola.hop)) return JDSP_EINVAL;
    const long n_total = offs.lay.n_total;
    if (n_total == 0 || (!out_i16 && !out_f32)) {              // nothing to launch: the outputs are zero everywhere
        if (out_i16 && n_samples) memset(out_i16, 0, (size_t)n_samples * sizeof(int16_t));
        if (out_f32 && n_samples) memset(out_f32, 0, (size_t)n_samples * sizeof(float));
        return dev(nullptr, nullptr, nullptr, 0, nullptr, nullptr);
    }
    if (own.null) return reject(own.null);
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int16_t *d_i16 = nullptr;
    float *d_f32 = nullptr;
    hipError_t e = ola.stage_out((size_t)n_samples, out_i16, out_f32, d_i16, d_f32);
    if (e != hipSuccess) return fail(ctx, JDSP_EHIP, (std::string(entry) + ": buffers").c_str(), e);
    HostCall hc(ctx, entry);
    offs.upload(hc);
    const int64_t *d_id = live ? hc.upload(stream_id, (size_t)n * sizeof(int64_t)) : nullptr;
    e = inputs(hc, n_total, offs.lay.end);
    if (e != hipSuccess) hc.result(fail(ctx, JDSP_EHIP, (std::string(entry) + ": buffers").c_str(), e));
    if (d_i16) hc.zero(d_i16, (size_t)n_samples * sizeof(int16_t));            // outside the written ranges
    if (d_f32) hc.zero(d_f32, (size_t)n_samples * sizeof(float));
    if (hc.ok()) hc.result(dev(d_id, offs.d_sample, offs.d_unit, n_total, d_i16, d_f32));
    ola.download_out(hc, (size_t)n_samples, out_i16, out_f32);
    return hc.finish();
}

}  // namespace jdsp
