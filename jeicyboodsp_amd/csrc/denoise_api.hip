// denoise_api.hip -- C ABI of the spectral-subtraction / Wiener stream object.
#include "jdsp_internal.h"

using jdsp::fail;

static jdsp::DenoiseGeom geom(const jdsp_denoise *h) { return {h->n_fft, h->win512h.get()}; }

// the launchers' view of the workspace's chunked noise average
static jdsp::NoiseAccum accum(const jdsp_denoise *h)
{
    const jdsp_denoise::Workspace &w = h->ws;
    return {w.chunk_alpha.get(), w.chunk_beta.get(), w.a_start.get(), w.lat_alpha.get(), w.lat_chunk.get()};
}

extern "C" {

int jdsp_denoise_create(jdsp_ctx *ctx, int mode, jdsp_denoise **out) { return jdsp_denoise_create_cfg(ctx, mode, 1024, 512, out); }

int jdsp_denoise_block_len(const jdsp_denoise *h) { return h ? h->block : 0; }

int jdsp_denoise_create_cfg(jdsp_ctx *ctx, int mode, int n_fft, int hop, jdsp_denoise **out)
{
    if (!ctx || !out) return JDSP_EINVAL;
    *out = nullptr;
    if (mode != JDSP_SPECSUB && mode != JDSP_WIENER) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_create: mode");
    if (!((n_fft == 1024 && hop == 512) || (n_fft == 512 && hop == 256)))
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_create_cfg: (n_fft, hop) must be (1024, 512) or (512, 256)");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp::ensure_stft1024_table(ctx);
    if (rc) return rc;
    jdsp_denoise *h = new (std::nothrow) jdsp_denoise();
    if (!h) return fail(ctx, JDSP_ENOMEM, "jdsp_denoise_create");
    h->ctx = ctx;
    h->mode = mode;
    h->n_fft = n_fft;
    h->block = hop;
    hipError_t e = hipSuccess;
    if (n_fft == 512) {
        // Hamming over 512 points exactly as the reference writes it (SS:226, PI 3.141592): the VAD's FP64 second half
        // (SS:131: the first half multiplies the never-updated, all-zero keep buffer) and the halved FP32 window
        double w_hi[256];
        float w_h[512];
        for (int i = 0; i < 512; i++) {
            const double w = (0.54 - 0.46 * cos(2 * 3.141592 * i / (512 - 1)));
            w_h[i] = (float)(0.5 * w);
            if (i >= 256) w_hi[i - 256] = w;
        }
        e = h->w_hi256.upload(w_hi, 256);
        if (e == hipSuccess) e = h->win512h.upload(w_h, 512);
    }
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = h->st[i].alloc(1);
    if (e == hipSuccess) e = h->plan.alloc(1);
    if (e == hipSuccess) e = h->sh_range.alloc(4);
    if (e == hipSuccess) e = h->sh_a_in.alloc(1024);
    if (e == hipSuccess) e = h->sh_zero_run.alloc(1);
    if (e == hipSuccess) e = hipMemset(h->sh_zero_run.get(), 0, sizeof(int));
    if (e == hipSuccess && jdsp::ensure_vad_window(ctx)) e = hipErrorUnknown;
    h->w_hi = n_fft == 512 ? h->w_hi256.get() : ctx->vad_w_hi.get();
    if (e != hipSuccess) {
        jdsp_denoise_destroy(h);
        return fail(ctx, JDSP_EHIP, "jdsp_denoise_create: alloc", e);
    }
    rc = jdsp_denoise_reset(h);
    if (rc) {
        jdsp_denoise_destroy(h);
        return rc;
    }
    *out = h;
    return JDSP_OK;
}

int jdsp_denoise_destroy(jdsp_denoise *h)
{
    if (!h) return JDSP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return JDSP_OK;
}

int jdsp_denoise_reset(jdsp_denoise *h)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    for (int i = 0; i < 2; i++) JDSP_HIP(ctx, hipMemsetAsync(h->st[i].get(), 0, sizeof(jdsp::DenoiseState), ctx->stream));
    h->calls = 0;
    h->cur = 0;
    h->last_blocks = 0;
    h->redo_valid = 0;
    return JDSP_OK;
}

int jdsp_denoise_set_option(jdsp_denoise *h, const char *name, long value)
{
    if (!h || !name) return JDSP_EINVAL;
    if (!strcmp(name, "vad_trace")) {
        if (value != 0 && value != 1) return fail(h->ctx, JDSP_EINVAL, "jdsp_denoise_set_option: vad_trace must be 0 or 1");
        h->opt_vad_trace = (int)value;
        return JDSP_OK;
    }
    if (!strcmp(name, "blocks_per_wave")) {
        if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
            return fail(h->ctx, JDSP_EINVAL, "jdsp_denoise_set_option: blocks_per_wave must be 0 (auto), 1, 2, 4 or 8");
        h->opt_k = (int)value;
        return JDSP_OK;
    }
    return fail(h->ctx, JDSP_EINVAL, "jdsp_denoise_set_option: unknown option");
}

long jdsp_denoise_blocks_out(const jdsp_denoise *h, long n_blocks)
{
    if (!h || n_blocks < 0) return 0;
    const long first_emit = h->calls >= 2 ? 0 : 2 - h->calls;       // SS:260-263
    return n_blocks > first_emit ? n_blocks - first_emit : 0;
}

static int reserve2(jdsp_denoise *h, long max_blocks);

int jdsp_denoise_reserve(jdsp_denoise *h, long max_blocks)
{
    if (!h || max_blocks < 0) return JDSP_EINVAL;
    return reserve2(h, max_blocks);
}

// max_blocks: blocks the run-length plan covers (a sharded run: the whole stream's)
static int reserve2(jdsp_denoise *h, long max_blocks)
{
    jdsp_ctx *ctx = h->ctx;
    if (max_blocks <= h->ws.run.cap_blocks) return JDSP_OK;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    jdsp_denoise::Workspace &w = h->ws;
    w = {};                                           // freed before anything is allocated
    const size_t n = (size_t)max_blocks;
    hipError_t e = w.run.reserve(n);
    if (e == hipSuccess) e = w.dbg_energy.alloc(n);
    if (e == hipSuccess) e = w.dbg_zcr.alloc(n);
    // worst case: every block feeds the noise average; an estimate can latch at most every 10th block.  (No magnitude
    // rows: noise_accum_kernel folds them into per-chunk maps in registers.)
    const size_t n_rows = n / 10 + 2;
    if (e == hipSuccess) e = w.rows.alloc(n_rows * 1024);
    if (e == hipSuccess) e = w.lat_alpha.alloc(n_rows);
    if (e == hipSuccess) e = w.lat_chunk.alloc(n_rows);
    const size_t n_chunks = n < (size_t)jdsp::kNoiseChunks ? (n > 0 ? n : 1) : (size_t)jdsp::kNoiseChunks;   // launch_noise_estimate's grid
    if (e == hipSuccess) e = w.chunk_alpha.alloc(n_chunks);
    if (e == hipSuccess) e = w.chunk_beta.alloc(n_chunks * 1024);
    if (e == hipSuccess) e = w.a_start.alloc(n_chunks * 1024);
    if (e == hipSuccess) e = w.redo.alloc(n + 1);
    if (h->redo_valid == 1) h->redo_valid = 0;
    if (e != hipSuccess) {
        w = {};
        return fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_denoise_reserve", e);
    }
    return JDSP_OK;
}

int jdsp_denoise_process_dev(jdsp_denoise *h, const int16_t *pcm_dev, long n_blocks, int16_t *out_dev,
                             float *precast_dev, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_process: n_blocks < 0");
    const long n_out = jdsp_denoise_blocks_out(h, n_blocks);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (n_blocks == 0) return JDSP_OK;
    if (!pcm_dev || (n_out > 0 && !out_dev)) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_process: NULL buffer");
    if (((uintptr_t)pcm_dev & 15u) || ((uintptr_t)out_dev & 15u))
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_process: buffers must be 16-byte aligned");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp_denoise_reserve(h, n_blocks);      // no-op once sized (call jdsp_denoise_reserve before graph capture)
    if (rc) return rc;
    const jdsp::DenoiseState *st_in = h->st[h->cur].get();
    jdsp::DenoiseState *st_out = h->st[h->cur ^ 1].get();
    hipStream_t s = ctx->stream;
    const jdsp::DenoiseGeom g = geom(h);
    const jdsp_denoise::Workspace &w = h->ws;
    const jdsp::RunPlanWs &r = w.run;
    const float2 *table = ctx->stft1024_table.get();
    if (jdsp::launch_vad(s, h->block, pcm_dev, n_blocks, h->w_hi, 1, r.flags.get(),
                         h->opt_vad_trace ? w.dbg_energy.get() : nullptr, h->opt_vad_trace ? w.dbg_zcr.get() : nullptr) ||
        jdsp::launch_denoise_plan(s, r.flags.get(), n_blocks, st_in, st_out, r.ver_base.get(), r.snap_mask.get(),
                                  r.events.get(), r.ev_n.get(), h->plan.get()) ||
        jdsp::launch_noise_estimate(s, g, pcm_dev, n_blocks, st_in, st_out, r.events.get(), r.ev_n.get(), h->plan.get(),
                                    r.ver_base.get(), r.snap_mask.get(), table, accum(h), w.rows.get()) ||
        jdsp::launch_denoise(s, g, h->mode, h->opt_k, ctx->n_cu, pcm_dev, n_blocks, h->calls, st_in, st_out,
                             r.ver_base.get(), r.snap_mask.get(), w.rows.get(), table, out_dev, precast_dev, w.redo.get()))
        return fail(ctx, JDSP_EHIP, "denoise launch", hipGetLastError());
    h->redo_valid = 1;
    h->cur ^= 1;
    h->calls += n_blocks;
    h->last_blocks = n_blocks;
    h->last_trace_valid = h->opt_vad_trace;
    return JDSP_OK;
}

int jdsp_denoise_process(jdsp_denoise *h, const int16_t *pcm_host, long n_blocks, int16_t *out_host,
                         float *precast_host, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_process: n_blocks < 0");
    const long n_out = jdsp_denoise_blocks_out(h, n_blocks);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (n_blocks == 0) return JDSP_OK;
    if (!pcm_host || (n_out > 0 && !out_host)) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_process: NULL buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t blk = (size_t)h->block;
    const size_t in_b = (size_t)n_blocks * blk * sizeof(int16_t);
    const size_t out_b = (size_t)(n_out > 0 ? n_out : 1) * blk * sizeof(int16_t);
    jdsp::HostCall hc(ctx, "jdsp_denoise_process");
    const int16_t *d_in = hc.upload(pcm_host, in_b);
    int16_t *d_out = hc.alloc<int16_t>(out_b);
    float *d_pre = precast_host ? hc.alloc<float>(out_b * 2) : nullptr;
    if (hc.ok()) hc.result(jdsp_denoise_process_dev(h, d_in, n_blocks, d_out, d_pre, nullptr));
    hc.download(out_host, d_out, (size_t)n_out * blk * 2);
    hc.download(precast_host, d_pre, (size_t)n_out * blk * 4);
    return hc.finish();
}

int jdsp_denoise_apply(jdsp_denoise *h, const int16_t *pcm_host, long n_blocks, const double *noise_host,
                       int16_t *out_host, float *precast_host, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_blocks < 0 || !noise_host) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_apply: bad argument");
    const long n_out = jdsp_denoise_blocks_out(h, n_blocks);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (n_blocks == 0) return JDSP_OK;
    if (!pcm_host || (n_out > 0 && !out_host)) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_apply: NULL buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = jdsp_denoise_reserve(h, n_blocks);
    if (rc) return rc;
    float row[1024];
    for (int i = 0; i < h->n_fft; i++) row[i] = (float)noise_host[i];          // pdEstimatedNoiseSpec[FFT_PROCESSING_SIZE]
    const size_t blk_b = (size_t)h->block * sizeof(int16_t);
    const size_t in_b = (size_t)n_blocks * blk_b, out_b = (size_t)(n_out > 0 ? n_out : 1) * blk_b;
    hipStream_t s = ctx->stream;
    jdsp::DenoiseState *st_in = h->st[h->cur].get(), *st_out = h->st[h->cur ^ 1].get();
    float *rows = h->ws.rows.get();
    int *ver_base = h->ws.run.ver_base.get();
    unsigned long long *snap_mask = h->ws.run.snap_mask.get();
    jdsp::HostCall hc(ctx, "jdsp_denoise_apply");
    const int16_t *d_in = hc.upload(pcm_host, in_b);
    int16_t *d_out = hc.alloc<int16_t>(out_b);
    float *d_pre = precast_host ? hc.alloc<float>(out_b * 2) : nullptr;
    hc.upload_to(rows, row, sizeof(float) * (size_t)h->n_fft);
    hc.zero(ver_base, ((size_t)n_blocks / 64 + 1) * sizeof(int));                      // every block uses row 0
    hc.zero(snap_mask, ((size_t)n_blocks / 64 + 1) * sizeof(unsigned long long));
    hc.copy_dev(st_out, st_in, sizeof(jdsp::DenoiseState));
    if (hc.ok() && jdsp::launch_denoise(s, geom(h), h->mode, h->opt_k, ctx->n_cu, d_in, n_blocks, h->calls, st_in, st_out,
                                        ver_base, snap_mask, rows, ctx->stft1024_table.get(), d_out, d_pre,
                                        h->ws.redo.get()))
        hc.result(fail(ctx, JDSP_EHIP, "denoise launch", hipGetLastError()));
    hc.download(out_host, d_out, (size_t)n_out * blk_b);
    hc.download(precast_host, d_pre, (size_t)n_out * blk_b * 2);
    rc = hc.finish();
    if (!rc) {
        h->cur ^= 1;
        h->calls += n_blocks;
        h->last_blocks = 0;
        h->redo_valid = 1;
    }
    return rc;
}

int jdsp_vad_blocks_ex(jdsp_ctx *ctx, int variant, int block_len, const int16_t *pcm_host, long n_blocks,
                       uint8_t *voice_host, int64_t *energy_sum_host, int32_t *zcr_host)
{
    if (!ctx) return JDSP_EINVAL;
    if ((variant != JDSP_VAD_DENOISE && variant != JDSP_VAD_MVDR) || (block_len != 512 && block_len != 256))
        return fail(ctx, JDSP_EINVAL, "jdsp_vad_blocks_ex: variant 0 | 1, block_len 512 | 256");
    if (n_blocks < 0 || (n_blocks > 0 && !pcm_host)) return fail(ctx, JDSP_EINVAL, "jdsp_vad_blocks: bad argument");
    if (n_blocks == 0) return JDSP_OK;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const double *w = nullptr;
    int rc = jdsp::ensure_vad_window_ex(ctx, variant, block_len, &w);
    if (rc) return rc;
    const size_t n = (size_t)n_blocks, in_bytes = n * (size_t)block_len * sizeof(int16_t);
    jdsp::HostCall hc(ctx, "jdsp_vad_blocks");
    const int16_t *d_in = hc.upload(pcm_host, in_bytes);
    unsigned char *d_v = hc.alloc<unsigned char>(n);
    long long *d_e = hc.alloc<long long>(n * 8);
    int *d_z = hc.alloc<int>(n * 4);
    const int use_zcr = variant == JDSP_VAD_DENOISE;                    // BF:233 tests the energy alone
    if (hc.ok() && jdsp::launch_vad(ctx->stream, block_len, d_in, n_blocks, w, use_zcr, d_v, d_e, d_z))
        hc.result(fail(ctx, JDSP_EHIP, "vad launch", hipGetLastError()));
    hc.download(voice_host, d_v, n);
    hc.download(energy_sum_host, d_e, n * 8);
    hc.download(zcr_host, d_z, n * 4);
    return hc.finish();
}

int jdsp_vad_blocks(jdsp_ctx *ctx, const int16_t *pcm_host, long n_blocks, uint8_t *voice_host,
                    int64_t *energy_sum_host, int32_t *zcr_host)
{
    return jdsp_vad_blocks_ex(ctx, JDSP_VAD_DENOISE, 512, pcm_host, n_blocks, voice_host, energy_sum_host, zcr_host);
}

/* ---- multi-GPU: one rank's share of a stream (include/jdsp.h "sharded denoise") ------------- */
int jdsp_denoise_shard_vad_dev(jdsp_denoise *h, const int16_t *pcm_ext_dev, long ext0, long b0, long b1, long n_total,
                               uint8_t *flags_own_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (!(0 <= ext0 && ext0 <= b0 && b0 <= b1 && b1 <= n_total) || (b0 >= 2 ? ext0 != b0 - 2 : ext0 != 0))
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_shard_vad: need ext0 = max(b0-2, 0) <= b0 <= b1 <= n_total");
    if (b1 > b0 && (!pcm_ext_dev || !flags_own_dev)) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_shard_vad: NULL buffer");
    if ((uintptr_t)pcm_ext_dev & 15u) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_shard_vad: pcm must be 16-byte aligned");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = reserve2(h, n_total);
    if (rc) return rc;
    rc = jdsp_denoise_reset(h);                       // a sharded run is one fresh global stream
    if (rc) return rc;
    h->sh_ext0 = ext0; h->sh_b0 = b0; h->sh_b1 = b1; h->sh_total = n_total; h->sh_pcm = pcm_ext_dev;
    if (jdsp::launch_vad(ctx->stream, h->block, pcm_ext_dev + (b0 - ext0) * h->block, b1 - b0, h->w_hi, 1, flags_own_dev,
                         nullptr, nullptr))
        return fail(ctx, JDSP_EHIP, "vad launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_denoise_shard_summary_dev(jdsp_denoise *h, const uint8_t *flags_all_dev, float *summary_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (!h->sh_pcm && h->sh_b1 > h->sh_b0) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_shard_summary: call shard_vad first");
    if (!flags_all_dev || !summary_dev) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_shard_summary: NULL buffer");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const jdsp::RunPlanWs &r = h->ws.run;
    if (jdsp::launch_run_plan(s, flags_all_dev, h->sh_total, h->sh_zero_run.get(), nullptr, 10, r.ver_base.get(),
                              r.snap_mask.get(), r.events.get(), r.ev_n.get(), h->plan.get()) ||
        jdsp::launch_shard_summary(s, geom(h), h->sh_pcm, h->sh_b1 - h->sh_ext0, h->sh_ext0, h->sh_b0, h->sh_b1,
                                   r.events.get(), r.ev_n.get(), h->plan.get(), r.ver_base.get(), r.snap_mask.get(),
                                   ctx->stft1024_table.get(), h->sh_range.get(), accum(h), h->ws.rows.get(), summary_dev))
        return fail(ctx, JDSP_EHIP, "shard summary launch", hipGetLastError());
    return JDSP_OK;
}

int jdsp_denoise_shard_rows_dev(jdsp_denoise *h, const float *summaries_all_dev, int world, int rank, float *last_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (!summaries_all_dev || !last_dev || world < 1 || rank < 0 || rank >= world)
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_shard_rows: bad argument");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    if (jdsp::launch_shard_rows(ctx->stream, geom(h), summaries_all_dev, rank, h->sh_b0, h->sh_b1, h->plan.get(),
                                h->sh_range.get(), accum(h), h->sh_a_in.get(), h->ws.rows.get(), last_dev))
        return fail(ctx, JDSP_EHIP, "shard rows launch", hipGetLastError());
    return JDSP_OK;
}

long jdsp_denoise_shard_blocks_out(const jdsp_denoise *h)
{
    if (!h) return 0;
    const long lo = h->sh_b0 > 2 ? h->sh_b0 : 2;                      // SS:260-263: global blocks 0 and 1 emit nothing
    return h->sh_b1 > lo ? h->sh_b1 - lo : 0;
}

int jdsp_denoise_shard_finish_dev(jdsp_denoise *h, const float *last_all_dev, int world, int rank, int16_t *out_dev,
                                  float *precast_dev, long *n_out_blocks)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    const long n_out = jdsp_denoise_shard_blocks_out(h);
    if (n_out_blocks) *n_out_blocks = n_out;
    if (!last_all_dev || world < 1 || rank < 0 || rank >= world || (n_out > 0 && !out_dev))
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_shard_finish: bad argument");
    if ((uintptr_t)out_dev & 15u) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_shard_finish: out must be 16-byte aligned");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (jdsp::launch_shard_row0(s, geom(h), last_all_dev, rank, h->ws.rows.get()))
        return fail(ctx, JDSP_EHIP, "row0 launch", hipGetLastError());
    if (n_out > 0) {
        jdsp::DenoiseShard sh;
        sh.ver_block_off = h->sh_ext0;
        sh.ver_row_off = h->sh_range.get() + 2;
        const long lo = h->sh_b0 > 2 ? h->sh_b0 : 2;
        sh.emit_from = lo - h->sh_ext0;
        sh.emit_to = h->sh_b1 - h->sh_ext0;
        // fresh state: the two halo blocks in front of the shard rebuild the overlap tail
        if (jdsp::launch_denoise(s, geom(h), h->mode, h->opt_k, ctx->n_cu, h->sh_pcm, h->sh_b1 - h->sh_ext0, h->sh_ext0,
                                 h->st[h->cur].get(), h->st[h->cur ^ 1].get(), h->ws.run.ver_base.get(),
                                 h->ws.run.snap_mask.get(), h->ws.rows.get(), ctx->stft1024_table.get(), out_dev,
                                 precast_dev, h->ws.redo.get(), &sh))
            return fail(ctx, JDSP_EHIP, "denoise launch", hipGetLastError());
        h->redo_valid = 1;
    }
    return JDSP_OK;
}

/* ---- a batch of ragged utterances, each a fresh stream (include/jdsp.h "batched denoise") --- */
static int batch_supported(jdsp_denoise *h, const char *what)
{
    if (h->n_fft == 1024) return JDSP_OK;
    return fail(h->ctx, JDSP_EINVAL, (std::string(what) + ": (1024, 512) handles only; a (512, 256) handle pairs two frames "
                                      "in one transform, which is not built across utterance boundaries").c_str());
}

int jdsp_denoise_batch_reserve(jdsp_denoise *h, long max_blocks_total, long max_utts)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (max_blocks_total < 0 || max_utts < 0 || max_blocks_total > 0x7ffffff0L)
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_batch_reserve: max_blocks_total must be 0 .. 2^31 - 16, max_utts >= 0");
    int rc = batch_supported(h, "jdsp_denoise_batch_reserve");
    if (rc) return rc;
    jdsp_denoise::BatchWs &w = h->bws;
    if (max_blocks_total <= w.cap_blocks) {                     // the utterances need no memory of their own
        if (max_utts > w.cap_utts) w.cap_utts = max_utts;
        return JDSP_OK;
    }
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    w = {};                                                     // freed before anything is allocated
    if (h->redo_valid == 2) h->redo_valid = 0;
    const size_t n = (size_t)max_blocks_total, n_rows = n / 10 + 1;
    hipError_t e = w.flags.alloc(n + 1);
    if (e == hipSuccess) e = w.row_idx.alloc(n + 1);
    if (e == hipSuccess) e = w.redo.alloc(n + 1);
    if (e == hipSuccess) e = w.rows.alloc(n_rows * 1024);
    if (e == hipSuccess) e = hipMemset(w.rows.get(), 0, 1024 * sizeof(float));       // row 0: nothing latched yet
    if (e != hipSuccess) {
        w = {};
        return fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_denoise_batch_reserve", e);
    }
    w.cap_blocks = max_blocks_total;
    w.cap_utts = max_utts;
    return JDSP_OK;
}

// vad_only: no utterance has a third block (the host entry knows; nothing but the flags can come out)
static int batch_dev(jdsp_denoise *h, const int16_t *pcm_dev, const int64_t *sample_first_dev,
                     const int64_t *block_first_dev, long n_utts, long n_blocks_total, int16_t *out_dev,
                     float *precast_dev, uint8_t *flags_dev, float *noise_last_dev, int vad_only)
{
    jdsp_ctx *ctx = h->ctx;
    if (n_utts < 0 || n_blocks_total < 0) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_batch: n_utts or n_blocks_total < 0");
    int rc = batch_supported(h, "jdsp_denoise_batch");
    if (rc) return rc;
    if (!jdsp::aligned(pcm_dev, 16) || !jdsp::aligned(out_dev, 16) || !jdsp::aligned(precast_dev, 8) ||
        !jdsp::aligned(noise_last_dev, 4) || !jdsp::aligned(sample_first_dev, 8) || !jdsp::aligned(block_first_dev, 8))
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_batch: pcm and out must be 16-byte, precast and the offset arrays "
                                      "8-byte, noise_last 4-byte aligned");
    h->redo_valid = 0;
    if (n_utts == 0) return JDSP_OK;
    if (n_blocks_total == 0) {                                 // only empty utterances: no kernel, their estimates are zero
        if (noise_last_dev)
            JDSP_HIP(ctx, hipMemsetAsync(noise_last_dev, 0, (size_t)n_utts * 1024 * sizeof(float), ctx->stream));
        return JDSP_OK;
    }
    if (!out_dev && !precast_dev && !flags_dev && !noise_last_dev) return JDSP_OK;     // nothing to write
    if (!pcm_dev || !sample_first_dev || !block_first_dev)
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_batch: pcm, sample_first or block_first is NULL");
    const jdsp_denoise::BatchWs &w = h->bws;
    if (n_blocks_total > w.cap_blocks || n_utts > w.cap_utts)
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_batch_dev: the batch exceeds what jdsp_denoise_batch_reserve sized "
                                      "(the device entry does not allocate)");
    hipStream_t s = ctx->stream;
    if (jdsp::launch_denoise_batch(s, h->mode, h->opt_k, ctx->n_cu, pcm_dev,
                                   reinterpret_cast<const long long *>(sample_first_dev),
                                   reinterpret_cast<const long long *>(block_first_dev), n_utts, n_blocks_total, h->w_hi,
                                   ctx->stft1024_table.get(), flags_dev ? flags_dev : w.flags.get(), w.row_idx.get(),
                                   w.rows.get(), w.redo.get(), out_dev, precast_dev, noise_last_dev,
                                   vad_only || (!out_dev && !precast_dev && !noise_last_dev)))
        return fail(ctx, JDSP_EHIP, "jdsp_denoise_batch: launch", hipGetLastError());
    if (!vad_only && (out_dev || precast_dev)) h->redo_valid = 2;
    return JDSP_OK;
}

int jdsp_denoise_batch_dev(jdsp_denoise *h, const int16_t *pcm_dev, const int64_t *sample_first_dev,
                           const int64_t *block_first_dev, long n_utts, long n_blocks_total, int16_t *out_dev,
                           float *precast_dev, uint8_t *flags_dev, float *noise_last_dev)
{
    if (!h) return JDSP_EINVAL;
    JDSP_HIP(h->ctx, hipSetDevice(h->ctx->device));
    return batch_dev(h, pcm_dev, sample_first_dev, block_first_dev, n_utts, n_blocks_total, out_dev, precast_dev, flags_dev,
                     noise_last_dev, 0);
}

int jdsp_denoise_batch(jdsp_denoise *h, const int16_t *pcm_host, long n_samples, const int64_t *sample_first_host,
                       const int64_t *block_first_host, long n_utts, int16_t *out_host, float *precast_host,
                       uint8_t *flags_host, float *noise_last_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n_utts < 0 || n_samples < 0) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_batch: n_utts or n_samples < 0");
    int rc = batch_supported(h, "jdsp_denoise_batch");
    if (rc) return rc;
    if (n_utts > 0 && (!sample_first_host || !block_first_host))
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_batch: sample_first or block_first is NULL");
    jdsp::RaggedOffsets offs;                                  // a span of b blocks is b hops: n = hop
    if (offs.check(ctx, "jdsp_denoise_batch", "block_first", sample_first_host, block_first_host, n_utts, n_samples,
                   h->block, h->block))
        return JDSP_EINVAL;
    const long n_total = offs.lay.n_total, end = offs.lay.end;
    // what no launch writes is zero: everything outside the spans, the spans' first and last blocks, the estimate of
    // an utterance too short to latch
    if (out_host && n_samples) memset(out_host, 0, (size_t)n_samples * sizeof(int16_t));
    if (precast_host && n_samples) memset(precast_host, 0, (size_t)n_samples * sizeof(float));
    if (noise_last_host && n_utts) memset(noise_last_host, 0, (size_t)n_utts * 1024 * sizeof(float));
    h->redo_valid = 0;
    const bool vad_only = offs.lay.longest <= 2;
    if (n_total == 0 || (vad_only ? !flags_host : (!out_host && !precast_host && !flags_host && !noise_last_host)))
        return JDSP_OK;                                        // nothing to launch
    if (!pcm_host) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_batch: pcm is NULL");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    rc = jdsp_denoise_batch_reserve(h, n_total, n_utts);
    if (rc) return rc;
    jdsp::HostCall hc(ctx, "jdsp_denoise_batch");
    offs.upload(hc);
    const int16_t *d_pcm = hc.upload(pcm_host, (size_t)end * sizeof(int16_t));         // nothing past the last span is read
    const bool run = !vad_only;
    int16_t *d_out = run && out_host ? hc.alloc<int16_t>((size_t)end * sizeof(int16_t)) : nullptr;
    float *d_pre = run && precast_host ? hc.alloc<float>((size_t)end * sizeof(float)) : nullptr;
    uint8_t *d_flags = flags_host ? hc.alloc<uint8_t>((size_t)n_total) : nullptr;
    float *d_noise = run && noise_last_host ? hc.alloc<float>((size_t)n_utts * 1024 * sizeof(float)) : nullptr;
    if (d_out) hc.zero(d_out, (size_t)end * sizeof(int16_t));
    if (d_pre) hc.zero(d_pre, (size_t)end * sizeof(float));
    if (hc.ok())
        hc.result(batch_dev(h, d_pcm, offs.d_sample, offs.d_unit, n_utts, n_total, d_out, d_pre, d_flags, d_noise, vad_only));
    hc.download(out_host, d_out, d_out ? (size_t)end * sizeof(int16_t) : 0);
    hc.download(precast_host, d_pre, d_pre ? (size_t)end * sizeof(float) : 0);
    hc.download(flags_host, d_flags, (size_t)n_total);
    hc.download(noise_last_host, d_noise, d_noise ? (size_t)n_utts * 1024 * sizeof(float) : 0);
    return hc.finish();
}

/* ---- live streams: chunks that continue carried streams (include/jdsp.h "live denoise streams") --- */
static int live_open(jdsp_denoise *h, const char *what)
{
    if (h->lws.n_streams) return JDSP_OK;
    return fail(h->ctx, JDSP_EINVAL, (std::string(what) + ": no live streams (call jdsp_denoise_streams_reserve first)").c_str());
}

// every stream fresh: zeros everywhere (both parities 0)
static hipError_t live_zero(jdsp_denoise *h)
{
    jdsp_denoise::LiveWs &w = h->lws;
    hipError_t e = hipMemsetAsync(w.state.get(), 0, w.state.count(), h->ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(w.rows.get(), 0, (size_t)w.n_streams * 2 * 1024 * sizeof(float), h->ctx->stream);
    return e;
}

int jdsp_denoise_streams_reserve(jdsp_denoise *h, long n_streams, long max_blocks_total)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = batch_supported(h, "jdsp_denoise_streams_reserve");
    if (rc) return rc;
    if (n_streams < 1 || n_streams > 0x3fffffffL || max_blocks_total < 0 || max_blocks_total > 0x3ffffff0L)
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_streams_reserve: n_streams must be 1 .. 2^30 - 1, max_blocks_total 0 .. 2^30 - 16");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));          // nothing enqueued still uses the old buffers
    jdsp_denoise::LiveWs &w = h->lws;
    w = {};
    if (h->redo_valid == 3) h->redo_valid = 0;
    const size_t n = (size_t)n_streams, nb = (size_t)max_blocks_total;
    // the state's parts in one allocation, the widest alignment first
    const size_t b_seen = n * sizeof(long long), b_tail = 2 * n * 512 * sizeof(float),
                 b_avg = n * jdsp::kLiveAvgFloats * sizeof(float), b_prev = 2 * n * 1024 * sizeof(short),
                 b_word = n * sizeof(int);
    hipError_t e = w.state.alloc(b_seen + b_tail + b_avg + b_prev + 5 * b_word);
    if (e == hipSuccess) e = w.rows.alloc((2 * n + n + nb / 11 + 2) * 1024);
    if (e == hipSuccess) e = w.flags.alloc(nb + 1);
    if (e == hipSuccess) e = w.row_idx.alloc(nb + 1);
    if (e == hipSuccess) e = w.redo.alloc(1 + nb + n);
    if (e == hipSuccess) e = w.latched.alloc(n);
    if (e == hipSuccess) {
        char *p = w.state.get();
        w.seen = reinterpret_cast<long long *>(p), p += b_seen;
        float *tail = reinterpret_cast<float *>(p);
        p += b_tail;
        float *avg = reinterpret_cast<float *>(p);
        p += b_avg;
        short *prev = reinterpret_cast<short *>(p);
        p += b_prev;
        int *word = reinterpret_cast<int *>(p);
        w.parity = word, w.est_parity = word + n;
        w.view = {w.parity, w.est_parity, w.seen, word + 2 * n, word + 3 * n, prev, tail, avg, w.rows.get(), w.latched.get(),
                  n_streams};
        w.n_streams = n_streams;
        e = live_zero(h);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) {
        w = {};
        return fail(ctx, e == hipErrorOutOfMemory ? JDSP_ENOMEM : JDSP_EHIP, "jdsp_denoise_streams_reserve", e);
    }
    w.cap_blocks = max_blocks_total;
    return JDSP_OK;
}

int jdsp_denoise_streams_reset_dev(jdsp_denoise *h, const int64_t *stream_id_dev, long n_ids)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = batch_supported(h, "jdsp_denoise_streams_reset_dev");
    if (!rc) rc = live_open(h, "jdsp_denoise_streams_reset_dev");
    if (rc) return rc;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    jdsp_denoise::LiveWs &w = h->lws;
    if (!stream_id_dev) {
        JDSP_HIP(ctx, live_zero(h));
        return JDSP_OK;
    }
    if (n_ids < 0 || n_ids > w.n_streams)
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_streams_reset_dev: n_ids must be 0 .. n_streams (ids are distinct within a call)");
    if (!jdsp::aligned(stream_id_dev, 8)) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_streams_reset_dev: stream_id must be 8-byte aligned");
    if (jdsp::launch_denoise_live_reset(ctx->stream, reinterpret_cast<const long long *>(stream_id_dev), n_ids, w.view,
                                        w.parity, w.est_parity, w.seen))
        return fail(ctx, JDSP_EHIP, "jdsp_denoise_streams_reset_dev: launch", hipGetLastError());
    return JDSP_OK;
}

// the scalar checks both entries make before anything else
static int live_counts(jdsp_denoise *h, const char *what, long n_chunks, long n_blocks_total)
{
    jdsp_ctx *ctx = h->ctx;
    int rc = batch_supported(h, what);
    if (!rc) rc = live_open(h, what);
    if (rc) return rc;
    const std::string e(what);
    if (n_chunks < 0 || n_blocks_total < 0) return fail(ctx, JDSP_EINVAL, (e + ": n_chunks or the number of blocks < 0").c_str());
    if (n_chunks > h->lws.n_streams)
        return fail(ctx, JDSP_EINVAL, (e + ": more chunks than live streams (ids are distinct within a call)").c_str());
    if (n_blocks_total > h->lws.cap_blocks)
        return fail(ctx, JDSP_EINVAL, (e + ": more blocks than jdsp_denoise_streams_reserve sized the workspace for").c_str());
    return JDSP_OK;
}

int jdsp_denoise_streams_dev(jdsp_denoise *h, const int16_t *pcm_dev, const int64_t *stream_id_dev,
                             const int64_t *sample_first_dev, const int64_t *block_first_dev, long n_chunks,
                             long n_blocks_total, int16_t *out_dev, float *precast_dev, uint8_t *flags_dev,
                             int64_t *n_emitted_dev)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    int rc = live_counts(h, "jdsp_denoise_streams_dev", n_chunks, n_blocks_total);
    if (rc) return rc;
    if (!jdsp::aligned(pcm_dev, 16) || !jdsp::aligned(out_dev, 16) || !jdsp::aligned(precast_dev, 8) ||
        !jdsp::aligned(stream_id_dev, 8) || !jdsp::aligned(sample_first_dev, 8) || !jdsp::aligned(block_first_dev, 8) ||
        !jdsp::aligned(n_emitted_dev, 8))
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_streams_dev: pcm and out must be 16-byte, precast, n_emitted, the "
                                      "stream ids and the offset arrays 8-byte aligned");
    if (n_chunks == 0 || n_blocks_total == 0) return JDSP_OK;   // nothing launched, nothing changed
    if (!pcm_dev || !stream_id_dev || !sample_first_dev || !block_first_dev)
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_streams_dev: pcm, stream_id, sample_first or block_first is NULL");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const jdsp_denoise::LiveWs &w = h->lws;
    if (jdsp::launch_denoise_live(ctx->stream, h->mode, h->opt_k, ctx->n_cu, pcm_dev,
                                  reinterpret_cast<const long long *>(stream_id_dev),
                                  reinterpret_cast<const long long *>(sample_first_dev),
                                  reinterpret_cast<const long long *>(block_first_dev), n_chunks, n_blocks_total, h->w_hi,
                                  ctx->stft1024_table.get(), flags_dev ? flags_dev : w.flags.get(), w.row_idx.get(),
                                  w.redo.get(), w.view, w.parity, w.est_parity, w.seen, out_dev, precast_dev,
                                  reinterpret_cast<long long *>(n_emitted_dev)))
        return fail(ctx, JDSP_EHIP, "jdsp_denoise_streams_dev: launch", hipGetLastError());
    h->redo_valid = 3;
    return JDSP_OK;
}

int jdsp_denoise_streams(jdsp_denoise *h, const int16_t *pcm_host, long n_samples, const int64_t *stream_id_host,
                         const int64_t *sample_first_host, const int64_t *block_first_host, long n_chunks,
                         int16_t *out_host, float *precast_host, uint8_t *flags_host, int64_t *n_emitted_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    const char *me = "jdsp_denoise_streams";
    int rc = live_counts(h, me, n_chunks, 0);
    if (rc) return rc;
    if (n_samples < 0) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_streams: n_samples < 0");
    if (n_chunks > 0 && (!stream_id_host || !sample_first_host || !block_first_host))
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_streams: stream_id, sample_first or block_first is NULL");
    const jdsp::StreamIdVerdict v = jdsp::stream_ids_check(stream_id_host, n_chunks, h->lws.n_streams);
    if (v != jdsp::StreamIdVerdict::kOk) return fail(ctx, JDSP_EINVAL, jdsp::stream_ids_message(v, me).c_str());
    jdsp::RaggedOffsets offs;
    if (offs.check(ctx, me, "block_first", sample_first_host, block_first_host, n_chunks, n_samples, h->block, h->block))
        return JDSP_EINVAL;
    const long n_total = offs.lay.n_total, end = offs.lay.end;
    rc = live_counts(h, me, n_chunks, n_total);
    if (rc) return rc;
    // what no launch writes is zero
    if (out_host && n_samples) memset(out_host, 0, (size_t)n_samples * sizeof(int16_t));
    if (precast_host && n_samples) memset(precast_host, 0, (size_t)n_samples * sizeof(float));
    if (n_emitted_host && n_chunks) memset(n_emitted_host, 0, (size_t)n_chunks * sizeof(int64_t));
    if (n_total == 0) return JDSP_OK;                          // nothing to launch
    if (!pcm_host) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_streams: pcm is NULL");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    jdsp::HostCall hc(ctx, me);
    offs.upload(hc);
    const int64_t *d_id = hc.upload(stream_id_host, (size_t)n_chunks * sizeof(int64_t));
    const int16_t *d_pcm = hc.upload(pcm_host, (size_t)end * sizeof(int16_t));         // nothing past the last span is read
    int16_t *d_out = out_host ? hc.alloc<int16_t>((size_t)end * sizeof(int16_t)) : nullptr;
    float *d_pre = precast_host ? hc.alloc<float>((size_t)end * sizeof(float)) : nullptr;
    uint8_t *d_flags = flags_host ? hc.alloc<uint8_t>((size_t)n_total) : nullptr;
    int64_t *d_emit = n_emitted_host ? hc.alloc<int64_t>((size_t)n_chunks * sizeof(int64_t)) : nullptr;
    if (d_out) hc.zero(d_out, (size_t)end * sizeof(int16_t));
    if (d_pre) hc.zero(d_pre, (size_t)end * sizeof(float));
    if (hc.ok())
        hc.result(jdsp_denoise_streams_dev(h, d_pcm, d_id, offs.d_sample, offs.d_unit, n_chunks, n_total, d_out, d_pre,
                                           d_flags, d_emit));
    hc.download(out_host, d_out, d_out ? (size_t)end * sizeof(int16_t) : 0);
    hc.download(precast_host, d_pre, d_pre ? (size_t)end * sizeof(float) : 0);
    hc.download(flags_host, d_flags, (size_t)n_total);
    hc.download(n_emitted_host, d_emit, (size_t)n_chunks * sizeof(int64_t));
    return hc.finish();
}

int jdsp_denoise_streams_state(jdsp_denoise *h, const int64_t *stream_id_host, long n_ids, float *noise_host,
                               int64_t *blocks_seen_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    const char *me = "jdsp_denoise_streams_state";
    int rc = batch_supported(h, me);
    if (!rc) rc = live_open(h, me);
    if (rc) return rc;
    const jdsp_denoise::LiveWs &w = h->lws;
    if (n_ids < 0 || (n_ids > 0 && !stream_id_host)) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_streams_state: bad argument");
    for (long i = 0; i < n_ids; i++)
        if (stream_id_host[i] < 0 || stream_id_host[i] >= w.n_streams)
            return fail(ctx, JDSP_EINVAL, "jdsp_denoise_streams_state: a stream id lies outside [0, n_streams)");
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (long i = 0; i < n_ids; i++) {
        const int64_t id = stream_id_host[i];
        int ep = 0;
        JDSP_HIP(ctx, hipMemcpyAsync(&ep, w.est_parity + id, sizeof(int), hipMemcpyDeviceToHost, s));
        if (blocks_seen_host)
            JDSP_HIP(ctx, hipMemcpyAsync(blocks_seen_host + i, w.seen + id, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        JDSP_HIP(ctx, hipStreamSynchronize(s));
        if (noise_host)
            JDSP_HIP(ctx, hipMemcpyAsync(noise_host + (size_t)i * 1024,
                                         w.rows.get() + ((size_t)(ep & 1) * w.n_streams + id) * 1024, 1024 * sizeof(float),
                                         hipMemcpyDeviceToHost, s));
    }
    JDSP_HIP(ctx, hipStreamSynchronize(s));
    return JDSP_OK;
}

int jdsp_denoise_noise(jdsp_denoise *h, double *noise_host)
{
    if (!h || !noise_host) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    float tmp[1024];
    JDSP_HIP(ctx, hipMemcpyAsync(tmp, h->st[h->cur].get()->noise, sizeof(tmp), hipMemcpyDeviceToHost, ctx->stream));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < h->n_fft; i++) noise_host[i] = tmp[i];
    return JDSP_OK;
}

long jdsp_denoise_frames_recomputed(jdsp_denoise *h)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (!h->redo_valid || (h->mode != JDSP_SPECSUB && h->n_fft == 1024)) return 0;   // 1024-point Wiener lists nothing
    int n = 0;
    JDSP_HIP(ctx, hipSetDevice(ctx->device));
    const int *count = h->redo_valid == 3 ? h->lws.redo.get() : h->redo_valid == 2 ? h->bws.redo.get() : h->ws.redo.get();
    JDSP_HIP(ctx, hipMemcpyAsync(&n, count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return n;
}

int jdsp_denoise_vad_trace(jdsp_denoise *h, long n, uint8_t *voice_host, int64_t *energy_sum_host, int32_t *zcr_host)
{
    if (!h) return JDSP_EINVAL;
    jdsp_ctx *ctx = h->ctx;
    if (n < 0 || n > h->last_blocks) return fail(ctx, JDSP_EINVAL, "jdsp_denoise_vad_trace: n exceeds the last call");
    if ((energy_sum_host || zcr_host) && !h->last_trace_valid)
        return fail(ctx, JDSP_EINVAL, "jdsp_denoise_vad_trace: energies / ZCR are kept only with set_option(\"vad_trace\", 1) before the call");
    if (n == 0) return JDSP_OK;
    if (voice_host) JDSP_HIP(ctx, hipMemcpyAsync(voice_host, h->ws.run.flags.get(), (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (energy_sum_host)
        JDSP_HIP(ctx, hipMemcpyAsync(energy_sum_host, h->ws.dbg_energy.get(), (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (zcr_host) JDSP_HIP(ctx, hipMemcpyAsync(zcr_host, h->ws.dbg_zcr.get(), (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    JDSP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JDSP_OK;
}

}  // extern "C"
