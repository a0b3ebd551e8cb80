// jdsp_internal.h -- shared declarations of libjdsp (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/jdsp.h"
#include "ragged_layout.h"

namespace jdsp {

// Owner of one device allocation of count() elements: move-only, freed by the destructor.  Every step hands back HIP's
// own error -- the JDSP_* code and the message stay the caller's -- and after a failed one the buffer is empty
// (get() == nullptr, count() == 0).  It sets no device and synchronises nothing: both are the caller's job.
template <class T> class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    size_t count() const { return n_; }
    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr, n_ = 0;
    }
    // frees what it holds first: the peak footprint is one allocation, not two
    hipError_t alloc(size_t count)
    {
        reset();
        void *p = nullptr;      // hipMalloc leaves it alone when it fails
        const hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e == hipSuccess) p_ = (T *)p, n_ = count;
        return e;
    }
    // all or nothing: a buffer whose copy failed is not kept
    hipError_t upload(const T *host, size_t count)
    {
        hipError_t e = alloc(count);
        if (e == hipSuccess && (e = hipMemcpy(p_, host, count * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess) reset();
        return e;
    }
    // contents are not carried over
    hipError_t grow(size_t count) { return count <= n_ ? hipSuccess : alloc(count); }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace jdsp

struct jdsp_ctx {
    int device = 0;
    int n_cu = 0;
    size_t hbm_bytes = 0;
    char name[64] = {0};
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;      // the stream work is enqueued on
    hipEvent_t switch_ev = nullptr;    // orders the old stream's work before the new stream's (jdsp_set_stream)
    std::string error;
    int opt_stft_fpw = 0;              // 0 = auto
    int opt_stft_window = 0;           // 0 Hamming (the reference), 1 Hann -- jdsp_stft_* only
    int opt_stft_read_pass = -1;       // read-only pass that pulls the PCM into the Infinity Cache before the transform:
                                       // 0 never, 1 always, -1 auto (large hop-512 batches); stft_kernels.hip
    int opt_stft_touch_wg = 0;         // tuning: workgroups per CU of that pass (0 = default)
    int opt_stft_f64_kernel = 0;       // 0: stft1024_f64_v2_kernel, 1: round 2's stft1024_f64_kernel (A/B)
    int opt_stft_f64_fpw = 0;          // frames one wave of the FP64 analysis walks (0 = one round of resident waves)
    // device tables, created on first use (jdsp::ensure_table)
    jdsp::DevBuf<float2> stft1024_table;
    jdsp::DevBuf<float2> stft1024_table_hann, win512_hann;
    jdsp::DevBuf<float2> stft1024_table_rect;   // rectangular window: the partitioned convolver's forward frames
    jdsp::DevBuf<float2> win512;             // halved Hamming-512 pairs
    jdsp::DevBuf<double2> c2c_tw[16];        // by log2(n_fft)
    jdsp::DevBuf<double> stft_f64_table;     // FP64 STFT: window + split twiddles (fft_c2c_kernels.hip)
    jdsp::DevBuf<float2> conv_tw4096, conv_tw8192;   // made together; conv_tw8192 goes up last, so it stands for both
    jdsp::DevBuf<double> vad_w_hi;           // second half of the FP64 Hamming window
    jdsp::DevBuf<double> vad_w_ex[2][2];     // jdsp_vad_blocks_ex: [variant][block 512 | 256]
    jdsp::DevBuf<double> lpc_win[2];         // jdsp_lpc: FP64 Hamming(2 block_len), block 256 | 512
    // pinned-host pipeline of jdsp_stft_i16: copy-in / compute / copy-out on three streams
    hipStream_t pipe_in = nullptr, pipe_out = nullptr;
    hipEvent_t pipe_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    jdsp::DevBuf<char> pipe_buf[4];    // in[2], out[2]
};

namespace jdsp {

// All of the reference's static state for one SS/Wiener stream (device memory).
struct DenoiseState {
    int run_len;          // main(): iNumOfIteration                      SS:72,99,108
    int pad[3];
    float avg[1024];      // EstimateNoiseSpectrum: rgsdAveragedNS         SS:161
    float noise[1024];    // main(): rgdEstimatedNS                        SS:70
    short prev[512];      // the keep buffers = previous input block       SS:164,208
    float tail[512];      // rgsdOveraped[0..511] after the shift          SS:209,255
};
struct DenoisePlan { int n_events, n_snap, pad0, pad1; };

// Workspace of the chunked noise average (denoise_kernels.hip, noise_accum_kernel): one affine map per chunk of events
constexpr int kNoiseChunks = 4096;         // most chunks a call is cut into = noise_accum's largest grid (4 waves per SIMD)
struct NoiseAccum {
    float *chunk_alpha;    // [kNoiseChunks]
    float *chunk_beta;     // [kNoiseChunks][1024]
    float *a_start;        // [kNoiseChunks][1024]   the average entering each chunk
    float *lat_alpha;      // [rows]                 per latched row: the chunk's alpha up to and including the latch
    int *lat_chunk;        // [rows]                 ... and its chunk
};

// How the run kernels (denoise_run_kernel, denoise512_run_kernel) and the FP64 pass map local block indices onto the
// (possibly global) plan and what they emit.
struct DenoiseShard {
    long ver_block_off;        // global index of local block 0 (0 when not sharded)
    const int *ver_row_off;    // device int: latches before the shard, subtracted from the version (or NULL)
    long emit_from, emit_to;   // local block range written to `out`
};

// The frame size a denoise launcher works at: 1024 (blocks of 512), or 512 (blocks of 256) with the handle's halved
// Hamming(512); win512 is not read at 1024.
struct DenoiseGeom {
    int n_fft;
    const float *win512;
};

// BeamForming_MVDR_ver1.cpp's state between calls (device memory)
constexpr int kMvdrTableVersions = 8192;     // 2-microphone MVDR: calls with fewer events than this get their weights from a table (16 KB per version)
constexpr int kMvnChunks = 128;            // chunks the n-microphone covariance update cuts a call's events into
constexpr int kMvnBatchEvents = 128;       // ... and the events per chunk of an utterance of a batch (mvdrn_batch_kernels.hip)

struct MvdrState {
    int run_len;          // main(): iNumOfIteration             MVDR:59,99,108
    int pad[3];
    double corr[4];       // rgdSpatialCorr, row-major             MVDR:57
    short prev_l[512];    // previous block of each channel (temp buffers :56, keep buffers :130-131)
    short prev_r[512];
};

// Device-side view of one MFCC configuration (passed by value to the kernel).
struct MfccDev {
    int win_len, hop, n_chan, n_cep, bin_stride;   // bin_stride 2: 512-point bins out of the 1024-point transform
    int n_bins;
    float preemph;
    const float2 *window;        // [512] halved Hamming pairs over win_len, zero beyond
    const float *mel_fb;         // [512] rgdFilterBank as float (zero beyond n_bins)
    const int *mel_k;            // [512] rgdFiBins
    // lane-per-index form of the same filterbank (mfcc_x2_kernel): lane L sums the bins [seg[L].x, +seg[L].y)
    // (at most piece_len, all with rgdFiBins value seg[L].z); seg_wc[q * 64 + L] = {w, 1 - w of bin 2 q; w, 1 - w of bin 2 q + 1},
    // both ZERO past the piece's last bin (eight dwordx4 loads per lane instead of thirty-two dwords, and each
    // (w, 1 - w) an aligned register pair for the packed multiply-add); seg_ok = it fits 64 lanes
    const int4 *seg;
    const float4 *seg_wc;
    int piece_len;               // 8, 12 or 16: no piece is longer (the smallest for which the pieces fit 64 lanes)
    int seg_ok;
    // per channel ch: lanes [x, x + y) hold pieces with index ch (their `hi` parts), lanes [z, z + w) pieces with index
    // ch + 1 (their `lo` parts); chan_ok = no channel needs more than four of either
    const int4 *chan_src;
    int chan_ok;
    const double *dct;           // [max(n_chan, 40)][32]: sqrt(2/C) cos(PI i (k-0.5)/C), zero past n_cep and past n_chan
    const double *lifter_w;      // [32]: 1 + L/2 sin(PI i / L)
    // which frames to compute again (mfcc_leak_one), and what the FP64 pass needs
    const float *chan_w2;        // [64]: sum over the channel's bins of its squared filterbank weights, zero past n_chan
    float leak_k2;               // 2^-46 L_max^2 (2 / C) / 2.5e-6^2
    double preemph_f64;
    const double *win_f64;       // [1024] Hamming over win_len (not halved), zero beyond
    const double2 *tw_f64;       // [n_fft of 1024] exp(-2 pi j m / n_fft)
    const double *fb_f64;        // [512] rgdFilterBank (zero beyond n_bins)
};

int fail(jdsp_ctx *ctx, int code, const char *what, hipError_t e = hipSuccess);
// a: a power of two.  NULL is aligned to anything: whether a pointer may be NULL is a question of its own
inline bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

#define JDSP_HIP(ctx, call)                                             \
    do {                                                                \
        hipError_t e_ = (call);                                         \
        if (e_ != hipSuccess) return ::jdsp::fail((ctx), JDSP_EHIP, #call, e_); \
    } while (0)

// The device side of one host-pointer entry: owns the call's device buffers (freed by the destructor) and enqueues its
// copies on the context's stream.  The first failure sticks -- a failed allocation as JDSP_ENOMEM, a failed copy or
// sync as JDSP_EHIP, the *_dev twin's or launcher's code through result() -- and every later step is a no-op.
class HostCall {
public:
    HostCall(jdsp_ctx *ctx, const char *entry) : ctx_(ctx), entry_(entry) {}
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;

    bool ok() const { return rc_ == JDSP_OK; }
    template <class T> T *alloc(size_t bytes)
    {
        if (!ok()) return nullptr;
        const hipError_t e = n_ < kMaxBufs ? buf_[n_].alloc(bytes ? bytes : 1) : hipErrorOutOfMemory;
        step(JDSP_ENOMEM, "hipMalloc", e);
        return e == hipSuccess ? (T *)buf_[n_++].get() : nullptr;
    }
    template <class T> T *upload(const T *host, size_t bytes)
    {
        T *d = alloc<T>(bytes);
        upload_to(d, host, bytes);
        return d;
    }
    // into memory the handle (or this call) already owns
    void upload_to(void *dev, const void *host, size_t bytes)
    {
        if (ok() && bytes) step(JDSP_EHIP, "H2D", hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx_->stream));
    }
    void zero(void *dev, size_t bytes)
    {
        if (ok()) step(JDSP_EHIP, "memset", hipMemsetAsync(dev, 0, bytes, ctx_->stream));
    }
    void copy_dev(void *dst, const void *src, size_t bytes)
    {
        if (ok()) step(JDSP_EHIP, "D2D", hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx_->stream));
    }
    // host may be NULL (an output the caller did not ask for): skipped
    void download(void *host, const void *dev, size_t bytes)
    {
        if (ok() && host && bytes)
            step(JDSP_EHIP, "D2H", hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx_->stream));
    }
    // what the *_dev twin or launcher returned (it has set the context's message itself)
    void result(int rc)
    {
        if (ok()) rc_ = rc;
    }
    // Synchronises even after a failure: the buffers are freed behind it.
    int finish()
    {
        const hipError_t e = hipStreamSynchronize(ctx_->stream);
        if (ok()) step(JDSP_EHIP, "sync", e);
        return rc_;
    }

private:
    void step(int code, const char *what, hipError_t e)
    {
        if (e != hipSuccess) rc_ = fail(ctx_, code, (std::string(entry_) + ": " + what).c_str(), e);
    }
    static constexpr int kMaxBufs = 8;
    jdsp_ctx *ctx_;
    const char *entry_;
    DevBuf<char> buf_[kMaxBufs];
    int n_ = 0;
    int rc_ = JDSP_OK;
};

// The two offset arrays of a host entry over a batch of ragged utterances (ragged_layout.h; the kernels' walk over
// them: ragged_batch.h).  check() comes behind the entry's own argument checks and reports a bad layout as the
// entry's JDSP_EINVAL; upload() then brings both arrays to the device for the *_dev twin.
struct RaggedOffsets {
    RaggedLayout lay;                                      // check()'s end, n_total and longest
    const int64_t *d_sample = nullptr, *d_unit = nullptr;  // upload()'s: [n_utts] and [n_utts + 1]

    // axis: the unit array's name in the entry's messages, "frame_first" or "block_first"
    int check(jdsp_ctx *ctx, const char *entry, const char *axis, const int64_t *sample_first, const int64_t *unit_first,
              long n_utts, long n_samples, long n, long hop)
    {
        sample_ = sample_first, unit_ = unit_first, n_utts_ = n_utts;
        lay = ragged_layout_check(sample_first, unit_first, n_utts, n_samples, n, hop);
        if (lay.verdict == RaggedVerdict::kOk) return JDSP_OK;
        return fail(ctx, JDSP_EINVAL, ragged_layout_message(lay.verdict, entry, axis).c_str());
    }
    void upload(HostCall &hc)
    {
        d_sample = hc.upload(sample_, (size_t)n_utts_ * sizeof(int64_t));
        d_unit = hc.upload(unit_, (size_t)(n_utts_ + 1) * sizeof(int64_t));
    }

private:
    const int64_t *sample_ = nullptr, *unit_ = nullptr;
    long n_utts_ = 0;
};

// A device table made on first use: JDSP_OK at once when `buf` holds it; otherwise fill(host) writes its `count`
// elements and they go up whole or not at all, so a table that exists is a table that was filled.
template <class T, class Fill> int ensure_table(jdsp_ctx *ctx, DevBuf<T> &buf, size_t count, Fill fill)
{
    if (buf.get()) return JDSP_OK;
    std::vector<T> host(count);
    fill(host.data());
    const hipError_t e = buf.upload(host.data(), count);
    return e == hipSuccess ? JDSP_OK : fail(ctx, JDSP_EHIP, "device table", e);
}

// The per-call arrays of the run-length plan (launch_run_plan, launch_denoise_plan) for calls of up to cap_blocks
// blocks.  reserve() is all or nothing; the early return when the workspace is large enough, the stream synchronise
// before anything is freed and the error code stay with the handle's own reserve function.
struct RunPlanWs {
    DevBuf<unsigned char> flags;            // [n] the VAD's decision per block
    DevBuf<int> events, ev_n;               // [n]
    DevBuf<int> ver_base;                   // [n / 64 + 1]
    DevBuf<unsigned long long> snap_mask;   // [n / 64 + 1]
    long cap_blocks = 0;

    hipError_t reserve(size_t n)
    {
        hipError_t e = flags.alloc(n);
        if (e == hipSuccess) e = events.alloc(n);
        if (e == hipSuccess) e = ev_n.alloc(n);
        if (e == hipSuccess) e = ver_base.alloc(n / 64 + 1);
        if (e == hipSuccess) e = snap_mask.alloc(n / 64 + 1);
        if (e == hipSuccess) cap_blocks = (long)n;
        else *this = RunPlanWs();
        return e;
    }
};

// stft_kernels.hip
int stft1024_table_count();
void fill_stft1024_table(float2 *host_table, int window_kind);
int launch_stft1024(hipStream_t stream, int n_cu, int fpw_opt, const short *pcm, long n_frames, long hop, float2 *spec,
                    const float2 *table, int read_pass = 0, int touch_wg_per_cu = 0);


int launch_stft1024_half(hipStream_t stream, const short *pcm, long n_frames, float2 *spec, long pitch,
                         const float2 *table);
int launch_stft512(hipStream_t stream, int n_cu, const short *pcm, long n_frames, long hop, float2 *spec,
                   const float2 *table, const float2 *win512);
void fill_win512(float2 *w, int window_kind);
// bins 0..512 of every frame of n_utts ragged utterances in one launch (the layout of launch_stftmask_ragged): global
// frame j is the row spec + j pitch (pitch even); hop 1024 | 512 | 256; run_opt 0 = auto
int launch_stft_half_batch(hipStream_t s, int hop, int run_opt, const short *pcm, const long long *sample_first,
                           const long long *frame_first, long n_utts, long n_frames_total, float2 *spec, long pitch,
                           const float2 *table);

// fft_c2c_kernels.hip
int launch_bitrev_table(hipStream_t stream, short *table_dev, int n_fft, int bits);
int launch_fft_process_f64(hipStream_t stream, const double2 *in, double2 *out, int n_fft, int log2n, long batch,
                           int forward, const double2 *tw);
void fill_c2c_twiddles(double2 *t, int n_fft);
int launch_stft1024_f64(hipStream_t stream, int n_cu, const short *pcm, long n_frames, long hop, const double *table,
                        const double2 *tw512, double2 *out, int variant, int fpw);
int launch_pcm_read_pass(hipStream_t stream, int n_cu, int wg_per_cu, const short *pcm, long n_samples);
void fill_stft1024_f64_table(double *t);          // [1024 window doubles][512 double2 split twiddles]
int launch_dft_direct_f64(hipStream_t stream, int kind, const void *in, double2 *inout, int n, long batch);


// denoise_kernels.hip
// block_len 512 | 256
int launch_vad(hipStream_t s, int block_len, const short *pcm, long n_blocks, const double *w_hi, int use_zcr,
               unsigned char *flags, long long *dbg_energy, int *dbg_zcr);
int launch_run_plan(hipStream_t s, const unsigned char *flags, long n_blocks, const int *run_len_in, int *run_len_out,
                    int latch_run, int *ver_base, unsigned long long *snap_mask, int *events, int *ev_n,
                    DenoisePlan *plan);
int launch_denoise_plan(hipStream_t s, const unsigned char *flags, long n_blocks, const DenoiseState *st_in,
                        DenoiseState *st_out, int *ver_base, unsigned long long *snap_mask, int *events, int *ev_n,
                        DenoisePlan *plan);
int launch_noise_estimate(hipStream_t s, DenoiseGeom g, const short *pcm, long n_blocks, const DenoiseState *st_in,
                          DenoiseState *st_out, const int *events, const int *ev_n, const DenoisePlan *plan,
                          const int *ver_base, const unsigned long long *snap_mask, const float2 *table,
                          const NoiseAccum &acc, float *noise_rows);
// k_opt: the handle's blocks_per_wave option, the run kernel's blocks per wave (0: one round of resident waves;
// 1024-point frames only)
int launch_denoise(hipStream_t s, DenoiseGeom g, int mode, int k_opt, int n_cu, const short *pcm, long n_blocks,
                   long calls_before, const DenoiseState *st_in, DenoiseState *st_out, const int *ver_base,
                   const unsigned long long *snap_mask, const float *noise_rows, const float2 *table, short *out,
                   float *precast, int *redo, const DenoiseShard *shard = nullptr);
int launch_shard_summary(hipStream_t s, DenoiseGeom g, const short *pcm_ext, long n_ext, long ext0, long b0, long b1,
                         const int *events, const int *ev_n, const DenoisePlan *plan, const int *ver_base,
                         const unsigned long long *snap_mask, const float2 *table, int *range, const NoiseAccum &acc,
                         float *rows, float *summary);
int launch_shard_rows(hipStream_t s, DenoiseGeom g, const float *summaries_all, int rank, long b0, long b1,
                      const DenoisePlan *plan, const int *range, const NoiseAccum &acc, float *a_in, float *rows,
                      float *last);
int launch_shard_row0(hipStream_t s, DenoiseGeom g, const float *last_all, int rank, float *rows);
// a batch of ragged utterances, each a fresh 1024-point stream (jdsp_denoise_batch_dev's layout): the VAD, the noise
// pass (one wave per utterance), the run kernel and, for spectral subtraction, the FP64 pass
int launch_denoise_batch(hipStream_t s, int mode, int run_opt, int n_cu, const short *pcm, const long long *sample_first,
                         const long long *block_first, long n_utts, long n_blocks, const double *w_hi,
                         const float2 *table, unsigned char *flags, int *row_idx, float *rows, int *redo, short *out,
                         float *precast, float *noise_last, int vad_only);
// The live streams of a jdsp_denoise handle as a kernel sees them (jdsp_denoise_streams_*, include/jdsp.h): stream s is
// a fresh stream of main() whose statics live here.  What several waves of one launch read and one of them writes is
// held twice, and a word says which copy is current: prev, tail and listed under parity[s], the estimate under
// est_parity[s].  A launch only READS the two words, loads from copy p and stores to copy p ^ 1; denoise_live_commit_kernel,
// enqueued behind the launches, flips parity[s] for the streams that were given blocks, est_parity[s] for those whose
// chunk latched, and adds the blocks to seen[s] (LiveStreams above is the same rule for an overlap-add tail).  The
// running average and the run length are read and written by the one wave that walks the chunk's flags, so one copy.
// Bytes per stream: 4,096 prev + 4,096 tail + 8,192 estimate + 2,560 average + 28 of words = 18,972.
constexpr int kLiveAvgFloats = 640;       // noise_batch_kernel's pair-owned registers: [10][64]
struct DenoiseLive {
    const int *parity;        // [n_streams] 0 | 1
    const int *est_parity;    // [n_streams] 0 | 1
    const long long *seen;    // [n_streams] blocks delivered so far (the reference's call counters)
    int *run_len;             // [n_streams] iNumOfIteration (SS:72), saturated at 11: only == 1, > 1, >= 3, == 10 are asked
    int *listed;              // [2][n_streams] the stream's last frame went to the FP64 pass
    short *prev;              // [2][n_streams][1024] the stream's last two blocks
    float *tail;              // [2][n_streams][512] rgsdOveraped[512..1023] as the run kernel leaves it
    float *avg;               // [n_streams][kLiveAvgFloats] rgsdAveragedNS
    float *rows;              // [2 n_streams][1024] rgdEstimatedNS, copy e of stream s = row e n_streams + s; behind them
                              // the rows latched in the current call, chunk c's from 2 n_streams + c + block_first[c] / 11
    int *latched;             // [n_streams] per CHUNK of the current call: it latched
    long n_streams;
};
// the chunks of live streams: the VAD, the noise pass (one wave per chunk, from the carried state), the run kernel, for
// spectral subtraction the FP64 pass, and the commit.  out and precast may be NULL (the state advances all the same);
// n_emitted may be NULL.  redo: [1 + n_blocks + n_chunks]
int launch_denoise_live(hipStream_t s, int mode, int run_opt, int n_cu, const short *pcm, const long long *stream_id,
                        const long long *sample_first, const long long *block_first, long n_chunks, long n_blocks,
                        const double *w_hi, const float2 *table, unsigned char *flags, int *row_idx, int *redo,
                        const DenoiseLive &lv, int *parity, int *est_parity, long long *seen, short *out, float *precast,
                        long long *n_emitted);
// the n_ids listed streams fresh again
int launch_denoise_live_reset(hipStream_t s, const long long *stream_id, long n_ids, const DenoiseLive &lv, int *parity,
                              int *est_parity, long long *seen);
int ensure_stft1024_table(jdsp_ctx *ctx);
int ensure_vad_window(jdsp_ctx *ctx);
// FP64 Hamming(2 block_len) over the positions a block occupies in the VAD's frame: keep + i, keep = block_len (SS:127-128)
// or block_len - 1 (BeamForming_MVDR_ver1.cpp:37,213-214); cached per context
int ensure_vad_window_ex(jdsp_ctx *ctx, int variant, int block_len, const double **w);
// fastconv_kernels.hip
// (fastconv) Sample `pos` of this call's stream (pos < 0: history carried in the handle).  Samples of
// the first n_hist blocks of a stream never reach the transform in the reference (its queue
// holds uninitialised malloc() blocks for them, :120): they are defined as zero.
struct ConvStream {
    const short *pcm;        // this call's samples
    const short *hist;       // last hist_len samples before this call
    long n_samples;          // in pcm
    long global0;            // global index of pcm[0]
    long valid_from;         // global index of the first sample that exists for the convolver
    int hist_len;
};

int launch_spectrum_to_f32(hipStream_t s, const double2 *in, float2 *out, long n, float scale);
int launch_fastconv(hipStream_t st, int n_fft, const ConvStream &s, long n_out_blocks, int first_block, int block,
                    int n_taps, int n_filters, const float2 *H, const float2 *table, const float2 *tw4096,
                    const float2 *tw8192, short *out, float *precast, long plane, short *hist_out);
void fill_conv_twiddles(float2 *tw4096, float2 *tw8192);
constexpr int kUpolsRowPitch = 520;      // = kUpolsPitch in fastconv_kernels.hip
int launch_spectrum_rows_to_f32(hipStream_t s, const double2 *in, float2 *out, long rows);
int launch_fastconv_upols(hipStream_t st, const ConvStream &s, long n_out_blocks, int first_block, int block, int n_part,
                          int n_filters, const float2 *Hp, const float2 *rect_table, short *staged, float2 *X,
                          short *out, float *precast, long plane, short *hist_out);
int ensure_stft1024_table_rect(jdsp_ctx *ctx);
// binaural_kernels.hip
// The live streams of a jdsp_binaural handle as a kernel sees them (include/jdsp.h, "binaural rendering"): stream s is
// one source as heard in one mix.  Everything it carries is held twice, copy p of stream s at index p n_streams + s, and
// parity[s] says which copy is current -- the rule of LiveStreams and DenoiseLive: the wave of a mix's block 0 reads
// the carried state while the wave of its last block writes the next one, and with more than one block they are not
// the same wave.  A launch only READS parity (the kernel takes it as a __restrict__ argument of its own), loads from
// copy p and stores to copy p ^ 1; binaural_commit_kernel, enqueued behind it, flips parity[s] for the chunks of mixes
// that got blocks.  Bytes per stream, both copies: 2 x (1,024 + 4 + 4 + 4) = 2,072, and 4 of parity.
struct BinauralStreams {
    short *hist;          // [2][n_streams][512] the stream's last 512 samples (zeros: silence before a fresh stream)
    int *dir;             // [2][n_streams] the direction of its last delivery
    float *gain;          // [2][n_streams] ... and the gain, compared as a bit pattern
    int *started;         // [2][n_streams] 0: fresh, (dir, gain) mean nothing and its first delivery does not fade
    long n_streams;
};
// spec: [rows][1024] FP64 spectra of the zero-padded taps; bank: [rows][640] (the layout: binaural_kernels.hip)
int launch_binaural_bank(hipStream_t s, const double2 *spec, float2 *bank, long rows);
// the render launch over n_blocks_total > 0 blocks and the commit behind it; out_i16 and out_f32 may be NULL
int launch_binaural_render(hipStream_t s, const short *pcm, const long long *stream_id, const long long *sample_first,
                           const int *dir, const float *gain, const long long *chunk_first, const long long *block_first,
                           long n_mixes, long n_chunks, long n_blocks_total, const float2 *bank, int n_dirs,
                           const float2 *table, const BinauralStreams &st, int *parity, short *out_i16, float *out_f32,
                           long plane);
int launch_binaural_reset(hipStream_t s, const long long *stream_id, long n_ids, const BinauralStreams &st);
// mvdr_kernels.hip
int launch_mvdr(hipStream_t s, const short *left, const short *right, long n_blocks, long calls_before,
                const MvdrState *st_in, MvdrState *st_out, const int *events, const DenoisePlan *plan,
                const int *ver_base, const unsigned long long *snap_mask, double *delta, double *rver,
                const double2 *steer, const float2 *table, short *out, float *precast, float4 *wtab,
                double *tile_sums);
int launch_mvdr_corr_total(hipStream_t s, const short *left, const short *right, long n_blocks, const MvdrState *st_in,
                           const int *events, const DenoisePlan *plan, const float2 *table, double *delta, double *total,
                           double *tile_sums);
int launch_mvdr_apply(hipStream_t s, const short *left, const short *right, long n_blocks, long calls_before,
                      const MvdrState *st_in, MvdrState *st_out, const int *ver_base, const unsigned long long *snap_mask,
                      const double *rver, const double2 *steer, const float2 *table, short *out, float *precast);
int launch_mvdr_shard_summary(hipStream_t s, const short *left_ext, const short *right_ext, long n_ext, long ext0,
                              long b0, long b1, const MvdrState *zero_state, const int *events,
                              const DenoisePlan *plan, const int *ver_base, const unsigned long long *snap_mask,
                              const float2 *table, int *range, double *delta, double *total, double *tile_sums);
int launch_mvdr_shard_finish(hipStream_t s, const short *left_ext, const short *right_ext, long n_ext, long ext0,
                             long b0, long b1, const MvdrState *zero_state, MvdrState *scratch_state,
                             const DenoisePlan *plan, const int *ver_base, const unsigned long long *snap_mask,
                             const int *range, const double *delta, const double *sums_all, int rank, double *rver,
                             const double2 *steer, const float2 *table, short *out, float *precast, double *tile_sums);
// mvdrn_kernels.hip
int launch_mvdrn(hipStream_t s, const short *pcm, long chan_stride, int n_mics, long n_blocks, long calls_before,
                 const short *prev_in, short *prev_out, const int *events, const DenoisePlan *plan, const int *ver_base,
                 const unsigned long long *snap_mask, float2 *spec, const double2 *cov_in, double2 *cov_out,
                 const double2 *steer, double loading, float2 *weights, const float2 *table, short *out, float *precast, double2 *chunk_ws, int chunk_cap);
int launch_mvdrn512(hipStream_t s, const short *pcm, long chan_stride, int n_mics, long n_blocks, long calls_before,
                    const short *prev_in, short *prev_out, const int *events, const DenoisePlan *plan, const int *ver_base,
                    const unsigned long long *snap_mask, float2 *spec, const double2 *cov_in, double2 *cov_out,
                    const double2 *steer, double loading, float2 *weights, const float2 *table, short *out, float *precast, double2 *chunk_ws, int chunk_cap);
// mvdrn_batch_kernels.hip
// The workspace of a batch of ragged utterances as the launcher sees it (jdsp_mvdrn::BatchWs owns it), for up to n
// blocks in up to U utterances; P = kMvnBatchEvents.
struct MvnBatchView {
    unsigned char *code;   // [n] voice | first block of its utterance << 1
    int *evpre;            // [n] estimation frames at or before each block of the concatenated axis: its weight row
    int *events;           // [n] the block of every estimation frame
    int *tile_off;         // [n / 2048 + 2] the prefix sum's tile offsets
    int *ev_first;         // [U + 1] the first estimation frame of every utterance
    int *slot_utt;         // [U + n / P + 2] the utterance of every chunk slot
    float2 *spec;          // [n][n_mics][513]
    float2 *weights;       // [n + 1][8][513]; row 0: no estimation frame yet
    double2 *chunk;        // [2 n / P + 2][513][64] chunk sums, then entering matrices, of utterances of more than P events
};
// every utterance a fresh 1024-point stream; flags, out and precast may each be NULL (out and precast both NULL: the
// VAD alone runs).  Enqueues only: no allocation, no synchronisation, no host read of the offsets.
int launch_mvdrn_batch(hipStream_t s, const short *pcm, long chan_stride, int n_mics, const long long *sample_first,
                       const long long *block_first, long n_utts, long n_blocks, const double *w_vad, const double2 *steer,
                       double loading, const float2 *table, const MvnBatchView &ws, unsigned char *flags, short *out,
                       float *precast);
// mvdrn_live_kernels.hip
// The live streams of a jdsp_mvdrn handle as a kernel sees them (jdsp_mvdrn_streams_*, include/jdsp.h), and the
// workspace of one delivery of up to n blocks in up to n_streams chunks.  Everything a stream carries is held ONCE
// (DESIGN.md 3.13): its covariance is read and written by the one wave that walks its eight bins, and the carried
// blocks, the count and the carried word are written by the delivery's last launch, which nothing of the delivery follows.
// Bytes per stream: 525,312 covariance + 8,192 carried blocks + 8 + 4 = 533,516.
struct MvnLive {
    double2 *cov;          // [n_streams][513][64] the running sum, the handle's own layout
    short *prev;           // [n_streams][8][512] the stream's last block of every microphone
    long long *seen;       // [n_streams] blocks delivered so far
    int *word;             // [n_streams] bit 0: the stream's last block was quiet; above it its estimation frames so
                           // far, saturated at 8 (0 for a fresh stream)
    long n_streams;
    unsigned char *code;   // [n] the VAD's decision per block of the concatenated axis
    int *row;              // [n] estimation frames of its chunk at or before each block: its weight row in the chunk
    int *events;           // [n] chunk c's estimation frames as blocks of the chunk, from block_first[c] on
    int *ev_n;             // [n_streams] their number, per chunk
    float2 *spec;          // [n][n_mics][513] spectra of the estimation frames, chunk c's from row block_first[c] on
    float2 *weights;       // [n + n_streams][8][513] chunk c's rows from block_first[c] + c on: the carried matrix, then
                           // one per estimation frame
};
// the chunks of live streams: VAD, plan, event spectra, update, apply and the state; flags, out and precast may each be
// NULL (the state advances all the same).  Enqueues only.
int launch_mvdrn_live(hipStream_t s, const short *pcm, long chan_stride, int n_mics, const long long *stream_id,
                      const long long *sample_first, const long long *block_first, long n_chunks, long n_blocks,
                      const double *w_vad, const double2 *steer, double loading, const float2 *table, const MvnLive &lv,
                      unsigned char *flags, short *out, float *precast);
// the n_ids listed streams fresh again
int launch_mvdrn_live_reset(hipStream_t s, const long long *stream_id, long n_ids, const MvnLive &lv);
// pitch_kernels.hip
int launch_pitch(hipStream_t s, const short *pcm, long n_blocks, const short *prev_block, const float2 *table, int *arg,
                 float *rmax, float *autocorr);
// timedomain_kernels.hip
// method 2 (AMDF) | 3 (autocorrelation); arg, value and curve may each be NULL
int launch_pitch_lag(hipStream_t s, int method, const short *pcm, long n_blocks, const short *prev_block, int *arg,
                     double *value, double *curve);
// win: [2 block_len] FP64 window; autocorr ([order + 1] per block) may be NULL
int launch_lpc(hipStream_t s, const short *pcm, long n_blocks, int block_len, int order, const short *prev_block,
               const double *win, double *autocorr, double *lpc);
// streamfilter_kernels.hip
// coeff: [n_sections][2][3] doubles; state: [n_streams][n_sections + 1][2] int16; precast may be NULL
int launch_geq(hipStream_t s, const short *pcm, long n_streams, long n_samples, long pitch, const double *coeff,
               int n_sections, short *state, short *out, double *precast);
// coef: [n_streams][filter_len] doubles; keep: [n_streams][filter_len - 1] int16; precast may be NULL
int launch_nlms(hipStream_t s, const short *input, const short *refsig, long n_streams, long n_samples, long pitch,
                int filter_len, double mu, double compensation, double *coef, short *keep, short *est, short *err,
                double *precast);
// istft_kernels.hip
// ws: [n_fft] synthesis window / n_fft; g: [hop] WOLA gain; tails: [n_fft - hop] floats; run_opt 0 = auto
int launch_istft(hipStream_t s, int n_cu, int n_fft, int hop, int half, const float2 *spec, long pitch, long n_frames,
                 const float *ws, const float *g, const float *tail_in, float *tail_out, short *out, float *out_f32,
                 const float2 *table, int run_opt);
int launch_istft_flush(hipStream_t s, const float *tail, const float *g, int n_tail, int hop, short *out, float *out_f32);
// The live streams of a handle as a kernel sees them (the host side: OlaStreams, ola_api.h).  Stream s keeps two tails of
// n_tail = n - hop floats, tails[(p n_streams + s) n_tail ..) for p = 0, 1, and the word parity[s] says which of them
// holds the partial sums the stream's next chunk starts from.  A transform launch only READS parity: every wave of it
// sees the same value, loads from tail p and stores to tail p ^ 1, so the waves that read a chunk's carried tail (all
// whose halo starts at the chunk's first frame) and the one wave that writes its new tail (the owner of its last
// frame) never touch the same memory, whatever order they run in.  launch_ola_streams_commit, enqueued behind the
// launch, flips parity[s] for the streams that were given frames.  Nothing of it is host state, so a captured launch
// replays correctly, and a stream without a chunk in a call is not touched at all.  (A word, not a byte: gfx950 has no
// scalar byte load.  The live kernels take stream_id and parity a second time as __restrict__ arguments of their own:
// through this struct the compiler cannot tell them from the tails the kernel stores to, and fetched both with vector
// loads and v_readfirstlane at every chunk boundary inside a run: profiles/r18_ola_live_streams_isa.txt.)
struct LiveStreams {
    const long long *stream_id;   // [n_chunks] the stream of chunk c; distinct within a call, in [0, n_streams)
    const int *parity;            // [n_streams] 0 | 1
    float *tails;                 // [2][n_streams][n_tail]
    long n_streams;
    int n_tail;
};
// n_spans independent streams in one launch, no tail in or out: the layout of launch_stftmask_ragged with spectrum rows
// where that has mask rows.  live != NULL: the spans are chunks of live streams; chunk c starts from the tail of stream
// live->stream_id[c], writes its hop F_c samples and leaves the new tail in the stream's other buffer
int launch_istft_ragged(hipStream_t s, int n_cu, int n_fft, int hop, int half, const float2 *spec, long pitch,
                        long n_frames_total, const long long *sample_first, const long long *frame_first, long n_spans,
                        const LiveStreams *live, const float *ws, const float *g, short *out, float *out_f32,
                        const float2 *table, int run_opt);
// the n_tail samples of the n_ids listed streams (live.stream_id) to sample_first[i] onwards, their tails zeroed behind
// them; out and out_f32 both NULL (sample_first is then not read): the reset of those streams
int launch_ola_streams_flush(hipStream_t s, const LiveStreams &live, long n_ids, const long long *sample_first,
                             const float *g, int hop, short *out, float *out_f32);
// parity[stream_id[c]] ^= 1 for the chunks with frames
int launch_ola_streams_commit(hipStream_t s, const long long *stream_id, const long long *frame_first, long n_chunks,
                              int *parity);
// stftmask_kernels.hip (n_fft 1024)
// mask: rows of float or float2 (complex_mask), pitch elements apart (0: one row); wa: [1024] analysis window / 2;
// ws: [1024] synthesis window; g: [hop] emission gain; tails: [1024 - hop] floats; run_opt 0 = auto.  For the frames
// FP32 cannot hold (stftmask_unsafe) -- f64: [3072] the analysis window, the synthesis window (both unrounded) and
// exp(-2 pi i t / 1024), t < 512, as (re, im) pairs; count: two words, the emitted ones among them are added to
// count[epoch & 1] and the other is zeroed for the next call (epoch: the host's number of the call)
int launch_stftmask(hipStream_t s, int n_cu, int hop, int complex_mask, const short *pcm, const void *mask, long pitch,
                    long n_frames, const float *wa, const float *ws, const float *g, const float *tail_in,
                    float *tail_out, short *out, float *out_f32, const float2 *table, int run_opt, const double *f64,
                    unsigned int *count, unsigned int epoch);
// n_spans independent streams in one launch, no tail in or out: utterance u is the frames (= mask rows) frame_first[u] ..
// frame_first[u + 1] - 1 of n_frames_total and reads and writes from sample sample_first[u] (even) of pcm and out on
// (device arrays, [n_spans] and [n_spans + 1]).  live != NULL: the spans are chunks of live streams, as launch_istft_ragged's
int launch_stftmask_ragged(hipStream_t s, int n_cu, int hop, int complex_mask, const short *pcm, const void *mask,
                           long pitch, long n_frames_total, const long long *sample_first, const long long *frame_first,
                           long n_spans, const LiveStreams *live, const float *wa, const float *ws, const float *g,
                           short *out, float *out_f32, const float2 *table, int run_opt, const double *f64,
                           unsigned int *count, unsigned int epoch);
// mfcc_kernels.hip
// ---- GMM / HMM (gmm_kernels.hip) ----
// packed per-GMM record (doubles): alpa[4], mean[4][4], var[4][4], coef[4][4], eig[4][12][4], and for the
// fused evaluation nhiv[4][4] = -0.5 / var and cprod[4] = the product of a mixture's four coef
constexpr int kGmmAlpa = 0, kGmmMean = 4, kGmmVar = 20, kGmmCoef = 36, kGmmEig = 52, kGmmNhiv = 244, kGmmCprod = 260,
              kGmmRecord = 264;
constexpr int kGmmMaxClasses = 256;
int launch_gmm_score(hipStream_t stream, const double *feats, long n_frames, const long long *utt_first, long n_utts,
                     const double *gmm, int n_classes, int fused, double *scores, int *best);
int launch_hmm_viterbi(hipStream_t stream, const double *feats, long n_frames, const long long *utt_first, long n_utts,
                       const double *gmm, const double *log_trans, int n_models, int fused, double log_init, double *b,
                       double *scores, int *best, int *path, double *trellis);
int launch_mfcc(hipStream_t s, const short *pcm, const long long *starts, long n_frames, const MfccDev &p,
                const float2 *table, double *feats, int *redo);

// ---- GMM training (gmm_train_kernels.hip) ----
// Per-class training state in HBM (doubles, then ints): what Train: keeps in its GMMParameter between files, plus the
// stats of jdsp_gmm_train_stats.
constexpr int kTrAlpa = 0, kTrMean = 4, kTrCov = 52, kTrCost = 628, kTrDoubles = 629;
constexpr int kTrSeen = 0, kTrPasses = 1, kTrCapped = 2, kTrSelected = 3, kTrFiles = 7, kTrStatus = 8, kTrInts = 9;
struct GmmTrainState {
    double d[kTrDoubles];
    int i[kTrInts];
    int pad;
};
constexpr int kGmmTrainMaxClasses = 1024;
int launch_gmm_train(hipStream_t s, int threads, int n_classes, const double *feats, long n_frames,
                     const long long *file_first, const int *file_class, long n_files, int kmeans_max_passes,
                     GmmTrainState *state, unsigned char *sel, double *wbuf);
int launch_gmm_train_params(hipStream_t s, int n_classes, const GmmTrainState *state, jdsp_gmm_train_param *out);

}  // namespace jdsp

struct jdsp_denoise {
    jdsp_ctx *ctx = nullptr;
    int mode = 0;
    long calls = 0;                       // blocks consumed so far (the reference's call counters)
    jdsp::DevBuf<jdsp::DenoiseState> st[2];
    int cur = 0;                          // st[cur] is the state the next call reads
    const double *w_hi = nullptr;         // borrowed: the VAD's window, second half of the FP64 Hamming(2 block) -- the context's or w_hi256
    jdsp::DevBuf<jdsp::DenoisePlan> plan;
    // sized by jdsp_denoise_reserve for calls of up to run.cap_blocks blocks
    struct Workspace {
        jdsp::RunPlanWs run;
        jdsp::DevBuf<long long> dbg_energy;
        jdsp::DevBuf<int> dbg_zcr;
        jdsp::DevBuf<float> rows;         // [n / 10 + 2][1024] latched estimates of the call (row 0: the one carried in)
        // jdsp::NoiseAccum's arrays
        jdsp::DevBuf<float> chunk_alpha, chunk_beta, a_start, lat_alpha;
        jdsp::DevBuf<int> lat_chunk;
        jdsp::DevBuf<int> redo;           // [n + 1] {count, frames...}: spectral-subtraction frames computed again in FP64
    } ws;
    // sized by jdsp_denoise_batch_reserve for batches of up to cap_blocks blocks in up to cap_utts utterances
    struct BatchWs {
        jdsp::DevBuf<unsigned char> flags; // [n] the VAD's decision per block of the batch
        jdsp::DevBuf<int> row_idx;         // [n] the latched row in force at each block
        jdsp::DevBuf<float> rows;          // [n / 10 + 1][1024]; row 0 stays zero: no estimate latched yet
        jdsp::DevBuf<int> redo;            // [n + 1] {count, frames...} as ws.redo
        long cap_blocks = -1, cap_utts = -1;
    } bws;
    // sized by jdsp_denoise_streams_reserve: n_streams live streams (jdsp::DenoiseLive) and the workspace of one call
    // over up to cap_blocks blocks.  Nothing here is read or written by the handle's own stream or the batch entries.
    struct LiveWs {
        long n_streams = 0, cap_blocks = 0;  // n_streams 0: not reserved
        jdsp::DevBuf<char> state;          // one allocation: what DenoiseLive carries per stream, but the estimates
        jdsp::DevBuf<float> rows;          // [2 n_streams + n_streams + cap_blocks / 11 + 2][1024]: DenoiseLive::rows
        jdsp::DevBuf<unsigned char> flags; // [cap_blocks]
        jdsp::DevBuf<int> row_idx;         // [cap_blocks]
        jdsp::DevBuf<int> redo;            // [1 + cap_blocks + n_streams] {count, frames...}
        jdsp::DevBuf<int> latched;         // [n_streams]
        jdsp::DenoiseLive view;            // pointers into the above
        int *parity = nullptr, *est_parity = nullptr;   // the three words only the commit and reset kernels write
        long long *seen = nullptr;
    } lws;
    long last_blocks = 0;
    int redo_valid = 0;                   // the last call's count is there for jdsp_denoise_frames_recomputed: 1 in ws.redo[0], 2 in bws.redo[0], 3 in lws.redo[0]
    int opt_k = 0;
    int opt_vad_trace = 0;                // 1: keep every block's energy sum and ZCR for jdsp_denoise_vad_trace (slower VAD kernel)
    int last_trace_valid = 0;             // the option's value when the last call ran: what jdsp_denoise_vad_trace may hand out
    int n_fft = 1024, block = 512;        // FFT_PROCESSING_SIZE, BLOCK_LEN = KEEP_LEN (SS:53-55); 512 / 256 also built
    jdsp::DevBuf<double> w_hi256;         // 512-point frames: second half of the FP64 Hamming(512) (VAD)
    jdsp::DevBuf<float> win512h;          // 512-point frames: 0.5 * Hamming(512), natural order
    // sharded (multi-GPU) run in progress: jdsp_denoise_shard_*
    long sh_ext0 = 0, sh_b0 = 0, sh_b1 = 0, sh_total = 0;
    const int16_t *sh_pcm = nullptr;      // borrowed: the caller's PCM of the run
    jdsp::DevBuf<int> sh_range;           // {first event, one past last event, latches before the shard}
    jdsp::DevBuf<float> sh_a_in;          // [1024]
    jdsp::DevBuf<int> sh_zero_run;        // a zero (run length entering a fresh global stream)
};

struct jdsp_mfcc {
    jdsp_ctx *ctx = nullptr;
    jdsp_mfcc_cfg cfg;
    jdsp::MfccDev dev;                    // its pointers are views into blob
    jdsp::DevBuf<char> blob;              // one device allocation holding every table
    jdsp::DevBuf<int> redo;               // 512-FFT configurations: {count, frames or frame pairs to compute again in FP64} (mfcc_redo_f64_kernel)
    std::vector<double> mel_freqs, fbank;
    std::vector<int> fi_bins;
    // FP64 tables of the separately callable sub-steps (stage_api.hip), built on first use
    jdsp::DevBuf<char> stage_blob;
    const double *stage_fb = nullptr, *stage_cos = nullptr, *stage_lift = nullptr;   // views into stage_blob
    const int *stage_fi = nullptr;
};

struct jdsp_gmm {
    jdsp_ctx *ctx = nullptr;
    int n_classes = 0;
    int fused = 0;                        // "evaluation" option: 0 the reference's operation order, 1 fused
    jdsp::DevBuf<double> records;         // [n_classes][kGmmRecord]
};

struct jdsp_gmm_trainer {
    jdsp_ctx *ctx = nullptr;
    int n_classes = 0;
    int threads = 256;                    // "threads_per_class"
    int kmeans_max_passes = 10000;        // "kmeans_max_passes"
    jdsp::DevBuf<jdsp::GmmTrainState> state;   // [n_classes]
    jdsp::DevBuf<jdsp_gmm_train_param> out;    // [n_classes]: the host entry's staging of jdsp_gmm_train_params
    jdsp::DevBuf<unsigned char> sel;      // [frames]: k-means Selection bits
    jdsp::DevBuf<double> wbuf;            // [frames][4]: E-step weights
};

struct jdsp_geq {
    jdsp_ctx *ctx = nullptr;
    int n_sections = 0;
    long n_streams = 0;
    jdsp::DevBuf<double> coeff;           // [n_sections][2][3]
    jdsp::DevBuf<short> state;            // [n_streams][n_sections + 1][2]
};

struct jdsp_nlms {
    jdsp_ctx *ctx = nullptr;
    int filter_len = 0;
    long n_streams = 0;
    double mu = 0, compensation = 0;
    jdsp::DevBuf<double> coef;            // [n_streams][filter_len]
    jdsp::DevBuf<short> keep;             // [n_streams][filter_len - 1]
};

struct jdsp_hmm {
    jdsp_ctx *ctx = nullptr;
    int n_models = 0;
    int fused = 0;                        // "evaluation" option, as jdsp_gmm
    jdsp::DevBuf<double> records;         // [n_models * 6][kGmmRecord]
    jdsp::DevBuf<double> log_trans;       // [n_models][6][6], log() taken on the host
    jdsp::DevBuf<double> emission;        // scratch [frames][n_models * 6], grown on demand
};

struct jdsp_fastconv {
    jdsp_ctx *ctx = nullptr;
    int n_fft = 0, n_taps = 0, n_filters = 0, block = 0, n_hist = 0;
    jdsp::DevBuf<float2> H;               // [n_filters][n_fft]
    // uniformly partitioned path (n_fft 8192, block % 512 == 0): see fastconv_kernels.hip
    int n_part = 0;                       // 0: not used
    jdsp::DevBuf<float2> Hp;              // [n_filters][n_part][520]: bins 0..512 of every 512-tap partition
    jdsp::DevBuf<short> staged;           // [512 n_part + samples of a call]
    jdsp::DevBuf<float2> X;               // [frames][520]
    long ws_samples = 0;                  // samples per call the workspace is sized for
    jdsp::DevBuf<short> hist[2];          // last hist_len samples of the stream, ping-pong
    int hist_len = 0;                     // n_taps - 1; partitioned: 512 n_part, every sample a call's first frames read
    int cur = 0;
    long calls = 0;                       // blocks consumed so far (siNumOfCount)
};

struct jdsp_binaural {
    jdsp_ctx *ctx = nullptr;
    int n_dirs = 0, n_taps = 0;
    jdsp::DevBuf<float2> bank;            // [n_dirs][2][640]: binaural_kernels.hip
    // sized by jdsp_binaural_streams_reserve
    long n_streams = 0;                   // 0: not reserved
    jdsp::DevBuf<char> state;             // one allocation: what BinauralStreams carries, and the parity words
    jdsp::BinauralStreams view{};         // pointers into it
    int *parity = nullptr;                // [n_streams]: only the commit kernel (and a reset of all) writes it
};

struct jdsp_mvdr {
    jdsp_ctx *ctx = nullptr;
    double d_time = 0;
    long calls = 0;
    jdsp::DevBuf<jdsp::MvdrState> st[2];
    int cur = 0;
    jdsp::DevBuf<jdsp::DenoisePlan> plan;
    jdsp::DevBuf<double2> steer;          // [1024] steering vector's second component per bin
    jdsp::DevBuf<double> w_vad;           // Hamming[511 .. 1022] in FP64
    // sized by mvdr_reserve for calls of up to n = run.cap_blocks blocks
    struct Workspace {
        jdsp::RunPlanWs run;
        jdsp::DevBuf<double> delta, rver;
        jdsp::DevBuf<double> tile_sums;   // [n / 1024 + 1][4] sums of the prefix pass's tiles of 1024 events
        jdsp::DevBuf<float4> wtab;        // [min(n + 1, kMvdrTableVersions)][1024] per-version weights (mvdr_weights_kernel)
    } ws;
    // sharded (multi-GPU) run in progress
    long sh_ext0 = 0, sh_b0 = 0, sh_b1 = 0, sh_total = 0;
    const int16_t *sh_left = nullptr, *sh_right = nullptr;   // borrowed: the caller's channels of the run
    jdsp::DevBuf<int> sh_range;           // {first event, one past last, versions before the shard}
    jdsp::DevBuf<int> sh_zero_run;
};

struct jdsp_mvdrn {
    jdsp_ctx *ctx = nullptr;
    int n_mics = 0;
    int n_fft = 1024, block = 512, n_bins = 513;   // FFT_PROCESSING_LEN, BLOCK_LEN, bins kept (1024 / 512 / 513 or 512 / 256 / 257)
    double loading = 0;
    long calls = 0;
    int cur = 0;
    jdsp::DevBuf<double2> cov[2];         // [513][64] per-bin covariance, ping-pong
    jdsp::DevBuf<short> prev[2];          // [8][512] previous block per microphone
    jdsp::DevBuf<int> run_len[2];
    jdsp::DevBuf<jdsp::DenoisePlan> plan;
    jdsp::DevBuf<double2> steer;          // [513][8]
    jdsp::DevBuf<double> w_vad;
    // sized by mvdrn_reserve for calls of up to run.cap_blocks blocks
    struct Workspace {
        jdsp::RunPlanWs run;
        jdsp::DevBuf<float2> spec, weights;
        jdsp::DevBuf<double2> chunk_ws;   // [2][chunk_cap][n_bins][64]: per-chunk covariance sums and entering matrices
        int chunk_cap = 0;
    } ws;
    // sized by jdsp_mvdrn_batch_reserve for batches of up to cap_blocks blocks in up to cap_utts utterances
    // (jdsp::MvnBatchView has the shapes); nothing here is read or written by the handle's own stream
    struct BatchWs {
        jdsp::DevBuf<unsigned char> code;
        jdsp::DevBuf<int> evpre, events, tile_off, ev_first, slot_utt;
        jdsp::DevBuf<float2> spec, weights;
        jdsp::DevBuf<double2> chunk;
        long cap_blocks = -1, cap_utts = -1;
    } bws;
    // sized by jdsp_mvdrn_streams_reserve: n_streams live streams and the workspace of one delivery (jdsp::MvnLive has
    // the shapes); apart from the handle's own stream and from the batch workspace
    struct LiveWs {
        long n_streams = 0, cap_blocks = 0;   // n_streams 0: not reserved
        jdsp::DevBuf<char> state;             // covariances, carried blocks, counts and quiet bits in one allocation
        jdsp::DevBuf<unsigned char> code;
        jdsp::DevBuf<int> row, events, ev_n;
        jdsp::DevBuf<float2> spec, weights;
        jdsp::MvnLive view = {};
    } lws;
};
