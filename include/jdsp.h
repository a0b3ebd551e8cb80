/*
 * jdsp.h -- C ABI of the MI355X (gfx950) engine behind JeicybooDSP's FFT-based
 * spectral path.  Plain C, plain pointers and sizes; no C++/torch types.
 *
 * The reference (phoenix163/JeicybooDSP) has no plugin/FFI layer: its seam is
 * the per-block free function each program's main() calls.  Every entry point
 * below names the reference function(s) (file:line) whose work it performs for
 * a whole batch of blocks at once; jeicyboodsp_amd/compat/ keeps the
 * reference's own per-block C++ signatures on top of this ABI, and
 * INTEGRATION.md shows the binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success and a negative JDSP_E* code on
 *     failure, never throws; jdsp_last_error() gives the text for the handle.
 *   - a jdsp_ctx is confined to one host thread / one stream of audio at a
 *     time (the reference's functions are non-re-entrant: static state in
 *     every per-block function, e.g. SpectralSubtraction_final.cpp:202,208-209;
 *     here that state lives in the handle).
 *   - "_dev" entry points take DEVICE pointers and only enqueue work on the
 *     handle's HIP stream: no allocation and no synchronisation once the
 *     handle is warm, i.e. after one call of that entry point (constant tables
 *     are built on first use) and after the matching *_reserve() where the
 *     entry has a workspace (jdsp_denoise_reserve, jdsp_denoise_batch_reserve, jdsp_mvdrn_batch_reserve,
 *     jdsp_reverb_batch_reserve, jdsp_reverb_streams_reserve, jdsp_hmm_reserve, jdsp_fastconv_reserve,
 *     jdsp_*_streams_reserve).
 *     The plain entry points take HOST pointers, copy in, run, copy out and
 *     synchronise.
 *   - GRAPH CAPTURE.  A warm "_dev" call can be captured into a hipGraph (bench.py
 *     does that; tests/test_graph_replay_gpu.py captures every entry named here).
 *     What a replay of the captured call does depends on where the entry's state
 *     lives, in three classes.
 *       Baked and live arguments, all classes: every SCALAR (n_frames, n_blocks, n_utts, n_chunks, n_ids,
 *       n_frames_total, n_blocks_total, pitches, hops, methods, orders) and every POINTER is baked into the graph at
 *       capture.  Read at replay: the CONTENTS of the buffers, and with them the device-side offset and id arrays
 *       (sample_first, frame_first, block_first, utt_first, frame_start, stream_id, ir, gain).  A replay may therefore deal the same
 *       n_frames_total among the same n_utts / n_chunks differently, move the spans, and name other streams.
 *       Class S, stateless: jdsp_stft_i16_dev, jdsp_stft_half_i16_dev, jdsp_stft_i16_f64_dev, jdsp_stft_half_batch_dev,
 *         jdsp_istft_batch_dev, jdsp_stftmask_batch_dev, jdsp_denoise_batch_dev, jdsp_mvdrn_batch_dev,
 *         jdsp_reverb_batch_dev, jdsp_mfcc_frames_dev,
 *         jdsp_pitch_autocorr_dev, jdsp_pitch_lag_dev, jdsp_lpc_dev, jdsp_gmm_score_dev, jdsp_hmm_viterbi_dev,
 *         jdsp_fft_process_f64_dev.  Every replay recomputes from what the buffers hold at that time and equals an
 *         eager call on the same contents, bit for bit.  Replay as often as wanted.
 *       Class D, state on the device only: jdsp_geq_process_dev, jdsp_nlms_process_dev, and the live streams
 *         jdsp_stftmask_streams_dev / _streams_flush_dev / _streams_reset_dev and jdsp_istft_streams_dev /
 *         _streams_flush_dev / _streams_reset_dev, and jdsp_denoise_streams_dev / jdsp_denoise_streams_reset_dev
 *         (their *_reserve: jdsp_denoise_streams_reserve), and jdsp_binaural_render_dev /
 *         jdsp_binaural_streams_reset_dev (jdsp_binaural_streams_reserve), and jdsp_mvdrn_streams_dev /
 *         jdsp_mvdrn_streams_reset_dev (jdsp_mvdrn_streams_reserve), and jdsp_reverb_streams_dev /
 *         jdsp_reverb_streams_reset_dev (jdsp_reverb_streams_reserve).  EVERY REPLAY ADVANCES THE STREAMS: it continues from the state the
 *         replay (or eager call) before it left, exactly as another eager call would.  Replay as often as wanted.
 *       Class H, state the host carries (which ping-pong copy is current, the stream position, passed to the kernels
 *         as arguments): jdsp_istft_process_dev / _flush_dev, jdsp_stftmask_process_dev / _flush_dev,
 *         jdsp_denoise_process_dev, jdsp_fastconv_process_dev, jdsp_mvdr_process_dev, jdsp_mvdrn_process_dev.  A
 *         captured call BELONGS TO THE HANDLE'S POSITION AT CAPTURE.  The host state advances when the call is
 *         captured; the device catches up when the graph is replayed.  So the graph (of one call or of several
 *         consecutive ones) may be replayed ONCE, there: nothing else may touch the handle between the capture and that
 *         replay, and the handle's reset (or a flush, which resets) invalidates the graph.  A second replay reads the
 *         stale copy and gives a wrong stream WITHOUT AN ERROR.  The replayable form of a jdsp_istft / jdsp_stftmask
 *         stream is the same handle's live-stream entries with n_streams = 1 (class D).
 *     The shard entries and the training entries are not covered by this promise.
 *   - spectra are interleaved (re, im) float pairs, full length n_fft per frame
 *     exactly like the reference's fftw_complex[FFT_PROCESSING_SIZE] buffers
 *     (SpectralSubtraction_final.cpp:205-206), in single precision.
 */
#ifndef JDSP_H
#define JDSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: jdsp_vad_blocks_ex added; jdsp_denoise_apply and jdsp_denoise_shard_* accept 512-point streams;
 *    jdsp_denoise_vad_trace's energies / counts follow the option's value at the time of the traced call;
 *    jdsp_set_option("stft.read_pass") accepts -1 / 0 / 1 only; the STFT synthesis entries jdsp_istft_* added;
 *    the GMM training entries jdsp_gmm_train_* and jdsp_gmm_param_from_train added; the time-domain pitch entries
 *    jdsp_pitch_lag* (AMDF, autocorrelation) and the LPC entries jdsp_lpc* added; the multi-stream IIR equaliser
 *    jdsp_geq_* and NLMS filter jdsp_nlms_* added; the fused STFT masking entries jdsp_stftmask_* added;
 *    jdsp_denoise_frames_recomputed added; the batched masking entries jdsp_stftmask_batch* added; the ragged-batch
 *    analysis and synthesis entries jdsp_stft_half_batch* and jdsp_istft_batch* added;
 *    jdsp_stftmask_frames_recomputed added; the batched denoise entries jdsp_denoise_batch* added; the live-stream
 *    entries jdsp_stftmask_streams* and jdsp_istft_streams* added; the live denoise streams jdsp_denoise_streams* added;
 *    live binaural rendering jdsp_binaural_* added; the batched n-microphone MVDR entries jdsp_mvdrn_batch* added;
 *    the live n-microphone MVDR streams jdsp_mvdrn_streams* added; batched reverberation jdsp_reverb_* added;
 *    the live reverberation streams jdsp_reverb_streams* added
 *    (backward compatible: nothing before them changed).  (1: rounds 1-2.) */
#define JDSP_ABI_VERSION 2

enum {
    JDSP_OK = 0,
    JDSP_EINVAL = -1,   /* bad argument / unsupported size */
    JDSP_EHIP = -2,     /* a HIP runtime call failed */
    JDSP_ENOMEM = -3,
    JDSP_ENODEV = -4    /* no gfx950 device / device ordinal out of range */
};

typedef struct jdsp_ctx jdsp_ctx;
typedef struct { float re, im; } jdsp_c32;

/* ---- handle ---------------------------------------------------------------- */
int jdsp_abi_version(void);
/* Creates a handle on HIP device `device`.  Fails with JDSP_ENODEV when there
 * is no GPU: there is no CPU fallback in this library. */
int jdsp_create(int device, jdsp_ctx **out);
int jdsp_destroy(jdsp_ctx *ctx);
const char *jdsp_last_error(const jdsp_ctx *ctx);   /* ctx may be NULL: global creation error */
/* Enqueue on a caller-owned hipStream_t (e.g. the caller framework's current
 * stream).  The value is used as given: NULL is HIP's default (null) stream.
 * jdsp_use_own_stream() goes back to the handle's private non-blocking stream.
 * When the stream actually changes, everything the handle (and its stream objects:
 * create/reset memsets, state carried between process calls) has enqueued on the
 * old stream is ordered before what follows on the new one (event record + wait;
 * no host synchronisation).  Exception: if either stream is being captured into a
 * hipGraph no event is inserted and that ordering is the caller's. */
int jdsp_set_stream(jdsp_ctx *ctx, void *hip_stream);
int jdsp_use_own_stream(jdsp_ctx *ctx);
/* Tuning knobs, by name; unknown names return JDSP_EINVAL.
 *   "stft.frames_per_wave"  consecutive frames one wavefront owns (0 = auto); for jdsp_stft_half_batch* the run of
 *                           global frames one wavefront walks across utterances (0 = 4).  Results are identical.
 *   "stft.read_pass"        -1 (default, auto) / 0 / 1: before the hop-512 transform of a large batch, one
 *                           read-only launch streams the PCM into the 256 MiB Infinity Cache, slab by slab, so
 *                           that HBM sees a read stream and then a write stream instead of their 1 : 8 mix
 *                           (65,536 frames whose PCM is in HBM: 98 us against 147 us; PCM that is already
 *                           cache-resident pays 9 us for nothing -- 0 turns the pass off).  Results are identical.
 *                           The FP64 analysis (jdsp_stft_i16_f64*) takes the same pass.
 *   "stft.f64_kernel"       0 (default): the FP64 analysis at four waves per SIMD (twiddles as powers of one value
 *                           per family); 1: round 2's kernel (all tables in registers, two waves per SIMD) -- A/B
 *   "stft.f64_frames_per_wave"  frames one wave of the FP64 analysis walks (0 = one round of resident waves)
 *   "stft.window"           window of jdsp_stft_*: 0 = the reference's Hamming
 *                           0.54-0.46cos(2*3.141592*i/(n-1)) (default), 1 = Hann 0.5-0.5cos(same).
 *                           The denoise / MFCC / pitch chains always use what the reference uses. */
int jdsp_set_option(jdsp_ctx *ctx, const char *name, long value);
int jdsp_synchronize(jdsp_ctx *ctx);
/* Device properties the host side sizes launches with. */
int jdsp_device_info(jdsp_ctx *ctx, int *n_cu, size_t *hbm_bytes, char *name, size_t name_len);

/* Device memory helpers for callers without their own allocator. */
int jdsp_malloc(jdsp_ctx *ctx, size_t bytes, void **dev_ptr);
int jdsp_free(jdsp_ctx *ctx, void *dev_ptr);
int jdsp_memcpy_h2d(jdsp_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
int jdsp_memcpy_d2h(jdsp_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);
/* Page-locked host memory.  Host-pointer entry points given PINNED buffers (these, or any
 * hipHostMalloc/hipHostRegister memory) overlap the PCIe copies with the kernels: jdsp_stft_i16
 * then streams the batch through in chunks on three HIP streams (copy in | transform | copy out). */
int jdsp_host_alloc(jdsp_ctx *ctx, size_t bytes, void **host_ptr);
int jdsp_host_free(jdsp_ctx *ctx, void *host_ptr);

/* ---- FFTAlgorithm_ver2.cpp -------------------------------------------------- */
/* Bitrev table (FFTAlgorithm_ver2.cpp:186-202), computed on the device with the
 * reference's 16-bit shift/or loop; bit count from block_len (:188), mask with
 * n_fft-1 (:202).  table_host: n_fft int16.  Bit-exact. */
int jdsp_bitrev_table(jdsp_ctx *ctx, int n_fft, int block_len, int16_t *table_host);
/* Batched FFTProcess (FFTAlgorithm_ver2.cpp:94-149): `batch` independent
 * n_fft-point complex transforms, interleaved double (COMPLEX, :20-22) in and
 * out, forward != 0 -> exp(-j..), unnormalised both ways.  Host pointers. */
int jdsp_fft_process_f64(jdsp_ctx *ctx, const double *in_host, double *out_host,
                         int n_fft, long batch, int forward);
int jdsp_fft_process_f64_dev(jdsp_ctx *ctx, const double *in_dev, double *out_dev,
                             int n_fft, long batch, int forward);

/* DFTProcess (FFTAlgorithm_ver2.cpp:162-173), IDFTProcess (:175-184) and IFFTProcess (:151-160): the
 * reference's definition-level O(N^2) transforms, evaluated on the device as the reference writes them
 * (angle ((2*PI)*i)*k/N with its PI 3.14159265358, terms added in i order, nothing fused) and, like the
 * reference, ACCUMULATED into the output the caller passes in (a caller that wants the plain transform
 * zeroes it first, as the reference's commented-out call sites :74,:76 would have to).  Any n >= 1 --
 * these are not restricted to powers of two.  `batch` independent transforms of length n, back to back.
 * in: int16[n] per transform for JDSP_DFT_I16, interleaved double (COMPLEX) otherwise. */
enum { JDSP_DFT_I16 = 0, JDSP_IDFT = 1, JDSP_IDFT_OVER_N = 2 };
int jdsp_dft_direct_f64_dev(jdsp_ctx *ctx, int kind, const void *in_dev, double *inout_dev, int n, long batch);
int jdsp_dft_direct_f64(jdsp_ctx *ctx, int kind, const void *in_host, double *inout_host, int n, long batch);

/* ---- STFT analysis: framing + Hamming + forward transform -------------------- */
/* Replaces, for n_frames frames at once, SpectralSubtraction_final.cpp:218-230
 * (== WienerFilter_final.cpp:181-193, noise path SS:168-180): frame f =
 * pcm[hop*f .. hop*f+n_fft) * (0.54-0.46cos(2*3.141592*i/(n_fft-1))) -> unnormalised
 * forward DFT, all n_fft bins.  pcm must hold hop*(n_frames-1)+n_fft samples.
 * Supported: n_fft = 1024 with hop = 512 (reference-native, the headline configuration: pcm
 * 16-byte aligned takes the fast kernel), n_fft = 1024 with any hop >= 1, and n_fft = 512 with
 * any hop (BASELINE config 3 as written; computed as the even bins of the zero-padded
 * 1024-point transform). */
int jdsp_stft_i16_dev(jdsp_ctx *ctx, const int16_t *pcm_dev, long n_frames,
                      int n_fft, int hop, jdsp_c32 *spec_dev);
/* Half-spectrum variant (n_fft 1024, hop 512, Hamming): bins 0..512 only, row f at
 * spec_dev + f * row_pitch complex64 (row_pitch >= 513; 513 = dense rows of 4,104 B instead of
 * 8,192).  The reference keeps all 1024 bins, so this is an extra, measured separately
 * (5,128 algorithmic bytes per frame). */
int jdsp_stft_half_i16_dev(jdsp_ctx *ctx, const int16_t *pcm_dev, long n_frames, jdsp_c32 *spec_dev, long row_pitch);
int jdsp_stft_i16(jdsp_ctx *ctx, const int16_t *pcm_host, long n_samples,
                  int n_fft, int hop, jdsp_c32 *spec_host, long *n_frames_out);
/* Half spectra of a batch of n_utts RAGGED utterances in one launch: the layout of jdsp_stftmask_batch_dev (below), so
 * the rows line up with its mask rows and with jdsp_istft_batch_dev's spectrum rows.  n_fft 1024; hop 1024, 512 or 256;
 * window by "stft.window".
 *   - Utterance u has F_u = frame_first[u + 1] - frame_first[u] frames (>= 0); its frame f is
 *     pcm[sample_first[u] + hop f .. + 1024) and goes to row frame_first[u] + f of `spec`, row_pitch complex64 apart,
 *     bins 0..512.
 *   - That row equals row f, bins 0..512, of jdsp_stft_i16_dev(pcm + sample_first[u], F_u, 1024, hop) on the utterance
 *     alone, BIT FOR BIT, wherever the utterance sits in the batch and for every "stft.frames_per_wave".
 *   - row_pitch must be EVEN and >= 514: every row then starts on a 16-byte boundary and takes the arithmetic of the
 *     full-spectrum entry.  (Dense rows of 513 remain jdsp_stft_half_i16_dev's layout: its odd rows factorise their
 *     twiddles differently and equal the full spectrum only to rounding.)  spec must be 16-byte, pcm 4-byte and the
 *     offset arrays 8-byte aligned; anything else, another hop, n_utts < 0 or n_frames_total < 0 is JDSP_EINVAL with a
 *     jdsp_last_error text, and nothing is launched.
 *   - Elements 513..row_pitch-1 of a row and rows >= n_frames_total are not written; no sample outside an utterance's
 *     span [sample_first[u], sample_first[u] + hop (F_u - 1) + 1024) is read.
 *   - jdsp_stft_half_batch_dev only enqueues on the context's stream and never reads the offset arrays on the host
 *     (int64, [n_utts] and [n_utts + 1]) -- hence n_frames_total, which must equal frame_first[n_utts].  The offsets
 *     are the caller's contract, the one of jdsp_stftmask_batch_dev: frame_first[0] = 0 and non-decreasing,
 *     sample_first even, the spans disjoint and inside pcm.
 *   - jdsp_stft_half_batch (host pointers, synchronous) checks all of that as jdsp_stftmask_batch does (pcm is
 *     n_samples long) and writes bins 0..512 of rows 0..frame_first[n_utts]-1 of spec_host.
 *   - n_utts == 0, n_frames_total == 0 and batches of empty utterances succeed and launch nothing. */
int jdsp_stft_half_batch_dev(jdsp_ctx *ctx, const int16_t *pcm_dev, const int64_t *sample_first_dev,
                             const int64_t *frame_first_dev, long n_utts, long n_frames_total, int hop,
                             jdsp_c32 *spec_dev, long row_pitch);
int jdsp_stft_half_batch(jdsp_ctx *ctx, const int16_t *pcm_host, long n_samples, const int64_t *sample_first_host,
                         const int64_t *frame_first_host, long n_utts, int hop, jdsp_c32 *spec_host,
                         long row_pitch);                                                /* host path, synchronous */
/* The same analysis in the reference's own precision (SS:218-230 computes in double): FP64 window, FP64 transform,
 * spec = n_frames x 1024 interleaved (re, im) doubles (16,384 B per frame).  n_fft = 1024, any hop >= 1.  Agrees with
 * the reference's FFTProcess on the same windowed frames to ~1e-11 of the frame peak (FFTProcess's truncated PI,
 * FFT:15); the FP32 entries above agree with this one to ~5e-7. */
int jdsp_stft_i16_f64_dev(jdsp_ctx *ctx, const int16_t *pcm_dev, long n_frames, int n_fft, int hop, double *spec_dev);
int jdsp_stft_i16_f64(jdsp_ctx *ctx, const int16_t *pcm_host, long n_samples, int n_fft, int hop, double *spec_host,
                      long *n_frames_out);

/* ---- STFT synthesis: inverse transform + overlap-add to PCM ---------------------- */
/* The step SpectralSubtraction_final.cpp:244-257 (= WienerFilter_final.cpp:215-228) performs -- unnormalised inverse
 * DFT, real part, 1/N, overlap-add with a shift of one hop, truncating (short) cast -- as a public, streaming, batched
 * entry for spectra the caller made (e.g. jdsp_stft_i16_dev's output with a mask applied in place).  A jdsp_istft
 * handle holds ONE output stream; frames are counted from the last reset; n = n_fft, R = n / hop.
 *   1. Spectrum of frame f: X_f = row f, row_pitch complex64 apart.
 *      JDSP_SPEC_FULL  n bins per row.  The frame is the REAL PART of the full complex inverse (as SS:244-251 takes
 *                      [i][0]), i.e. the inverse of H_f[k] = (X_f[k] + conj X_f[(n-k) mod n]) / 2: a non-Hermitian row
 *                      is handled exactly, not assumed away.
 *      JDSP_SPEC_HALF  bins 0..n/2 per row (jdsp_stft_half_i16_dev's layout), row_pitch >= n/2+1, taken as Hermitian:
 *                      H[n-k] = conj X[k]; the imaginary parts of bins 0 and n/2 are ignored.
 *   2. Frame signal: y_f[i] = w_s[i] * (1/n) * sum_k H_f[k] e^{+2 pi j i k / n}, i < n.  w_s = 1 for JDSP_WIN_NONE,
 *      else the Hamming / Hann of "stft.window": 0.54-0.46cos(2*3.141592*i/(n-1)) / 0.5-0.5cos(same).
 *   3. Overlap-add: s[t] = sum_f y_f[t - hop f], accumulated in FP32 in ascending frame order starting from 0 -- so the
 *      output does not depend on how the stream is cut into calls, or on the launch geometry, bit for bit.
 *   4. Emission: after frame f the samples t in [hop f, hop f + hop) are final and written as g[t mod hop] * s[t], with
 *      g = 1 when analysis_window == JDSP_WIN_NONE, else g[i] = 1 / sum_{r<R} w_a[i + r hop] w_s[i + r hop] (WOLA
 *      normalisation: jdsp_stft_i16_dev followed by this entry gives the input back).  create returns JDSP_EINVAL when
 *      an entry of that sum is below 1e-6 of its largest (e.g. Hann analysis at R = 1).
 *   5. Output: int16 = the oracle's cast_i16 of that float (truncate toward zero, keep the low 16 bits: values past
 *      +-32,768 wrap; beyond +-2^31 is out of scope), and optionally the float32 values themselves.  A call of F frames
 *      writes F*hop contiguous samples.  Both output pointers may be NULL: the stream then advances without writing
 *      (sharding primes a halo this way, see jeicyboodsp_amd/sharding.py).
 *   6. flush writes the n - hop samples still in the tail (same g, same cast), then resets the handle.
 * n = 1024, hop = 512, FULL, NONE, NONE is SS:244-257 exactly.
 * Accuracy of the float32 values, against steps 1-4 in FP64 (tests/test_istft_hard_gpu.py, on spectra of every kind):
 *   - every sample is within 1e-5 g[t mod hop] P of the exact one, P the largest |y_f[i]| of the stream;
 *   - every sample is within 1e-5 g[t mod hop] sum_f P_f |w_s[t - hop f]| of it, the sum over the frames that hold t
 *     and P_f frame f's largest sample before the synthesis window (step 2 with w_s = 1): a frame is held to its
 *     own size, not to a louder neighbour's, and a zero row or a purely anti-Hermitian FULL row adds exact zeros.
 * A NaN sample casts to int16 0.  A non-finite value in row f reaches only the samples of frame f's support, t in
 * [hop f, hop f + n): every other sample is what it is with that row zero, bit for bit, and the handle is clean again
 * after _reset or _flush (a live stream after _streams_reset / _streams_flush of its id, the others untouched).
 * Supported: n_fft 1024 or 512 with hop = n, n/2 or n/4.  Alignment: spec 8 bytes (a jdsp_c32), out_i16 4 bytes,
 * out_f32 8 bytes; anything else, or a row_pitch below the layout's bin count, is JDSP_EINVAL.  The _dev entries only
 * enqueue on the handle's stream (no allocation, no host synchronisation); the state is n_fft floats
 * twice (ping-pong) plus the window and gain tables, allocated at create.  jdsp_istft_process / _flush: host
 * pointers, synchronous (device buffers grown on demand in the handle).
 * Graph capture (Conventions): _process_dev and _flush_dev are class H -- WHICH of the two tails is current is host
 * state passed to the launch, so a captured call, or a captured run of consecutive calls, is graph-capturable ONCE, AT
 * THE STREAM POSITION IT WAS CAPTURED AT: replay it once, let nothing else touch the handle between capture and replay,
 * and capture again after _reset / _flush.  To replay one graph per delivery use the live-stream entries below with
 * n_streams = 1: the same stream, bit for bit, with its state on the device (class D).  _batch_dev is class S. */
typedef struct jdsp_istft jdsp_istft;
enum { JDSP_SPEC_FULL = 0, JDSP_SPEC_HALF = 1 };
enum { JDSP_WIN_NONE = -1, JDSP_WIN_HAMMING = 0, JDSP_WIN_HANN = 1 };   /* numbering of "stft.window" */
typedef struct { int n_fft, hop, layout, synthesis_window, analysis_window; } jdsp_istft_cfg;
int  jdsp_istft_create(jdsp_ctx *ctx, const jdsp_istft_cfg *cfg, jdsp_istft **out);
int  jdsp_istft_destroy(jdsp_istft *h);
int  jdsp_istft_reset(jdsp_istft *h);
/* "frames_per_wave": consecutive frames one wavefront walks (0 = auto: about one round of resident waves, at least
 * 4 (R - 1)); any value >= max(R - 1, 1) gives the same output bit for bit -- a tuning and testing knob. */
int  jdsp_istft_set_option(jdsp_istft *h, const char *name, long value);
long jdsp_istft_samples_out(const jdsp_istft *h, long n_frames);
int  jdsp_istft_process_dev(jdsp_istft *h, const jdsp_c32 *spec_dev, long row_pitch, long n_frames,
                            int16_t *out_i16_dev, float *out_f32_dev);
int  jdsp_istft_flush_dev(jdsp_istft *h, int16_t *out_i16_dev, float *out_f32_dev);
int  jdsp_istft_process(jdsp_istft *h, const jdsp_c32 *spec_host, long row_pitch, long n_frames,
                        int16_t *out_i16_host, float *out_f32_host);   /* host path, synchronous */
int  jdsp_istft_flush(jdsp_istft *h, int16_t *out_i16_host, float *out_f32_host);   /* host path, synchronous */
/* A batch of n_utts INDEPENDENT utterances in one launch, with the handle's configuration (every n_fft, hop, layout
 * and window combination create accepts), windows, gain and "frames_per_wave".  The layout is the one of
 * jdsp_stftmask_batch_dev (below), with spectrum rows where that has mask rows.  The two entries neither read nor
 * write the handle's carried tail, so they may be interleaved with _process / _flush of the handle's own stream.
 *   - Utterance u has F_u = frame_first[u + 1] - frame_first[u] frames (>= 0); its frame f is row frame_first[u] + f of
 *     `spec` (the rows of all utterances back to back, row_pitch complex64 apart).
 *   - Its result is what a fresh handle of the same configuration gives for _process of its F_u rows followed by
 *     _flush, bit for bit (int16 and float32, for every "frames_per_wave"): hop (F_u - 1) + n samples, written at
 *     out[sample_first[u] .. sample_first[u] + hop (F_u - 1) + n).  An utterance with F_u = 0 writes nothing, and the
 *     device entry touches no sample outside the spans.  Either output pointer may be NULL (both: nothing is done).
 *   - jdsp_istft_batch_dev only enqueues on the stream _process_dev uses: no allocation, no host synchronisation, no
 *     host read of the two offset arrays (int64, [n_utts] and [n_utts + 1], 8-byte aligned) -- hence n_frames_total,
 *     which must equal frame_first[n_utts].  The device-side offsets are the caller's contract: frame_first[0] = 0 and
 *     non-decreasing; every sample_first[u] even (for both frame sizes: one layout contract, although n = 512 would
 *     not need it); the spans inside the outputs, and disjoint.  No row >= n_frames_total is read.  row_pitch and the
 *     alignment of spec and the outputs are _process_dev's.
 *   - jdsp_istft_batch (host pointers, synchronous) checks all of that as jdsp_stftmask_batch does and returns
 *     JDSP_EINVAL with a jdsp_last_error text otherwise.  The outputs are n_samples long and ZERO outside the spans.
 *   - n_utts == 0, n_frames_total == 0 and batches of empty utterances succeed and launch nothing. */
int  jdsp_istft_batch_dev(jdsp_istft *h, const jdsp_c32 *spec_dev, long row_pitch, const int64_t *sample_first_dev,
                          const int64_t *frame_first_dev, long n_utts, long n_frames_total, int16_t *out_i16_dev,
                          float *out_f32_dev);
int  jdsp_istft_batch(jdsp_istft *h, const jdsp_c32 *spec_host, long row_pitch, const int64_t *sample_first_host,
                      const int64_t *frame_first_host, long n_utts, long n_samples, int16_t *out_i16_host,
                      float *out_f32_host);                                               /* host path, synchronous */
/* LIVE STREAMS on the synthesis handle: the six entries of jdsp_stftmask_streams_* (below, where the vocabulary and
 * the rules are written out) with spec_dev, row_pitch where those have pcm_dev, mask_dev, mask_pitch.  Chunk c of
 * stream stream_id[c] is the F_c spectrum rows frame_first[c] .. frame_first[c + 1] - 1; there is no PCM, so its span
 * is its hop F_c output samples, written at out[sample_first[c] .. + hop F_c).  Stream s's chunks in call order
 * followed by its _streams_flush equal a fresh handle's _process of all those rows, then _flush, bit for bit (int16
 * and float32, every "frames_per_wave", every order of chunks, every cut).  Every configuration create accepts. */
int  jdsp_istft_streams_reserve(jdsp_istft *h, long n_streams);
int  jdsp_istft_streams_reset_dev(jdsp_istft *h, const int64_t *stream_id_dev, long n_ids);        /* NULL: all */
int  jdsp_istft_streams_dev(jdsp_istft *h, const jdsp_c32 *spec_dev, long row_pitch, const int64_t *stream_id_dev,
                            const int64_t *sample_first_dev, const int64_t *frame_first_dev, long n_chunks,
                            long n_frames_total, int16_t *out_i16_dev, float *out_f32_dev);
int  jdsp_istft_streams_flush_dev(jdsp_istft *h, const int64_t *stream_id_dev, const int64_t *sample_first_dev,
                                  long n_ids, int16_t *out_i16_dev, float *out_f32_dev);
int  jdsp_istft_streams(jdsp_istft *h, const jdsp_c32 *spec_host, long row_pitch, const int64_t *stream_id_host,
                        const int64_t *sample_first_host, const int64_t *frame_first_host, long n_chunks,
                        long n_samples, int16_t *out_i16_host, float *out_f32_host);      /* host path, synchronous */
int  jdsp_istft_streams_flush(jdsp_istft *h, const int64_t *stream_id_host, const int64_t *sample_first_host,
                              long n_ids, long n_samples, int16_t *out_i16_host,
                              float *out_f32_host);                                       /* host path, synchronous */

/* ---- fused STFT masking: PCM -> analysis -> per-bin mask -> synthesis -> PCM ------- */
/* jdsp_stft_* followed by a multiplication of the spectrum and jdsp_istft_*, as ONE pass in which the spectrum never
 * reaches memory: a time-frequency mask from an enhancer or separator, a fixed spectral equaliser, a noise gate.
 * A jdsp_stftmask handle holds ONE output stream, like jdsp_istft; n = n_fft, R = n / hop.  The semantics are the
 * composition of entries above:
 *   1. Frame f of a call = pcm[hop f .. hop f + n) * w_a.  w_a, w_s: the numbering of JDSP_WIN_* (JDSP_WIN_NONE =
 *      rectangular; Hamming / Hann by the formulas of "stft.window").  pcm must hold hop (n_frames - 1) + n samples,
 *      as jdsp_stft_i16_dev requires: the caller presents the overlap again at a call cut -- the handle keeps no PCM,
 *      only the overlap-add tail.
 *   2. X_f = the unnormalised forward DFT of the frame, bins 0..n/2.
 *   3. Y_f[k] = M_f[k] X_f[k], k = 0..n/2.  M_f = row f of `mask`, mask_pitch ELEMENTS apart: float for
 *      JDSP_MASK_REAL, jdsp_c32 for JDSP_MASK_COMPLEX.  mask_pitch >= n/2 + 1, or 0: one row for every frame of the
 *      call (a fixed equaliser; the kernel keeps it in registers).
 *   4. Synthesis of Y is jdsp_istft's with JDSP_SPEC_HALF: Hermitian by construction (the imaginary parts of bins 0
 *      and n/2 -- so those of M[0], M[n/2] -- are ignored), 1/n, times w_s, overlap-add in FP32 in ascending frame
 *      order starting from 0, emission g[t mod hop] * s[t] with g = 1 when normalise == 0, else
 *      g[i] = 1 / sum_{r<R} w_a[i + r hop] w_s[i + r hop] (create returns JDSP_EINVAL when an entry of that sum is
 *      below 1e-6 of its largest: jdsp_istft_create's rule), the oracle's cast_i16.  Either output pointer may be
 *      NULL; with both NULL the stream advances without writing (a shard primes its halo this way,
 *      jeicyboodsp_amd/sharding.py).  A call of F frames writes F * hop contiguous samples.
 *   5. flush writes the n - hop samples still in the tail (same g, same cast), then resets the handle.
 * The output does not depend on how the stream is cut into calls or on the launch geometry, bit for bit.
 * Accuracy, of the float32 output against steps 1-5 in FP64, every sample: |err| <= 1e-5 P g[t mod hop], P the largest
 * |s| of the stream before the gain, and also |err| <= 1e-5 g[t mod hop] times the largest |s| over the hop-blocks
 * within R - 1 of the sample's own (the blocks covered by the frames that touch it) -- a loud stretch elsewhere in
 * the stream excuses nothing.  The second holds under masks that remove something loud and keep something faint too
 * (a notch on a hum, a separator's mask for a talker 80 dB under an interferer, |M| up to 1000): a frame whose FP32
 * transform rounding could show in its own output, rho = 2^-23 sqrt(E mean|M|^2 / sum y^2) > 8e-7 (E: the windowed
 * frame's energy, y: the frame before w_s), is computed again in FP64 inside the same launch, bit-identically
 * wherever the frame falls.  White input under a mask of order one has rho = 1.2e-7 and is never recomputed.
 * n_fft 1024, hop 512, JDSP_WIN_HAMMING, JDSP_WIN_NONE, normalise 0 with a mask of ones is SS:218-257 at a zero noise
 * estimate.
 * Supported: n_fft = 1024 with hop 1024, 512 or 256; both mask kinds.  (n_fft = 512 is JDSP_EINVAL: DESIGN.md 7.)
 * Alignment: pcm and out_i16 4 bytes, out_f32 8 bytes, a REAL mask 4 bytes, a COMPLEX mask 8 bytes; anything else, a
 * mask_pitch in 1..n/2 or n_frames < 0 is JDSP_EINVAL with a jdsp_last_error text.  The _dev entries only enqueue on
 * the handle's stream (no allocation, no host synchronisation); the state -- two tails (ping-pong),
 * the windows and the gain, the FP64 pass's tables and count -- is allocated at create.  jdsp_stftmask_process / _flush: host pointers, synchronous
 * (device buffers grown on demand in the handle).
 * Graph capture (Conventions): _process_dev and _flush_dev are class H, as on jdsp_istft -- graph-capturable ONCE, AT THE
 * STREAM POSITION THEY WERE CAPTURED AT: one replay, nothing else on the handle between capture and replay, capture
 * again after _reset / _flush.  A caller that replays one graph per delivery uses jdsp_stftmask_streams_dev with
 * n_streams = 1 (class D): the same stream, bit for bit.  _batch_dev is class S. */
typedef struct jdsp_stftmask jdsp_stftmask;
enum { JDSP_MASK_REAL = 0, JDSP_MASK_COMPLEX = 1 };
typedef struct { int n_fft, hop, analysis_window, synthesis_window, normalise, mask_kind; } jdsp_stftmask_cfg;
int  jdsp_stftmask_create(jdsp_ctx *ctx, const jdsp_stftmask_cfg *cfg, jdsp_stftmask **out);
int  jdsp_stftmask_destroy(jdsp_stftmask *h);
int  jdsp_stftmask_reset(jdsp_stftmask *h);
/* "frames_per_wave": consecutive frames one wavefront walks (0 = auto: about one round of resident waves, at least
 * 4 (R - 1)); values below max(R - 1, 1) are raised to it.  Every value gives the same output bit for bit. */
int  jdsp_stftmask_set_option(jdsp_stftmask *h, const char *name, long value);
long jdsp_stftmask_samples_out(const jdsp_stftmask *h, long n_frames);
/* Frames of the last _process / _batch call (host or device entry) that were computed again in FP64; 0 before any call
 * and after reset.  Waits for the handle's stream.  (The call number is a scalar baked at capture: a captured _dev call
 * replayed from a graph back to back counts under the one number it was captured with, and the figure is then the sum
 * over those replays; a call in between under the next number zeroes it.) */
long jdsp_stftmask_frames_recomputed(const jdsp_stftmask *h);
int  jdsp_stftmask_process_dev(jdsp_stftmask *h, const int16_t *pcm_dev, const void *mask_dev, long mask_pitch,
                               long n_frames, int16_t *out_i16_dev, float *out_f32_dev);
int  jdsp_stftmask_flush_dev(jdsp_stftmask *h, int16_t *out_i16_dev, float *out_f32_dev);
int  jdsp_stftmask_process(jdsp_stftmask *h, const int16_t *pcm_host, const void *mask_host, long mask_pitch,
                           long n_frames, int16_t *out_i16_host, float *out_f32_host);   /* host path, synchronous */
int  jdsp_stftmask_flush(jdsp_stftmask *h, int16_t *out_i16_host, float *out_f32_host);  /* host path, synchronous */
/* A batch of n_utts INDEPENDENT utterances in one launch, with the handle's configuration, windows and gain.  The
 * two entries neither read nor write the handle's carried tail, so they may be interleaved with _process / _flush of
 * the handle's own stream.
 *   - Utterance u has F_u = frame_first[u + 1] - frame_first[u] frames (>= 0).  Its frame f is
 *     pcm[sample_first[u] + hop f .. + n); its mask row is row frame_first[u] + f of `mask` (the rows of all
 *     utterances back to back, mask_pitch elements apart; mask_pitch 0: ONE row for every frame of every utterance).
 *   - Its result is what a fresh handle of the same configuration gives for _process of its F_u frames followed by
 *     _flush, bit for bit (int16 and float32, for every "frames_per_wave"): hop (F_u - 1) + n samples, the length of
 *     its PCM span, written at the SAME offset: out[sample_first[u] .. sample_first[u] + hop (F_u - 1) + n).  An
 *     utterance with F_u = 0 writes nothing, and the device entry touches no sample outside the spans.  Either
 *     output pointer may be NULL (both: nothing is done).
 *   - jdsp_stftmask_batch_dev only enqueues on the context's stream: no allocation, no host synchronisation, no host
 *     read of the two offset arrays (int64, [n_utts] and [n_utts + 1], 8-byte aligned) -- hence n_frames_total, which
 *     must equal frame_first[n_utts].  The device-side offsets are the caller's contract, as utt_first_dev is for
 *     jdsp_gmm_score_dev: frame_first[0] = 0 and non-decreasing; every sample_first[u] even (every access stays 4- or
 *     8-byte aligned); the spans inside pcm and the outputs, and disjoint.  No PCM outside an utterance's span and no
 *     mask row >= n_frames_total is read.
 *   - jdsp_stftmask_batch (host pointers, synchronous) checks all of that and returns JDSP_EINVAL with a
 *     jdsp_last_error text otherwise: frame_first[0] == 0, frame_first non-decreasing, sample_first even, >= 0 and
 *     ascending with sample_first[u] + span_u <= sample_first[u + 1], the last span <= n_samples.  pcm and the
 *     outputs are n_samples long; the outputs are ZERO outside the spans.
 *   - n_utts == 0, n_frames_total == 0 and batches of empty utterances succeed and launch nothing.  n_utts < 0, a
 *     mask_pitch in 1..n/2 and misaligned base pointers are JDSP_EINVAL, as in jdsp_stftmask_process_dev. */
int  jdsp_stftmask_batch_dev(jdsp_stftmask *h, const int16_t *pcm_dev, const void *mask_dev, long mask_pitch,
                             const int64_t *sample_first_dev, const int64_t *frame_first_dev, long n_utts,
                             long n_frames_total, int16_t *out_i16_dev, float *out_f32_dev);
int  jdsp_stftmask_batch(jdsp_stftmask *h, const int16_t *pcm_host, long n_samples, const void *mask_host,
                         long mask_pitch, const int64_t *sample_first_host, const int64_t *frame_first_host,
                         long n_utts, int16_t *out_i16_host, float *out_f32_host);        /* host path, synchronous */
/* LIVE STREAMS: n_streams independent output streams in the handle, next to its own one, whose overlap-add tails are
 * carried from call to call; one call advances any subset of them by a ragged number of frames each, in ONE transform
 * launch (plus one O(n_chunks) bookkeeping launch).  A CHUNK is what one live stream contributes to one call: chunk c
 * has its stream stream_id[c], F_c = frame_first[c + 1] - frame_first[c] frames (>= 0) and its first sample
 * sample_first[c].  The concatenated frame axis, the mask rows and the two offset arrays are those of
 * jdsp_stftmask_batch_dev with chunks where that has utterances; stream_id (int64, [n_chunks], 8-byte aligned) is new.
 *   - _streams_reserve is the only call that allocates, and it synchronises: the handle gets n_streams >= 1 live
 *     streams, all fresh; calling it again discards every live stream's state.  Before it the other five entries
 *     return JDSP_EINVAL with a text.  The state is the tail, n - hop floats per stream, held twice with one word per
 *     stream that says which copy is current: within a launch the waves that read a stream's carried tail and the
 *     wave that writes its new one never touch the same memory, and the word lives on the device.
 *   - _streams_dev, inputs of chunk c: frame f is pcm[sample_first[c] + hop f .. + n), its mask row is row
 *     frame_first[c] + f (mask_pitch 0: one row for everything).  As on _process_dev the caller presents the overlap
 *     again -- the handle keeps no PCM: the chunk's PCM span is hop (F_c - 1) + n samples and begins with the last
 *     n - hop samples of the stream's previous chunk.
 *   - _streams_dev, output of chunk c: hop F_c samples at out[sample_first[c] .. + hop F_c), the first hop F_c samples
 *     of its own PCM span, so one set of offsets serves input and output.  The remaining n - hop samples of the span
 *     are not written; nothing outside the spans is written or read.
 *   - Equivalence: the outputs of stream s's chunks in call order, followed by its _streams_flush, equal what a fresh
 *     single-stream handle of the same configuration gives for _process of all those frames, then _flush -- bit for
 *     bit, in int16 and float32, for every "frames_per_wave", every order of chunks within a call and every way the
 *     frames are cut into chunks and calls.  A stream with no chunk in a call, or with a chunk of 0 frames, keeps its
 *     state untouched.  jdsp_stftmask_frames_recomputed reports a _streams call like any other.
 *   - The handle's own stream (_process / _flush) and the stateless _batch entries are neither read nor written by any
 *     of this and may be interleaved with it on the same handle.
 *   - The caller's contract on the device: stream ids in [0, n_streams) and distinct within a call; n_chunks <=
 *     n_streams (a scalar: checked by the device entry too); frame_first[0] = 0, non-decreasing, frame_first[n_chunks]
 *     = n_frames_total; sample_first even; the spans disjoint and inside the buffers.  The host entries check all of
 *     it (sample_first ascending, as jdsp_stftmask_batch) and return JDSP_EINVAL with a jdsp_last_error text, every
 *     stream left as it was.  Alignments are those of the batch entries.  n_chunks == 0, n_frames_total == 0 and both
 *     outputs NULL behave as in the batch entries: they launch nothing and change no state.
 *   - _streams_flush_dev writes, for each of the n_ids listed streams, the n - hop tail samples at
 *     out[sample_first[i] .. + n - hop), g[t mod hop] * s[t] with the same cast, and then resets those streams (with
 *     both outputs NULL it only resets them).  _streams_reset_dev zeroes the listed streams, or all when stream_id_dev
 *     is NULL (n_ids is then ignored).  Ids are distinct and in range, as above.
 *   - Every _dev entry only enqueues on the stream _process_dev uses: no allocation, no host synchronisation, no host
 *     read of the arrays, and nothing baked into a launch that would make a replayed capture wrong.  They are
 *     graph-capturable, class D (Conventions): n_chunks / n_ids, n_frames_total, the pitches and the pointers are baked;
 *     stream_id, sample_first, frame_first and the buffers are read at replay; EVERY REPLAY ADVANCES the streams it
 *     names then from where they stand then, so one captured delivery (or a captured run of deliveries, flushes and
 *     resets) serves every later one of the same n_chunks and n_frames_total.  With n_streams = 1 this is the
 *     replayable form of the handle's own _process_dev / _flush_dev stream, which is class H.
 *   - jdsp_stftmask_streams / _streams_flush: host pointers, synchronous, check everything; pcm and the outputs are
 *     n_samples long and the outputs ZERO outside the written ranges.  For the flush the spans are the n - hop
 *     samples at each sample_first[i] (even, ascending, disjoint, inside n_samples). */
int  jdsp_stftmask_streams_reserve(jdsp_stftmask *h, long n_streams);
int  jdsp_stftmask_streams_reset_dev(jdsp_stftmask *h, const int64_t *stream_id_dev, long n_ids);  /* NULL: all */
int  jdsp_stftmask_streams_dev(jdsp_stftmask *h, const int16_t *pcm_dev, const void *mask_dev, long mask_pitch,
                               const int64_t *stream_id_dev, const int64_t *sample_first_dev,
                               const int64_t *frame_first_dev, long n_chunks, long n_frames_total,
                               int16_t *out_i16_dev, float *out_f32_dev);
int  jdsp_stftmask_streams_flush_dev(jdsp_stftmask *h, const int64_t *stream_id_dev, const int64_t *sample_first_dev,
                                     long n_ids, int16_t *out_i16_dev, float *out_f32_dev);
int  jdsp_stftmask_streams(jdsp_stftmask *h, const int16_t *pcm_host, long n_samples, const void *mask_host,
                           long mask_pitch, const int64_t *stream_id_host, const int64_t *sample_first_host,
                           const int64_t *frame_first_host, long n_chunks, int16_t *out_i16_host,
                           float *out_f32_host);                                          /* host path, synchronous */
int  jdsp_stftmask_streams_flush(jdsp_stftmask *h, const int64_t *stream_id_host, const int64_t *sample_first_host,
                                 long n_ids, long n_samples, int16_t *out_i16_host,
                                 float *out_f32_host);                                    /* host path, synchronous */

/* ---- spectral subtraction / Wiener filter ------------------------------------- */
/* One jdsp_denoise object holds everything the reference keeps in static locals
 * for one audio stream: main()'s run-length counter and noise estimate
 * (SpectralSubtraction_final.cpp:70-72), EstimateNoiseSpectrum's running
 * average (:161), the keep buffers (:164,:208), the overlap buffer (:209) and
 * the call counters (:202).  Feeding a stream in batches of any size -- down to
 * the reference's one 512-sample block per call -- yields the same output.
 *
 * jdsp_denoise_process* replaces, for n_blocks blocks, one iteration each of
 * main()'s loop: VoiceActivityDetection (SS:121-156 / WF:261-296),
 * EstimateNoiseSpectrum (SS:159-198 / WF:120-159) and SpectralSubtraction
 * (SS:201-264) or WienerFiltering (WF:162-235).  Like the reference, the first
 * two blocks of a stream produce no output (SS:260-263): *n_out_blocks =
 * jdsp_denoise_blocks_out().  out gets n_out blocks of 512 int16; precast (may
 * be NULL) gets the same samples before the (short) cast, as float. */
enum { JDSP_SPECSUB = 0, JDSP_WIENER = 1 };
typedef struct jdsp_denoise jdsp_denoise;
int jdsp_denoise_create(jdsp_ctx *ctx, int mode, jdsp_denoise **out);
/* The same object with the reference's macros as parameters: FFT_PROCESSING_SIZE = n_fft, BLOCK_LEN =
 * KEEP_LEN = hop (SS:53-55 / WF:42-44 are 1024 / 512 / 512 = jdsp_denoise_create; BASELINE config 3 words the workload
 * "512-pt STFT 50 % hop" = (512, 256)).  Blocks are then hop samples long everywhere below, the noise estimate has
 * n_fft entries, and the thresholds stay the reference's (energy 700, ZCR 200, latch at run length 10).  Supported:
 * (1024, 512) and (512, 256), on every entry below (batched, per-block jdsp_denoise_apply, sharded). */
int jdsp_denoise_create_cfg(jdsp_ctx *ctx, int mode, int n_fft, int hop, jdsp_denoise **out);
int jdsp_denoise_block_len(const jdsp_denoise *h);
int jdsp_denoise_destroy(jdsp_denoise *h);
int jdsp_denoise_reset(jdsp_denoise *h);                       /* back to a fresh stream */
/* "blocks_per_wave": the number of consecutive blocks one wave of the run kernel walks, on the stream entries and the
 * batch entries alike: 1 / 2 / 4 / 8, or 0 (default) for one round of resident waves over the call's blocks.  A tuning
 * knob only: the output bits do not depend on it ((1024, 512) handles; (512, 256) handles accept and ignore it).
 * "vad_trace": 1 keeps every block's energy sum and zero-crossing count for
 * jdsp_denoise_vad_trace (a slower VAD kernel: two exact wave reductions per block); 0 (default) keeps the flags only. */
int jdsp_denoise_set_option(jdsp_denoise *h, const char *name, long value);
long jdsp_denoise_blocks_out(const jdsp_denoise *h, long n_blocks);
/* Sizes the device workspace for batches of up to max_blocks (the only call
 * that allocates; process() calls it on demand). */
int jdsp_denoise_reserve(jdsp_denoise *h, long max_blocks);
int jdsp_denoise_process_dev(jdsp_denoise *h, const int16_t *pcm_dev, long n_blocks, int16_t *out_dev,
                             float *precast_dev, long *n_out_blocks);
int jdsp_denoise_process(jdsp_denoise *h, const int16_t *pcm_host, long n_blocks, int16_t *out_host,
                         float *precast_host, long *n_out_blocks);
/* Current rgdEstimatedNS (n_fft doubles, host).  Synchronises. */
int jdsp_denoise_noise(jdsp_denoise *h, double *noise_host);
/* How many frames of the last call (process, apply, shard_finish or batch) the FP32 kernels handed to the FP64 pass: in
 * spectral subtraction because transform rounding could show through the phase of bins far below the noise estimate
 * (exactly periodic input), and at 512-point frames, in both modes, because a quiet frame shares its transform with a
 * loud one.  1024-point Wiener: always 0.  Negative: an error code.
 * Synchronises. */
long jdsp_denoise_frames_recomputed(jdsp_denoise *h);
/* VoiceActivityDetection results of the first n blocks of the last process call:
 * voice flag, sum of squared truncated samples (dEnergy*1024, SS:135) and dZCR (SS:140).
 * Any pointer may be NULL.  The flags are always there; energies and counts only when the "vad_trace" option was
 * set WHEN THAT CALL RAN (JDSP_EINVAL otherwise -- since ABI version 2; setting it afterwards does not make a
 * trace appear).  Synchronises. */
int jdsp_denoise_vad_trace(jdsp_denoise *h, long n, uint8_t *voice_host, int64_t *energy_sum_host,
                           int32_t *zcr_host);

/* Batched denoise: n_utts INDEPENDENT utterances in one launch sequence, each a fresh stream of the reference's
 * main() with the handle's mode.  The entries neither read nor write the handle's own stream state (run length,
 * average, estimate, previous block, overlap, call count), so they may be interleaved with _process on the same
 * handle; jdsp_denoise_frames_recomputed reports the batch call's count when it was the last call.  (1024, 512)
 * handles only: on a (512, 256) handle the three entries return JDSP_EINVAL with a text (two 512-point frames share
 * one transform, and the pairing across utterance boundaries is not built).
 *   - Utterance u has B_u = block_first[u + 1] - block_first[u] blocks (>= 0) of hop = jdsp_denoise_block_len(h)
 *     samples; its block b is pcm[sample_first[u] + hop b .. + hop).
 *   - Its result is what a fresh handle of the same mode gives for _process of its B_u blocks: max(B_u - 2, 0) emitted
 *     blocks.  Emitted block k is the overlap buffer's first half after the frame [block k + 1, block k + 2] was added
 *     (SS:247-263: the call that consumes block k + 2 is the stream's call k + 3, the first that returns TRUE for
 *     k = 0), i.e. the enhanced signal at the time of input block k + 1, and it is written TIME-ALIGNED, at
 *     out[sample_first[u] + hop (k + 1) .. + hop); precast (the same samples before the (short) cast) likewise.  Indices
 *     computed for the noisy PCM (MFCC frame_start, ...) therefore apply to the output unchanged.  The first and the
 *     last block of each span are never written, and the device entry touches no sample outside the spans.
 *   - flags [n_blocks_total] uint8: the VAD decision of every block, in concatenated block order (block b of
 *     utterance u at block_first[u] + b).  noise_last [n_utts][1024] float32: the estimate in force after the
 *     utterance's last block, zeros if none was latched.  Any of the four output pointers may be NULL.
 *   - An utterance's out, precast, flags and noise_last do not depend, bit for bit, on where it stands in the batch,
 *     on its neighbours, on how the batch is split into calls, or on the "blocks_per_wave" option.  Against the oracle
 *     they are held to _process's bars; against _process itself they agree to those bars, not bit for bit (the single
 *     stream sums its noise average in chunks).
 *   - jdsp_denoise_batch_dev only enqueues on the context's stream: no allocation, no host synchronisation, no host
 *     read of the two offset arrays (int64, [n_utts] and [n_utts + 1], 8-byte aligned) -- hence n_blocks_total, which
 *     must equal block_first[n_utts].  It is graph-capturable, class S (Conventions): n_utts and n_blocks_total are
 *     baked, the two offset arrays and the PCM are read at every replay, and a replay equals an eager call on the same
 *     contents bit for bit, as often as it is replayed.  The device-side offsets are the caller's contract, the
 *     one of jdsp_stftmask_batch_dev: block_first[0] = 0 and non-decreasing; every sample_first[u] even, >= 0 and
 *     ascending; the spans, hop B_u long, disjoint and inside pcm and the outputs.  No PCM outside the spans is read.
 *     pcm and out 16-byte, precast 8-byte aligned, as in jdsp_denoise_process_dev.
 *   - Its workspace comes from jdsp_denoise_batch_reserve, the only call that allocates (and synchronises): per
 *     reserved block 1 (flag) + 4 (row index) + 4 (FP64 list) + 409.6 bytes (latched rows: an utterance of B blocks
 *     latches at most floor(B / 10) times, so 1 + floor(max_blocks_total / 10) rows of 4 KB hold any batch) = 419
 *     bytes; nothing per utterance.  A _dev call with more blocks or utterances than reserved is JDSP_EINVAL with a
 *     text.
 *   - jdsp_denoise_batch (host pointers, synchronous) reserves on demand, checks the offsets and returns JDSP_EINVAL
 *     with a jdsp_last_error text otherwise: block_first[0] == 0, block_first non-decreasing, sample_first even, >= 0
 *     and ascending with sample_first[u] + hop B_u <= sample_first[u + 1], the last span <= n_samples.  pcm, out and
 *     precast are n_samples long; the outputs are ZERO wherever the device entry would not write.
 *   - n_utts == 0, batches of empty utterances and all four outputs NULL succeed and launch nothing; so does a host
 *     batch in which every B_u <= 2, except for the VAD when flags are asked for (the device entry cannot know: its
 *     kernels then write nothing but flags and zero estimates).  n_utts < 0 and misaligned base pointers are
 *     JDSP_EINVAL. */
int jdsp_denoise_batch_reserve(jdsp_denoise *h, long max_blocks_total, long max_utts);
int jdsp_denoise_batch_dev(jdsp_denoise *h, const int16_t *pcm_dev, const int64_t *sample_first_dev,
                           const int64_t *block_first_dev, long n_utts, long n_blocks_total, int16_t *out_dev,
                           float *precast_dev, uint8_t *flags_dev, float *noise_last_dev);
int jdsp_denoise_batch(jdsp_denoise *h, const int16_t *pcm_host, long n_samples, const int64_t *sample_first_host,
                       const int64_t *block_first_host, long n_utts, int16_t *out_host, float *precast_host,
                       uint8_t *flags_host, float *noise_last_host);                   /* host path, synchronous */

/* LIVE STREAMS on the denoise handle: n_streams independent streams of the reference's main() in the handle, next to
 * its own one, whose statics (run length, running average, latched estimate, call counter, previous blocks, overlap)
 * live ON THE DEVICE and are carried from call to call.  One call advances any subset of them by a chunk of blocks each,
 * in one launch sequence.  The handle's own _process stream and the _batch entries are neither read nor written, and may
 * be interleaved with these entries on the same handle.  (1024, 512) handles only: on a (512, 256) handle every entry
 * here returns JDSP_EINVAL with a text, as the batch entries do.  (Vocabulary: jdsp_stftmask_streams_*, above.)
 *   - A CHUNK is what one stream contributes to one call.  Chunk c belongs to stream stream_id[c] and holds B_c =
 *     block_first[c + 1] - block_first[c] NEW blocks (>= 0) of hop = 512 samples at pcm[sample_first[c] .. + hop B_c):
 *     jdsp_denoise_batch_dev's layout with chunks for utterances, plus stream_id.  The handle keeps the history it needs.
 *   - EMISSION FOLLOWS THE STREAM.  A stream's block with index i (0-based, counted over all its calls) emits iff
 *     i >= 2 (SS:260-263); the emitted block is the enhanced signal at the time of input block i - 1, as in _process.
 *     For a stream that had seen N blocks the chunk emits E_c = B_c - max(0, min(B_c, 2 - N)) blocks, written PACKED at
 *     out[sample_first[c] + hop e .. + hop), e < E_c; precast likewise.  The other hop (B_c - E_c) samples of the span
 *     and everything outside the spans are neither written nor read.  There is NO FLUSH: the reference never emits a
 *     stream's overlap at its end; a reset ends a stream.
 *   - EQUIVALENCE, BIT FOR BIT: the emitted blocks of a stream, concatenated over its calls, are what
 *     jdsp_denoise_batch writes for ONE utterance of all those blocks (batch output block k + 1 = emission k), on out,
 *     precast, the VAD flags and the estimate in force (noise_last) -- however the blocks are cut into chunks and
 *     calls, in whatever order the chunks stand, for every "blocks_per_wave" and both modes, frames that go through the
 *     FP64 pass included.  A stream with no chunk in a call, or with a chunk of 0 blocks, is not touched.
 *   - jdsp_denoise_streams_reserve(h, n_streams, max_blocks_total) is the only call that allocates, and it synchronises.
 *     All streams start fresh; calling it again discards every stream.  Before it the other entries return JDSP_EINVAL
 *     with a text.  Per stream 18,972 bytes of state: the last two blocks (2,048) and the overlap (2,048), each held
 *     twice so that no launch reads memory it writes, the estimate twice (8,192), the running average (2,560) and
 *     28 bytes of words.  Per call a workspace for max_blocks_total blocks: per block 1 (flag) + 4 (row index) + 4 (FP64
 *     list) bytes, per stream 8 (a chunk's latch flag and list entry), and n_streams + max_blocks_total / 11 + 2 latched
 *     rows of 4 KB.  A call beyond it is JDSP_EINVAL.
 *   - jdsp_denoise_streams_dev and jdsp_denoise_streams_reset_dev only enqueue on the stream jdsp_denoise_batch_dev
 *     uses: no allocation, no host synchronisation, no host read of the arrays.  Graph-capturable, class D
 *     (Conventions): n_chunks / n_ids, n_blocks_total and the pointers are baked; ids, offsets and buffers are read at
 *     replay, and every replay advances the named streams from where they stand.  The caller's contract on the device:
 *     ids in [0, n_streams) and distinct within a call; n_chunks <= n_streams (checked); block_first[0] = 0,
 *     non-decreasing, block_first[n_chunks] = n_blocks_total; sample_first even; the spans disjoint and inside the
 *     buffers; pcm and out 16-byte, precast, n_emitted and the int64 arrays 8-byte aligned.
 *   - flags [n_blocks_total] uint8 in concatenated block order; n_emitted [n_chunks] int64 = E_c.  Any output pointer
 *     may be NULL.  With out and precast both NULL the state still advances exactly as with them (the VAD, the noise
 *     estimate, the blocks and the overlap; nothing is emitted).  n_chunks == 0 or n_blocks_total == 0 launches nothing
 *     and changes nothing.  reset_dev: the n_ids listed streams fresh again; stream_id_dev NULL: all of them.
 *   - jdsp_denoise_streams (host pointers, synchronous) checks all of that, with sample_first ascending as in
 *     jdsp_denoise_batch, and on a violation returns JDSP_EINVAL with a jdsp_last_error text and leaves every stream as
 *     it was.  pcm, out and precast are n_samples long; the outputs are ZERO wherever the device entry would not write.
 *   - jdsp_denoise_frames_recomputed reports a _streams call like any other.  A listed frame whose second output block
 *     arrives with the stream's next call is computed in FP64 again there, and counts in both calls.
 *   - jdsp_denoise_streams_state: [n_ids][1024] float32 estimates in force, in the layout of the batch entry's
 *     noise_last (zeros: nothing has latched), and the blocks each stream has seen.  Synchronises; either may be NULL. */
int jdsp_denoise_streams_reserve(jdsp_denoise *h, long n_streams, long max_blocks_total);
int jdsp_denoise_streams_reset_dev(jdsp_denoise *h, const int64_t *stream_id_dev, long n_ids);   /* NULL: all */
int jdsp_denoise_streams_dev(jdsp_denoise *h, const int16_t *pcm_dev, const int64_t *stream_id_dev,
                             const int64_t *sample_first_dev, const int64_t *block_first_dev, long n_chunks,
                             long n_blocks_total, int16_t *out_dev, float *precast_dev, uint8_t *flags_dev,
                             int64_t *n_emitted_dev);
int jdsp_denoise_streams(jdsp_denoise *h, const int16_t *pcm_host, long n_samples, const int64_t *stream_id_host,
                         const int64_t *sample_first_host, const int64_t *block_first_host, long n_chunks,
                         int16_t *out_host, float *precast_host, uint8_t *flags_host, int64_t *n_emitted_host);
int jdsp_denoise_streams_state(jdsp_denoise *h, const int64_t *stream_id_host, long n_ids, float *noise_host,
                               int64_t *blocks_seen_host);      /* synchronises; either output may be NULL */

/* Sharded denoise: one rank's share of ONE global stream of n_total blocks (multi-GPU,
 * SURVEY §8e).  The rank owns global blocks [b0, b1); pcm_ext_dev holds global blocks
 * [ext0, b1) with ext0 = max(b0 - 2, 0) (two halo blocks rebuild the overlap tail); blocks are
 * jdsp_denoise_block_len() samples (512, or 256 on 512-point frames: the exchanged buffers keep
 * their 1025-float size, entries past n_fft are unused).  Between
 * the steps the caller all-gathers three small buffers across ranks (any transport; RCCL in
 * jeicyboodsp_amd/sharding.py):
 *   1. shard_vad      -> flags_own (b1-b0 bytes)          all-gather -> flags_all (n_total bytes)
 *   2. shard_summary  -> summary (1025 floats: the affine map A <- a*A + b of this rank's
 *                         noise frames, SS:182-187)        all-gather -> summaries_all (world*1025)
 *   3. shard_rows     -> last (1025 floats: latch count and last latched estimate, SS:189-193)
 *                                                          all-gather -> last_all (world*1025)
 *   4. shard_finish   -> out: the emitted blocks among [max(b0,2), b1), shard_blocks_out() of them
 * Concatenating the ranks' outputs gives the single-GPU stream (int16 within +-1 LSB). */
int jdsp_denoise_shard_vad_dev(jdsp_denoise *h, const int16_t *pcm_ext_dev, long ext0, long b0, long b1, long n_total,
                               uint8_t *flags_own_dev);
int jdsp_denoise_shard_summary_dev(jdsp_denoise *h, const uint8_t *flags_all_dev, float *summary_dev);
int jdsp_denoise_shard_rows_dev(jdsp_denoise *h, const float *summaries_all_dev, int world, int rank, float *last_dev);
long jdsp_denoise_shard_blocks_out(const jdsp_denoise *h);
int jdsp_denoise_shard_finish_dev(jdsp_denoise *h, const float *last_all_dev, int world, int rank, int16_t *out_dev,
                                  float *precast_dev, long *n_out_blocks);

/* The reference's two helper functions on their own, for callers that keep main()'s
 * structure (jeicyboodsp_amd/compat): */
/* VoiceActivityDetection (SS:121-156) for n_blocks blocks of 512 host samples; outputs as
 * jdsp_denoise_vad_trace.  Any output pointer may be NULL. */
int jdsp_vad_blocks(jdsp_ctx *ctx, const int16_t *pcm_host, long n_blocks, uint8_t *voice_host,
                    int64_t *energy_sum_host, int32_t *zcr_host);
/* The same function at the other shapes it exists in.  variant JDSP_VAD_DENOISE: SS:121-156 = WF:261-296, frame
 * [zeros(block_len), block], voice <=> energy > 700 or ZCR < 200.  JDSP_VAD_MVDR: BeamForming_MVDR_ver1.cpp:207-242,
 * frame [zeros(block_len - 1), block, 0] (KEEP_LEN 511, :37), voice <=> energy > 700 (:233; the zero-crossing count
 * is still computed and returned, as the reference prints it).  block_len 512 (the reference's BLOCK_LEN) or 256
 * (FFT_PROCESSING_SIZE 512: BASELINE configs 3 and 5 as worded).  energy_sum = the integer sum of squares; the
 * reference's dEnergy is energy_sum / (2 block_len). */
#define JDSP_VAD_DENOISE 0
#define JDSP_VAD_MVDR 1
int jdsp_vad_blocks_ex(jdsp_ctx *ctx, int variant, int block_len, const int16_t *pcm_host, long n_blocks,
                       uint8_t *voice_host, int64_t *energy_sum_host, int32_t *zcr_host);
/* SpectralSubtraction / WienerFiltering (SS:201-264 / WF:162-235) with the CALLER's
 * pdEstimatedNoiseSpec (n_fft doubles, host) instead of the handle's own VAD + estimate: only
 * the keep buffer, the overlap buffer and the call counter of the handle are used. */
int jdsp_denoise_apply(jdsp_denoise *h, const int16_t *pcm_host, long n_blocks, const double *noise_host,
                       int16_t *out_host, float *precast_host, long *n_out_blocks);

/* ---- overlap-save fast convolution --------------------------------------------- */
/* Fast_Convolution_Based_3DAudio_Impl.cpp.  jdsp_fastconv_create replaces main()'s filter
 * set-up (:82-84) and the per-block FFT of the filter (:140,:143): taps is n_filters rows of
 * n_taps doubles (the reference: one row, rgdFirLPF_coefficients[7169] of FilterCoefficient.h);
 * n_fft is 8192 (reference-native) or 1024; block = n_fft - n_taps + 1 samples per call
 * (1024 native).  jdsp_fastconv_process* replaces AnalySisFreqDomain (:102-177) for n_blocks
 * blocks: like the reference, the first hist_blocks = ceil((n_taps-1)/block) blocks of a
 * stream produce no output (:119-123) and never reach the transform (the reference queues
 * uninitialised buffers for them, :120 -- defined as silence here).  out: n_filters planes of
 * n_out*block int16, plane-major; precast (may be NULL): the same values before the (short)
 * cast.  The handle carries the samples its next call reaches back to (the last n_taps-1; the
 * partitioned form: the last 512 ceil(n_taps/512)), so consecutive calls on one handle give the
 * same bits, int16 and pre-cast, however the stream is cut into them, through either entry (not
 * after jdsp_fastconv_set_position: see there).
 * Alignment of pcm_dev, out_dev and precast_dev: natural alignment (2, 2 and 4 bytes).  The
 * partitioned form stores two int16 as one dword and two pre-cast floats as one 8-byte store
 * at whatever address that gives: at an odd sample / float offset these are unaligned stores,
 * which the device takes as they are (global memory runs in unaligned-access mode under ROCm). */
typedef struct jdsp_fastconv jdsp_fastconv;
int jdsp_fastconv_create(jdsp_ctx *ctx, const double *taps, int n_taps, int n_filters, int n_fft,
                         jdsp_fastconv **out);
int jdsp_fastconv_destroy(jdsp_fastconv *h);
int jdsp_fastconv_reset(jdsp_fastconv *h);
/* Multi-GPU / random access: pretend `blocks_consumed` blocks of the stream have already been
 * processed (history = silence).  A rank that owns output blocks [e0, e1) of a stream feeds
 * input blocks [e0 + hist_blocks - hist_blocks', ...): see sharding.fastconv_sharded -- it
 * prepends hist_blocks halo blocks and drops the outputs they produce.  The partitioned form's
 * oldest frame reaches 512 ceil(n_taps/512) samples back, up to 512 more than the halo holds;
 * they weigh nothing in the sum but are in the frame the transform rounds, so a position set
 * this way equals the uncut stream within the 1e-5 bar, not bit for bit. */
int jdsp_fastconv_set_position(jdsp_fastconv *h, long blocks_consumed);
int jdsp_fastconv_block_len(const jdsp_fastconv *h);
int jdsp_fastconv_hist_blocks(const jdsp_fastconv *h);
long jdsp_fastconv_blocks_out(const jdsp_fastconv *h, long n_blocks);
/* Sizes the workspace for calls of up to n_blocks blocks ahead of time (the 8192-point configuration with a
 * block length that is a multiple of 512 runs as a partitioned convolution with a spectrum workspace). */
int jdsp_fastconv_reserve(jdsp_fastconv *h, long n_blocks);
int jdsp_fastconv_process_dev(jdsp_fastconv *h, const int16_t *pcm_dev, long n_blocks, int16_t *out_dev,
                              float *precast_dev, long *n_out_blocks);
int jdsp_fastconv_process(jdsp_fastconv *h, const int16_t *pcm_host, long n_blocks, int16_t *out_host,
                          float *precast_host, long *n_out_blocks);

/* ---- batched reverberation: ragged utterances, each with its own room response ------------- */
/* NOT a reference function: the reference convolves one stream with one fixed filter set (jdsp_fastconv_* above).  This
 * is the same uniformly partitioned overlap-save as jdsp_fastconv's 8192-point path, as the stateless batch entry the
 * other chains have: thousands of ragged utterances in one launch sequence, each convolved with its own long impulse
 * response out of a bank, at its own gain.  Its oracle is the FP64 direct convolution of tests/reverb_ref.py.
 *   - THE BANK.  taps: n_irs responses x n_taps real taps (double, host), 1 <= n_taps <= 7680, 1 <= n_irs <= 16384;
 *     anything else is JDSP_EINVAL with a text.  A response is cut into P = ceil(n_taps / 512) partitions of 512 taps
 *     (jdsp_reverb_n_part, 1 <= P <= 15); each, zero-padded to 1024 points, is transformed once in FP64 on the device
 *     as jdsp_fastconv_create does and kept as an FP32 row of the bins 0..512 at a pitch of 520: 4,160 P bytes per
 *     response, 62,400 at P = 15.  Blocks are 512 samples (jdsp_reverb_block_len).
 *   - THE LAYOUT is jdsp_denoise_batch_dev's: utterance u has B_u = block_first[u + 1] - block_first[u] >= 0 blocks of
 *     512 samples at pcm[sample_first[u]]; sample_first even; the spans disjoint, ascending and inside the buffers;
 *     block_first[0] = 0, non-decreasing, block_first[n_utts] = n_blocks_total.  ir[u] (int32, in [0, n_irs)) names the
 *     utterance's response and gain[u] (float32) its gain; gain NULL: every gain 1, bit for bit the same as an array
 *     of 1.0f.
 *   - SEMANTICS, in exact arithmetic, for 0 <= t < 512 B_u:  y_u[t] = gain[u] sum_k h[ir[u]][k] x_u[t - k],  x_u silent
 *     before the utterance's first sample.  The output is as long as the input, time-aligned, and written at the same
 *     offsets: out[sample_first[u] + t].  THE TAIL IS NOT APPENDED: a caller who wants the reverberation that rings on
 *     after the utterance's last sample appends P blocks of zeros to the utterance.  Nothing outside the spans is read
 *     or written; the analysis of an utterance's first block uses 512 zeros in front of it, not what precedes the
 *     span in pcm.
 *   - OUTPUT.  out_f32: the float value; out_i16: its (short) cast (truncate toward zero, keep the low 16 bits, as
 *     every chain here).  Either may be NULL; with both NULL nothing is done.
 *   - THE ARITHMETIC, fixed (csrc/reverb_kernels.hip): one 1024-point FP32 forward transform per block, of [previous
 *     block | block], rectangular window, bins 0..512 to a workspace row; output block c of an utterance is the second
 *     half of the inverse transform of sum_{p = 0}^{min(c, P - 1)} X[c - p] H_p, accumulated in FP32 with p ascending --
 *     an order that depends on c and P alone, not on where the wave, the workgroup or the utterance stands; rows in
 *     front of the utterance's first contribute nothing; the inverse's 1/1024 and the gain are ONE FP32 multiply per
 *     sample, by gain[u] * 2^-10 (itself one FP32 product).
 *   - GUARANTEES (tests/test_reverb_batch_gpu.py, bars: tests/reverb_cases.py).  (1) per utterance, with w the FP64
 *     value, x the samples, g the gain and h the response: every float sample within 1e-5 max(max|w|, 0.05 max|x| |g|
 *     sum|h|), and every sample of output block e within 1e-5 max(max|w| over the blocks e - 1 .. e + 1, 0.05 |g| sum|h|
 *     max|x| over the 512 (P + 1) input samples that end with block e, silence before the utterance) -- the bars the
 *     partitioned jdsp_fastconv path holds with the same arithmetic.  Where a bar is 0 the output is exact zeros
 *     (silence, gain 0).  The int16 IS the cast of the float, also past +-32768 (the low 16 bits), and within +-1 of
 *     the cast of the FP64 value modulo 65536.  (2) INDEPENDENCE: an utterance's bytes, in both outputs, do not depend
 *     on its place in the batch or in pcm, on the other utterances, their responses or gains, on the order of the
 *     utterances, or on how the batch is split into calls.
 *   - jdsp_reverb_batch_dev only enqueues on the context's stream (a plan launch of one workgroup, the analysis, the
 *     multiply-accumulate / inverse): no allocation, no host synchronisation, no host read of any array; every grid
 *     comes from the scalars n_utts and n_blocks_total, which must equal block_first[n_utts].  Graph-capturable, class
 *     S (Conventions): the scalars and the pointers are baked; pcm, the offsets, ir and gain are read at replay.  The
 *     caller's contract on the device is the layout above; pcm and out_i16 16-byte, out_f32 and the offset arrays
 *     8-byte, ir and gain 4-byte aligned (checked).  ir values are clamped into [0, n_irs) on the device instead of
 *     reading outside the bank.  n_utts == 0, n_blocks_total == 0 and batches of empty utterances succeed and launch
 *     nothing.
 *   - Its workspace comes from jdsp_reverb_batch_reserve, the only call that allocates (and synchronises): 4,160
 *     bytes per reserved block (the spectrum rows) and 8 (n_utts + 1) bytes of plan (the workgroups per utterance,
 *     prefixed).  It only grows.  A non-empty batch before it, or one larger than the reservation in blocks or
 *     utterances, is JDSP_EINVAL with a text.
 *   - jdsp_reverb_batch (host pointers, synchronous; pcm and the outputs are n_samples long) reserves on demand,
 *     checks the offsets as jdsp_denoise_batch does, and ir in range and the gains finite; a violation is JDSP_EINVAL
 *     with a jdsp_last_error text.  Its outputs are ZERO outside the spans. */
typedef struct jdsp_reverb jdsp_reverb;
int jdsp_reverb_create(jdsp_ctx *ctx, const double *taps /* [n_irs][n_taps] */, int n_irs, int n_taps, jdsp_reverb **out);
int jdsp_reverb_destroy(jdsp_reverb *h);
int jdsp_reverb_n_irs(const jdsp_reverb *h);
int jdsp_reverb_n_part(const jdsp_reverb *h);
int jdsp_reverb_block_len(const jdsp_reverb *h);   /* 512 */
int jdsp_reverb_batch_reserve(jdsp_reverb *h, long n_blocks, long n_utts);
int jdsp_reverb_batch_dev(jdsp_reverb *h, const int16_t *pcm_dev, const int64_t *sample_first_dev,
                          const int64_t *block_first_dev, const int32_t *ir_dev, const float *gain_dev /* may be NULL: 1 */,
                          long n_utts, long n_blocks_total, int16_t *out_i16_dev, float *out_f32_dev);
int jdsp_reverb_batch(jdsp_reverb *h, const int16_t *pcm_host, long n_samples, const int64_t *sample_first_host,
                      const int64_t *block_first_host, const int32_t *ir_host, const float *gain_host, long n_utts,
                      int16_t *out_i16_host, float *out_f32_host);

/* ---- live reverberation streams: carried spectra, a response per chunk -------------------------- */
/* NOT a reference function: jdsp_reverb_batch's arithmetic with the history kept in the handle, for callers with
 * thousands of open streams that each deliver a few blocks per tick, each in its own room.  The vocabulary is
 * jdsp_mvdrn_streams_*'s, the layout and the arithmetic are jdsp_reverb_batch_dev's.  P = jdsp_reverb_n_part(h).
 *   - A CHUNK is what one stream contributes to one call: chunk c belongs to stream stream_id[c] and holds B_c =
 *     block_first[c + 1] - block_first[c] >= 0 NEW blocks of 512 samples at pcm[sample_first[c]], with the response
 *     ir[c] and the gain gain[c] (NULL: every gain 1) for its blocks.  The handle keeps the history: the caller never
 *     presents a block twice.  Offsets and alignment as in jdsp_reverb_batch_dev (sample_first even; spans disjoint,
 *     ascending, inside the buffers; block_first[0] = 0, non-decreasing, block_first[n_chunks] = n_blocks_total).
 *   - SEMANTICS, in exact arithmetic: with x_s the concatenation of every block stream s has been given since its
 *     reserve or reset, and the chunk's blocks the stream blocks i0 .. i0 + B_c - 1, for t inside those blocks
 *     y[t] = gain[c] sum_k h[ir[c]][k] x_s[t - k], silence before the stream's first sample.  Every block is written,
 *     at its own place out[sample_first[c] + 512 b ..]; nothing outside the spans is read or written.  The outputs must
 *     not overlap pcm: the last launch of a call reads pcm again.  A stream delivered with one response and gain
 *     throughout is the batch's utterance of all its blocks.  A change of ir or gain between chunks is a HARD SWITCH at
 *     the chunk boundary: the new response is applied to the whole carried history.  Cross-fading is not built, nor a
 *     flush that rings the tail out: the caller delivers P blocks of zeros.
 *   - THE ARITHMETIC is the batch's, for stream block i: one forward transform of [block i - 1 | block i];
 *     sum_{p = 0}^{min(i, P - 1)} X[i - p] H_p, p ascending, in one FP32 accumulator chain; the walk ends at the
 *     stream's block 0, so the stream counts its blocks; one multiply by gain[c] 2^-10.
 *   - CUT INDEPENDENCE, BIT FOR BIT (tests/test_reverb_streams_gpu.py).  A stream's int16 and float bytes do not depend
 *     on how its blocks are cut into chunks and calls (one block per call included), on the order of chunks in a call,
 *     the stream id or n_streams, on the other streams or the gaps between spans.  For a stream with one (ir, gain)
 *     throughout they EQUAL THE BYTES jdsp_reverb_batch writes for one utterance of all its blocks; for any chunk, that
 *     batch's output for the utterance "all blocks so far" with the chunk's (ir, gain), sliced to the chunk -- a block is
 *     a function of i, P, the samples, the response and the gain alone.  The batch's bars and int16 rules hold as there.
 *   - A stream with no chunk in a call, or with a chunk of 0 blocks, is not touched.  With both outputs NULL the STATE
 *     ADVANCES exactly as with them (the batch entry does nothing then).  n_chunks == 0 or n_blocks_total == 0 launches
 *     nothing.
 *   - STATE, per stream, each part held once: blocks_seen (8 bytes), the last block's 512 samples (1,024 bytes), and a
 *     ring of the last P - 1 SPECTRUM rows, the row of stream block i at slot i mod (P - 1): 4,160 (P - 1) bytes, none
 *     at P = 1 -- 59,272 bytes per stream at P = 15.  Carrying spectra, not PCM, is the point: no forward transform is
 *     ever repeated.  Per call: a workspace of one row (4,160 bytes) per block of max_blocks_total and a plan of
 *     8 (n_streams + 1) bytes.
 *   - jdsp_reverb_streams_reserve(h, n_streams, max_blocks_total) is the only call that allocates, and it synchronises;
 *     1 <= n_streams < 2^30, 0 <= max_blocks_total <= 2^30 - 16.  All streams start fresh; calling it again discards
 *     them.  Before it the other entries return JDSP_EINVAL with a text.  The batch workspace and the live workspace
 *     are kept apart: jdsp_reverb_batch_dev and jdsp_reverb_streams_dev may be interleaved on one handle.
 *   - jdsp_reverb_streams_dev and jdsp_reverb_streams_reset_dev only enqueue on the context's stream: no allocation, no
 *     host synchronisation, no host read of any array; every grid comes from the scalars alone.  The launches of a
 *     delivery, whatever n_chunks, one linear chain with no parallel branches: the analysis of the new blocks into the
 *     workspace (in front of a chunk's first block stand the stream's carried samples, zeros for a fresh stream); a plan
 *     of one workgroup (waves per chunk, prefixed) and the multiply-accumulate / inverse, in which a WAVE owns two
 *     consecutive blocks of one chunk, walks the rows from the newest down (this chunk's from the workspace, older ones
 *     from the ring) and reads H straight from the bank -- no response in LDS, no workgroup barrier, workgroups of 4
 *     waves; both skipped when both outputs are NULL; and the commit, which copies the chunk's last min(B_c, P - 1) rows
 *     into the ring and its last 512 samples into the state and adds B_c to blocks_seen.  The commit is a launch of its
 *     own because the launches before it read exactly what it writes: stream order makes a delivery race-free with
 *     nothing held twice.  Graph-capturable, class D (Conventions): n_chunks / n_ids, n_blocks_total and the pointers are
 *     baked; ids, offsets, ir, gain and pcm are read at replay; every replay advances the named streams.  Checked on the
 *     host: n_chunks <= n_streams, n_blocks_total <= the reservation, the alignment (as the batch entry's; stream_id
 *     8-byte).  The caller's contract on the device: ids in [0, n_streams) and distinct within a call, the offsets as in
 *     the batch; ir is clamped into [0, n_irs) on the device.  jdsp_reverb_streams_reset_dev: the listed streams fresh
 *     (NULL: all of them).
 *   - LONG CHUNKS.  A chunk of hundreds of blocks works, but every wave reads H again from L2 and no speed is promised
 *     for it: recordings belong to jdsp_reverb_batch.
 *   - jdsp_reverb_streams (host pointers, synchronous; pcm and the outputs are n_samples long) checks all of that and
 *     also duplicate or out-of-range ids, ir out of range, non-finite gains and overlapping spans; on a violation it
 *     returns JDSP_EINVAL with a jdsp_last_error text and LEAVES EVERY STREAM AS IT WAS.  Its outputs are ZERO outside
 *     the spans.
 *   - jdsp_reverb_streams_state: blocks_seen and the last block's samples (zeros for a fresh stream) of the listed
 *     streams; it synchronises; either pointer may be NULL. */
int jdsp_reverb_streams_reserve(jdsp_reverb *h, long n_streams, long max_blocks_total);
int jdsp_reverb_streams_reset_dev(jdsp_reverb *h, const int64_t *stream_id_dev, long n_ids);      /* NULL: all */
int jdsp_reverb_streams_dev(jdsp_reverb *h, const int16_t *pcm_dev, const int64_t *stream_id_dev,
                            const int64_t *sample_first_dev, const int64_t *block_first_dev,
                            const int32_t *ir_dev, const float *gain_dev /* may be NULL: 1 */,
                            long n_chunks, long n_blocks_total, int16_t *out_i16_dev, float *out_f32_dev);
int jdsp_reverb_streams(jdsp_reverb *h, const int16_t *pcm_host, long n_samples, const int64_t *stream_id_host,
                        const int64_t *sample_first_host, const int64_t *block_first_host,
                        const int32_t *ir_host, const float *gain_host, long n_chunks,
                        int16_t *out_i16_host, float *out_f32_host);                              /* synchronous */
int jdsp_reverb_streams_state(jdsp_reverb *h, const int64_t *stream_id_host, long n_ids,
                              int64_t *blocks_seen_host, int16_t *last_block_host /* [n_ids][512] */);

/* ---- binaural rendering: live sources mixed per ear in the spectrum ------------------------- */
/* NOT a reference function: the reference convolves one mono stream with one fixed filter set
 * (Fast_Convolution_Based_3DAudio_Impl.cpp:102-177, jdsp_fastconv_* above).  This is the same overlap-save algorithm
 * in the form a spatialiser serves: many short deliveries at once, each output a MIX of a handful of sources, each
 * source heard from its own direction out of a bank of HRIRs at its own gain, both changing while the stream runs.
 * Its oracle is the FP64 restatement in tests/binaural_ref.py.
 *   - THE BANK.  hrir_taps: n_dirs directions x 2 ears x n_taps real taps (double, host), 1 <= n_taps <= 513,
 *     1 <= n_dirs <= 16384.  Transforms are 1024-point and blocks are 512 samples (jdsp_binaural_block_len; what the
 *     denoisers emit): the last 512 samples of a segment [previous block | block] are alias-free for up to 513 taps.
 *     The spectra are computed once, in FP64 on the device as jdsp_fastconv_create does, and kept as FP32 with the
 *     transform's 1/1024 and the split's 1/2 folded in (powers of two: exact) -- of every spectrum only the 640 values
 *     that are not implied by its Hermitian symmetry in the kernel's pair scheme: 10 KB per direction.
 *   - THE STREAMS.  jdsp_binaural_streams_reserve(h, n_streams) opens n_streams LIVE STREAMS, each ONE SOURCE AS HEARD
 *     IN ONE MIX (a talker heard by four listeners is four streams whose chunks point at the same PCM).  A stream
 *     carries its last 512 input samples, the direction and the gain of its last delivery, and a "started" word:
 *     1,036 bytes, held twice under a device-side parity word (a mix's first block reads what its last block
 *     replaces) = 2,076 bytes per stream.  It is the only call that allocates, and it synchronises; all streams
 *     start fresh, and calling it again discards every stream.  Before it the other stream entries (_reset_dev,
 *     _render_dev, _render, _streams_state) return JDSP_EINVAL with a text.
 *   - ONE CALL (a delivery) renders n_mixes mixes.  Mix m produces B_m = block_first[m + 1] - block_first[m] >= 0
 *     output blocks from the chunks c in [chunk_first[m], chunk_first[m + 1]) -- possibly none: B_m blocks of zeros.
 *     Chunk c belongs to stream stream_id[c]; its new samples are pcm[sample_first[c] .. + 512 B_m) -- no overlap is
 *     presented, the handle keeps the history -- heard from dir[c] (int32, in [0, n_dirs)) at gain[c] (float32).
 *     Input spans are only read: they MAY COINCIDE OR OVERLAP (the one difference from the other entries' "disjoint
 *     spans"; it holds for inputs only).
 *   - SEMANTICS, in exact arithmetic, per ear e, block b and sample i of mix m: with x the stream (its carried history,
 *     then this chunk; silence before a fresh stream's first sample), y_{d,g}[t] = g sum_k h[d][e][k] x[t - k], and
 *     (d0, g0) the carried direction and gain ((d0, g0) = (d1, g1) for a fresh stream), chunk c contributes
 *         y_{d1,g1}                                   to blocks b >= 1, and to block 0 when (d0, g0) == (d1, g1)
 *                                                     (gains compared as bit patterns);
 *         (1 - r[i]) y_{d0,g0} + r[i] y_{d1,g1},  r[i] = i / 512,   to block 0 otherwise:
 *     a move or a gain step is a one-block linear cross-fade, and a constant source costs nothing extra.  The mix is
 *     the sum over its chunks in list order.
 *   - OUTPUT.  out_i16[e plane + 512 (block_first[m] + b) + i] = (short) of the float (truncate toward zero, keep the
 *     low 16 bits, as every chain here); out_f32, same layout: the float itself.  Either may be NULL; with both NULL
 *     the streams still advance.  Nothing else of the planes is written.
 *   - STATE RULE.  After the call each delivered stream carries its chunk's last 512 samples and (d1, g1), started.
 *     Streams with no chunk, and the chunks of a mix with B_m = 0, are untouched.
 *   - THE ARITHMETIC, fixed (csrc/binaural_kernels.hip): per chunk one forward 1024-point real transform of the
 *     segment in FP32; THE GAIN multiplies the chunk's split spectrum in FP32, before the bank values; the products
 *     are accumulated per ear in list order; a block takes the PLAIN form -- one accumulated spectrum per ear, two
 *     inverse transforms -- exactly when none of its chunks fades, else the FADED form: two accumulated spectra per
 *     ear, "old" (d0, g0) and "new" (d1, g1), the unchanged chunks in both, four inverse transforms, and the ramp
 *     fma(r, new, (1 - r) old) in FP32 in the time domain.  Which form a block takes depends only on the carried and
 *     delivered (dir, gain) values.  S sources cost S + 2 transforms per block (S + 4 while something fades), not 3 S.
 *   - GUARANTEES (tests/test_binaural_gpu.py; (1) on hard streams: tests/test_binaural_streams_gpu.py).  (1) every float
 *     sample of an output block within 1e-5 sum_c max(P_c, 0.05 S_c) of the FP64 value: P_c the largest magnitude of
 *     chunk c's contribution to either ear over the block, and S_c = (the largest |sample| of the chunk's 1024-sample
 *     segment, silence before a fresh stream) x max(|g1| max_e sum_k |h[d1][e][k]|, and while the chunk fades
 *     |g0| max_e sum_k |h[d0][e][k]|), which bounds every sample of the segment's circular convolution.  0.05 S_c is
 *     the scale the FP32 round-off of a segment lives on where the kept samples themselves are (nearly) zero -- a quiet
 *     block behind a loud one under a one-tap filter, DC into taps that sum to 0, the silence behind a click; there no
 *     FP32 transform holds 1e-5 sum_c P_c, elsewhere the P_c terms are the larger and the bar is that one (the
 *     convolver's floor, tests/fastconv_cases.py, per chunk).  Where the bar is 0 the block is exact zeros.  An ear
 *     whose taps are all zero in every direction the mix hears is exact zeros.  The int16 IS the cast of the float,
 *     also where the float lies past +-32768 (the low 16 bits), and within +-1 of the cast of the FP64 value modulo
 *     65536.  Gains in the denormal range are outside the guarantee.  (2) CUTS: a delivery of B blocks with (d, g) equals, bit for bit
 *     in both outputs, any split of it into consecutive deliveries that each name the same (d, g), down to one block
 *     per call.  (3) INDEPENDENCE: a mix's bits do not depend on its place among the mixes, on the other mixes, on
 *     the order of mixes, on its streams' ids or on n_streams; they DO depend on the order of its own chunks.
 *     (4) a mix whose every chunk has gain 0.0f and carried gain 0.0f is exact zeros.
 *   - jdsp_binaural_render_dev and jdsp_binaural_streams_reset_dev only enqueue (the render launch and a commit
 *     launch of n_chunks threads that flips the parity of the delivered streams): no allocation, no host
 *     synchronisation, no host read of the arrays.  Graph-capturable, class D (Conventions): the scalars and the
 *     pointers are baked; every array, dir and gain included, is read at replay, and every replay advances the named
 *     streams from where they stand.  The caller's contract on the device: ids in [0, n_streams) and distinct within a
 *     call; n_chunks <= n_streams (checked); both *_first arrays start at 0 and do not decrease, chunk_first[n_mixes] =
 *     n_chunks, block_first[n_mixes] = n_blocks_total; sample_first even; plane even and >= 512 n_blocks_total
 *     (checked); the spans inside pcm; the int64 arrays 8-byte, pcm, out_i16, dir and gain 4-byte, out_f32 8-byte
 *     aligned (checked).  The device entry clamps dir and the ids into range instead of reading outside the bank.
 *     n_mixes == 0 or n_blocks_total == 0 launches nothing and changes nothing.  reset_dev: the n_ids listed streams
 *     fresh again; stream_id_dev NULL: all of them.
 *   - jdsp_binaural_render (host pointers, synchronous; pcm is n_samples long, the outputs 2 x plane) checks all of
 *     that and dir in range, finite gains, every span inside n_samples and the output blocks inside plane; on a
 *     violation it returns JDSP_EINVAL with a jdsp_last_error text and leaves every stream as it was.  Its outputs are
 *     ZERO outside the written blocks.
 *   - jdsp_binaural_streams_state: per listed stream its 512 carried samples, direction, gain and started word (any
 *     output may be NULL).  Synchronises. */
typedef struct jdsp_binaural jdsp_binaural;
int jdsp_binaural_create(jdsp_ctx *ctx, const double *hrir_taps /* [n_dirs][2][n_taps] */, int n_dirs, int n_taps,
                         jdsp_binaural **out);
int jdsp_binaural_destroy(jdsp_binaural *h);
int jdsp_binaural_n_dirs(const jdsp_binaural *h);
int jdsp_binaural_block_len(const jdsp_binaural *h);          /* 512 */
int jdsp_binaural_streams_reserve(jdsp_binaural *h, long n_streams);
int jdsp_binaural_streams_reset_dev(jdsp_binaural *h, const int64_t *stream_id_dev, long n_ids);   /* NULL: all */
int jdsp_binaural_render_dev(jdsp_binaural *h, const int16_t *pcm_dev, const int64_t *stream_id_dev,
                             const int64_t *sample_first_dev, const int32_t *dir_dev, const float *gain_dev,
                             const int64_t *chunk_first_dev, const int64_t *block_first_dev, long n_mixes, long n_chunks,
                             long n_blocks_total, int16_t *out_i16_dev, float *out_f32_dev, long plane);
int jdsp_binaural_render(jdsp_binaural *h, const int16_t *pcm_host, long n_samples, const int64_t *stream_id_host,
                         const int64_t *sample_first_host, const int32_t *dir_host, const float *gain_host,
                         const int64_t *chunk_first_host, const int64_t *block_first_host, long n_mixes, long n_chunks,
                         int16_t *out_i16_host, float *out_f32_host, long plane);
int jdsp_binaural_streams_state(jdsp_binaural *h, const int64_t *stream_id_host, long n_ids, int16_t *hist_host,
                                int32_t *dir_host, float *gain_host, int32_t *started_host);      /* synchronises */

/* ---- FFT autocorrelation pitch --------------------------------------------------- */
/* PitchEstimation_method1.cpp: CalcPitch (:69-116) for n_blocks blocks of 512 samples.
 * Frame b = [block b-1, block b] with no window; block -1 is prev_block (NULL: zeros, the
 * reference's initial keep buffer, :74).  arg[b] = the lag the reference prints as
 * "Estimation arg" (:109; pitch = 16000/arg), rmax[b] = the autocorrelation there;
 * autocorr (may be NULL) = r[0..511] per block (:95-97).  pcm must be 16-byte aligned.
 * AnalysisAdditiveWhiteGaussianNoise.cpp:98-133 (the analysis half of that program) is this same chain
 * without the arg-max: its dAutoCorrelation (:122-124) is the autocorr output here. */
int jdsp_pitch_autocorr_dev(jdsp_ctx *ctx, const int16_t *pcm_dev, long n_blocks, const int16_t *prev_block_dev,
                            int32_t *arg_dev, float *rmax_dev, float *autocorr_dev);
int jdsp_pitch_autocorr(jdsp_ctx *ctx, const int16_t *pcm_host, long n_blocks, const int16_t *prev_block_host,
                        int32_t *arg_host, float *rmax_host, float *autocorr_host);

/* ---- time-domain pitch: AMDF and autocorrelation (exact) -------------------------------- */
/* PitchEstimation_method2.cpp (JDSP_PITCH_AMDF) and PitchEstimation_method3.cpp (JDSP_PITCH_ACF): CalcPitch
 * (:69-101 of both) for n_blocks blocks of 512 samples.  Frame b = [block b-1, block b] with no window; block -1 is
 * prev_block (NULL: zeros, the reference's initial keep buffer, :71).
 *   curve[b][k] = dAutoCorrelation[k] (:79-84), k < 512: the sum over i < 1024-k of |x[i]-x[i+k]| (AMDF) or of
 *                 x[i]*x[i+k] (ACF), divided by (double)(1024-k).  The sums are integers below 2^53 that the
 *                 reference's double holds exactly, so they are computed exactly here and the one IEEE division
 *                 gives the reference's bits.
 *   value[b], arg[b] = dMin / dMax and iArg of the scan :87-95 (from lag 511 down to 101, `<=` for the AMDF, `>=`
 *                 for the ACF: among equal values the smallest lag wins); pitch = 16000/arg.  A silent frame gives
 *                 arg 101 and value 0.
 * Any of arg, value and curve may be NULL; without curve the lags below 101 are not computed.  pcm, prev_block and
 * curve must be 16-byte aligned.  n_blocks == 0 is a successful no-op; a method other than these two is JDSP_EINVAL.
 * Results are bit-exact and do not depend on how a stream is cut into calls (hand the last block over as prev_block). */
enum { JDSP_PITCH_AMDF = 2, JDSP_PITCH_ACF = 3 };          /* the reference's method numbers */
int jdsp_pitch_lag_dev(jdsp_ctx *ctx, int method, const int16_t *pcm_dev, long n_blocks, const int16_t *prev_block_dev,
                       int32_t *arg_dev, double *value_dev, double *curve_dev);
int jdsp_pitch_lag(jdsp_ctx *ctx, int method, const int16_t *pcm_host, long n_blocks, const int16_t *prev_block_host,
                   int32_t *arg_host, double *value_host, double *curve_host);

/* ---- LPC ---------------------------------------------------------------------------------- */
/* LPCEstimation.cpp: LPCEstimation (:87-137) for n_blocks blocks of block_len samples (256, the reference's
 * BLOCK_LEN, or 512), order p = 1 .. 16 (the reference's LPC_LEN is 12).  With N = 2 block_len, frame b =
 * [block b-1, block b] (block -1 = prev_block, NULL: zeros), all in FP64:
 *   y[i] = x[i] * (0.54 - 0.46 cos(2*3.141592*i/(N-1)))                                  (:104-106)
 *   autocorr[b][i] = (sum over j < N-i of y[j] y[j+i]) / (N-i), i <= p: p+1 doubles per block, may be NULL (:108-113)
 *   lpc[b] = T^-1 v with T[i][j] = r[|i-j|], v[i] = -r[i+1]: p doubles per block                    (:115-130)
 * The solve is Gaussian elimination with partial pivoting and a back substitution (the reference's Eigen inverse() is
 * a partial-pivot LU as well); its bits are not the reference's, its forward error is of the same size.  The order of
 * every sum is fixed per frame: a frame's output does not depend on the batch it arrives in.  A frame whose
 * elimination meets a zero or non-finite pivot -- the all-zero frame is one; the reference's result there is an
 * unspecified inf/NaN -- returns p quiet NaNs.  Every block gets a vector: the reference's "first call returns
 * FALSE" (:133-136) is the caller's business.  pcm and prev_block must be 16-byte aligned. */
int jdsp_lpc_dev(jdsp_ctx *ctx, const int16_t *pcm_dev, long n_blocks, int block_len, int order,
                 const int16_t *prev_block_dev, double *autocorr_dev, double *lpc_dev);
int jdsp_lpc(jdsp_ctx *ctx, const int16_t *pcm_host, long n_blocks, int block_len, int order,
             const int16_t *prev_block_host, double *autocorr_host, double *lpc_host);

/* ---- two-microphone MVDR beamformer ----------------------------------------------- */
/* BeamForming_MVDR_ver1.cpp.  One jdsp_mvdr object = the statics of one stereo stream
 * (rgdSpatialCorr :57, the run counter :59, the keep/temp buffers :56,:130-131, iNumOfCount
 * :137).  d_time is ProcessMVDR's dTime (:124; the reference's main() passes
 * (DISTANCE_OF_MIC/SPEED_OF_SOUND)*sin(0) = 0, :60,:121).  jdsp_mvdr_process* replaces, for
 * n_blocks blocks of 512 samples per channel, one iteration each of main()'s loop (:169-231):
 * VoiceActivityDetection on the left channel (:207-242), EstimateSpatialCorrMtx (:244-270) and
 * ProcessMVDR (:124-205).  The first block of a stream produces no output (:201-204); until the
 * correlation matrix is invertible the reference's samples are NaN, cast to 0 here.
 * jdsp_mvdr_corr: current rgdSpatialCorr, row-major (4 doubles, host; synchronises).
 * GUARANTEES, of _process*, _apply and the sharded run alike, against the reference's own arithmetic in FP64
 * (oracle/jdsp_oracle.c; tests/test_mvdr_gpu.py, and on hard scenes, delays and matrices tests/test_mvdr_hard_gpu.py):
 *   - precast: every finite sample within 1e-5 of the stream's own finite peak (the largest finite |sample| of the FP64
 *     value over the stream, at least 1), and finite exactly where the FP64 value is.
 *   - out: the (short) cast of precast, within 1 LSB of the cast of the FP64 value.  With d_time != 0 the reference's
 *     overwritten real part (:180-183) has gain above 1, so a full-scale stream leaves int16 before the cast (39,000 and
 *     more); the cast then keeps the low 16 bits of the value truncated to int32, here as in the reference built for
 *     x86-64, and the 1 LSB holds modulo 2^16.  (Where 1e-5 of the peak exceeds half an LSB -- a caller matrix close to
 *     singular under a delay has a peak in the millions -- the first bar is the one that holds.)
 *   - a singular matrix (before the first estimate; a channel that is exactly zero in every pause) gives the
 *     reference's non-finite samples: the non-finite value in precast, 0 in out.
 *   - rgdSpatialCorr: the diagonal is the exact integer sum of the estimation frames' energies (Parseval), within 1e-12
 *     of the reference's; the off-diagonal, rounding error of the reference's transforms (1e-17 of the diagonal), is
 *     exactly 0.
 *   - the output does not depend on how the stream is cut into calls or on host against device pointers, bit for bit
 *     (the matrix is a sum of integers, exact in FP64 in any grouping while it stays below 2^53; the weights are one
 *     FP64 closed form whether a call reads them from its table or computes them per block). */
typedef struct jdsp_mvdr jdsp_mvdr;
int jdsp_mvdr_create(jdsp_ctx *ctx, double d_time, jdsp_mvdr **out);
int jdsp_mvdr_destroy(jdsp_mvdr *h);
int jdsp_mvdr_reset(jdsp_mvdr *h);
long jdsp_mvdr_blocks_out(const jdsp_mvdr *h, long n_blocks);
int jdsp_mvdr_process_dev(jdsp_mvdr *h, const int16_t *left_dev, const int16_t *right_dev, long n_blocks,
                          int16_t *out_dev, float *precast_dev, long *n_out_blocks);
int jdsp_mvdr_process(jdsp_mvdr *h, const int16_t *left_host, const int16_t *right_host, long n_blocks,
                      int16_t *out_host, float *precast_host, long *n_out_blocks);
int jdsp_mvdr_corr(jdsp_mvdr *h, double *corr4_host);
/* The program's two helper functions on their own, for callers that keep main()'s structure -- or do not follow
 * it (jeicyboodsp_amd/compat: EstimateSpatialCorrMtx, ProcessMVDR with the reference's signatures):
 *   jdsp_mvdr_estimate_corr  EstimateSpatialCorrMtx (:244-270) for n_frames frames of 1024 samples per channel
 *                            ([previous block, block], rgsTempBufferL/R), every frame's contribution ADDED to the
 *                            caller's rgdSpatialCorr (4 doubles, row-major).  Touches no stream state.
 *   jdsp_mvdr_apply          ProcessMVDR (:124-205) for n_blocks blocks with the CALLER's rgdSpatialCorr instead of
 *                            the handle's own VAD + accumulation: only the two keep buffers (:130-131) and the call
 *                            counter (:137) of the handle are used and advanced. */
int jdsp_mvdr_estimate_corr(jdsp_mvdr *h, const int16_t *left_frames_host, const int16_t *right_frames_host, long n_frames,
                            double *corr4_inout_host);
int jdsp_mvdr_apply(jdsp_mvdr *h, const int16_t *left_host, const int16_t *right_host, long n_blocks,
                    const double *corr4_host, int16_t *out_host, float *precast_host, long *n_out_blocks);
/* Sharded MVDR (multi-GPU): the rank owns global blocks [b0, b1) of a stream of n_total
 * blocks; the ext buffers hold global blocks [ext0, b1), ext0 = max(b0 - 1, 0).  shard_vad ->
 * flags_own; all-gather -> flags_all; shard_summary -> sum4 (this rank's contribution to
 * rgdSpatialCorr); all-gather -> sums_all (world*4 doubles); shard_finish -> the emitted blocks
 * among [max(b0,1), b1).  rgdSpatialCorr is a running SUM (:263-268), so the matrix entering a
 * rank is the sum of the earlier ranks' contributions: the reduction SURVEY §8e asks for. */
int jdsp_mvdr_shard_vad_dev(jdsp_mvdr *h, const int16_t *left_ext_dev, const int16_t *right_ext_dev, long ext0, long b0,
                            long b1, long n_total, uint8_t *flags_own_dev);
int jdsp_mvdr_shard_summary_dev(jdsp_mvdr *h, const uint8_t *flags_all_dev, double *sum4_dev);
long jdsp_mvdr_shard_blocks_out(const jdsp_mvdr *h);
int jdsp_mvdr_shard_finish_dev(jdsp_mvdr *h, const double *sums_all_dev, int world, int rank, int16_t *out_dev,
                               float *precast_dev, long *n_out_blocks);

/* ---- MVDR generalised to n microphones, per-bin covariance (BASELINE config 5) ------------- */
/* NOT a reference function: the reference has 2 microphones and one real 2x2 matrix for all
 * bins (jdsp_mvdr above is that algorithm).  This keeps its framing, VAD, run counter and weight
 * formula and makes the correlation a Hermitian n_mics x n_mics matrix PER BIN, accumulated over
 * the same noise frames, R_k += X_k X_k^H / 1024; w_k = R_k^-1 c_k / (c_k^H R_k^-1 c_k) with
 * c_k[m] = exp(j 2 PI f_k delays_s[m]); y = Re IDFT(w^H X) over k = 0..1023 with the bins above 512 the mirrors of
 * those below (with a fractional delay w^H X is not real at k = 512; its imaginary part adds nothing to y).
 * loading >= 0 adds
 * loading * trace(R_k)/n_mics to the diagonal (with 0, R_k is singular until n_mics noise frames
 * have been seen, and the output is NaN -> 0 like the reference's before its first estimate).
 * Nothing is promised where R_k is only the transform's rounding error: after pauses that hold an exactly periodic
 * signal and no noise, most bins' R_k, the weights and which samples are finite are decided by that rounding.
 * pcm: n_mics planes, chan_stride samples apart, each n_blocks*512 samples. 2 <= n_mics <= 8. */
typedef struct jdsp_mvdrn jdsp_mvdrn;
int jdsp_mvdrn_create(jdsp_ctx *ctx, int n_mics, const double *delays_s, double loading, jdsp_mvdrn **out);
/* The same with FFT_PROCESSING_LEN = n_fft: 1024 (= jdsp_mvdrn_create: the reference's frame) or 512 (BASELINE config 5
 * as worded, "8-mic array, 512-pt STFT": blocks of 256 samples, KEEP_LEN 255, frames [first 255 samples of the previous
 * block, block, 0], 257 bins at k * 16000 / 512 Hz, R_k += X X^H / 512, samples 255..510 out).  Blocks are then n_fft / 2
 * samples everywhere below. */
int jdsp_mvdrn_create_cfg(jdsp_ctx *ctx, int n_mics, const double *delays_s, double loading, int n_fft, jdsp_mvdrn **out);
int jdsp_mvdrn_block_len(const jdsp_mvdrn *h);
int jdsp_mvdrn_destroy(jdsp_mvdrn *h);
int jdsp_mvdrn_reset(jdsp_mvdrn *h);
long jdsp_mvdrn_blocks_out(const jdsp_mvdrn *h, long n_blocks);
int jdsp_mvdrn_process_dev(jdsp_mvdrn *h, const int16_t *pcm_dev, long chan_stride, long n_blocks, int16_t *out_dev,
                           float *precast_dev, long *n_out_blocks);
int jdsp_mvdrn_process(jdsp_mvdrn *h, const int16_t *pcm_host, long chan_stride, long n_blocks, int16_t *out_host,
                       float *precast_host, long *n_out_blocks);

/* Batched n-microphone MVDR: n_utts INDEPENDENT utterances in one launch sequence, each a fresh stream with the
 * handle's n_mics, delays_s and loading.  The entries neither read nor write the handle's own stream state (covariance,
 * previous block, run length, call count), so they may be interleaved with _process on the same handle.  1024-point
 * handles only: on an n_fft = 512 handle the three entries return JDSP_EINVAL with a text (two blocks share one inverse
 * transform there, and the pairing across utterance boundaries is not built).  The layout is jdsp_denoise_batch_dev's,
 * on n_mics planes; what is not restated here is as there.
 *   - Utterance u has B_u = block_first[u + 1] - block_first[u] blocks (>= 0) of 512 samples; its block b of
 *     microphone m is pcm[m chan_stride + sample_first[u] + 512 b .. + 512): the same offsets on every plane.  pcm is
 *     16-byte aligned and chan_stride a multiple of 8, as in jdsp_mvdrn_process_dev; sample_first[u] is only even.
 *   - Its result is what a fresh handle gives for _process of its B_u blocks: max(B_u - 1, 0) emitted blocks.  The
 *     emission for input block b >= 1 (the frame [first 511 samples of block b - 1 | block b | 0], silence in front of
 *     block 0) is written TIME-ALIGNED, at out[sample_first[u] + 512 b .. + 512); precast (the same samples before the
 *     (short) cast) likewise.  out and precast are single planes.  The first block of each span is never written, and the
 *     device entry touches no sample outside the spans.  Where the fresh handle's samples are non-finite -- before the
 *     utterance's first estimation frame, and with loading == 0 before n_mics of them -- so are these: the non-finite
 *     value in precast, 0 in out.
 *   - flags [n_blocks_total] uint8: the VAD decision of every block on microphone 0, in concatenated block order.  Any
 *     of the three output pointers may be NULL.
 *   - An utterance's out, precast and flags do not depend, bit for bit, on where it stands in the batch, on its
 *     neighbours, on gaps between the spans, on chan_stride, or on how the batch is split into calls: its estimation
 *     frames are cut into chunks of 128 for the covariance update, a cut that depends on nothing but their number.
 *     Against the oracle they are held to _process's bars; against _process of a fresh handle on the utterance alone
 *     they agree to those bars, and bit equality is NOT promised (_process cuts by the call's count of estimation
 *     frames).  Measured: for utterances of at most 128 estimation frames both cuts add one frame at a time from
 *     zero, and the bits were equal in every case tried -- 8 utterances on 8 microphones, and on 3 microphones 127 and
 *     128 frames as well as 129, 256 and 257, where the cuts differ (tests/test_mvdrn_batch_gpu.py prints it).
 *   - jdsp_mvdrn_batch_dev only enqueues on the context's stream: no allocation, no host synchronisation, no host
 *     read of the two offset arrays (int64, [n_utts] and [n_utts + 1], 8-byte aligned) -- hence n_blocks_total, which
 *     must equal block_first[n_utts].  It is graph-capturable, class S (Conventions): n_utts, n_blocks_total,
 *     chan_stride and the pointers are baked, the two offset arrays and the PCM are read at every replay, and a replay
 *     equals an eager call on the same contents bit for bit, as often as it is replayed.  The device-side offsets are
 *     the caller's contract: block_first[0] = 0 and non-decreasing; every sample_first[u] even, >= 0 and ascending; the
 *     spans, 512 B_u long, disjoint and inside every plane and the outputs.  No PCM outside the spans is read.  out and
 *     precast 4-byte aligned.
 *   - Its workspace comes from jdsp_mvdrn_batch_reserve, the only call that allocates (and synchronises), kept apart
 *     from _process's.  In the worst case every block is an estimation frame, so per reserved block it holds, as
 *     _process's does, one spectrum set and one weight set, (n_mics + 8) x 513 x 8 bytes (65.7 KB at 8 microphones);
 *     on top 8.2 KB of chunk sums (2 max_blocks_total / 128 + 2 slots of 513 x 64 x 16 bytes, used only by utterances of
 *     more than 128 estimation frames) and 9 bytes of flag, weight-row index and event list: 73.9 KB per block at 8
 *     microphones, 5.9 GB per 80,000 blocks; 8 bytes per reserved utterance.  A _dev call with more blocks or
 *     utterances than reserved is JDSP_EINVAL with a text.  A corpus larger than memory is split into calls by whole
 *     utterances; by the independence above the bits are the same.  A workspace below the worst case is not built.
 *   - jdsp_mvdrn_batch (host pointers, synchronous) reserves on demand, checks the offsets as jdsp_denoise_batch does
 *     and returns JDSP_EINVAL with a jdsp_last_error text otherwise.  pcm is n_mics planes chan_stride >= n_samples
 *     apart; out and precast are n_samples long and ZERO wherever the device entry would not write.
 *   - n_utts == 0, batches of empty utterances and all three outputs NULL succeed and launch nothing.  n_utts < 0 and
 *     misaligned base pointers are JDSP_EINVAL. */
int jdsp_mvdrn_batch_reserve(jdsp_mvdrn *h, long max_blocks_total, long max_utts);
int jdsp_mvdrn_batch_dev(jdsp_mvdrn *h, const int16_t *pcm_dev, long chan_stride, const int64_t *sample_first_dev,
                         const int64_t *block_first_dev, long n_utts, long n_blocks_total,
                         int16_t *out_dev, float *precast_dev, uint8_t *flags_dev);
int jdsp_mvdrn_batch(jdsp_mvdrn *h, const int16_t *pcm_host, long chan_stride, long n_samples,
                     const int64_t *sample_first_host, const int64_t *block_first_host, long n_utts,
                     int16_t *out_host, float *precast_host, uint8_t *flags_host);      /* host path, synchronous */

/* LIVE STREAMS on the n-microphone MVDR handle: n_streams independent streams of jdsp_mvdrn in the handle, next to its
 * own one, whose state (the per-bin covariance, the last block of every microphone, whether that block was quiet, the
 * counts of blocks and of estimation frames) lives ON THE DEVICE and is carried from call to call.  One call advances any subset of them by a ragged
 * chunk of new blocks each, in one launch sequence of six launches whatever the number of chunks.  The handle's own
 * _process stream and the _batch entries are neither read nor written, the three workspaces are kept apart, and the
 * three may be interleaved on the same handle.  1024-point handles only: on an n_fft = 512 handle every entry here
 * returns JDSP_EINVAL with a text, as the batch entries do.  (Vocabulary: jdsp_denoise_streams_*, above.)
 *   - A CHUNK is what one stream contributes to one call.  Chunk c belongs to stream stream_id[c] and holds B_c =
 *     block_first[c + 1] - block_first[c] NEW blocks (>= 0) of 512 samples per microphone, microphone m's at
 *     pcm[m chan_stride + sample_first[c] .. + 512 B_c): jdsp_mvdrn_batch_dev's layout with chunks for utterances, plus
 *     stream_id, and its alignment rules: pcm 16-byte aligned, chan_stride a multiple of 8, sample_first even, the int64
 *     arrays 8-byte, out and precast 4-byte aligned.  The handle keeps the history it needs: the caller never presents
 *     a block twice.
 *   - EMISSION IS TIME-ALIGNED, as in the batch.  A stream's block with index i (0-based, counted over all its calls)
 *     emits iff i >= 1: the frame [first 511 samples of block i - 1 | block i | 0], written at the block's own place,
 *     out[sample_first[c] + 512 b .. + 512) for block b of chunk c; precast (the same samples before the (short) cast)
 *     likewise.  out and precast are single planes.  The only block never written is block 0 of a stream's life; nothing
 *     outside the spans is read or written.  Non-finite samples -- before the stream's first estimation frame, and with
 *     loading == 0 before n_mics of them -- are the non-finite value in precast and 0 in out.  With loading == 0 this is
 *     a RULE here: a sum of fewer than n_mics outer products is singular by rank, the stream counts its estimation
 *     frames, and until there are n_mics of them the weights are NaN wherever the stream is cut.  _process and the
 *     batch leave such a matrix to the elimination's rounding, which may give finite, meaningless samples instead
 *     (observed: the block of the second estimation frame on 3 microphones); nothing is promised between them there.
 *   - ESTIMATION FRAMES.  Block i is one iff blocks i and i - 1 are both quiet and both in the stream, so whether the
 *     stream's last block was quiet is part of what it carries.  The covariance is the running sum of X X^H / 1024 over
 *     them, carried in FP64.  A chunk's estimation frames are walked ONE AFTER ANOTHER from the carried matrix, whatever
 *     their number: the chunk's blocks before its first one use the weights of the matrix carried in (a fresh stream's
 *     is zero: the non-finite weights of a fresh handle, row 0 of the batch), and every estimation frame adds one set.
 *     A LONG CHUNK IS THEREFORE SERIAL, about 3.6 us per estimation frame on one wave per eight bins: these entries are
 *     for the short chunks of live delivery, and a recording belongs to jdsp_mvdrn_batch.
 *   - CUT INDEPENDENCE, BIT FOR BIT: a stream's out, its finite precast samples, which samples are finite, its flags
 *     and its carried covariance do not depend on how its blocks are cut into chunks and calls -- one block per call
 *     counts, and so does a cut between the two quiet blocks of an estimation frame -- nor on the order of the chunks in
 *     a call, on the stream id, on n_streams, on the other streams of the call, on gaps between the spans or on
 *     chan_stride.  It follows from the walk: the sum is formed one frame at a time in the stream's own order wherever
 *     the cuts fall.  A promise, compared as bytes (tests/test_mvdrn_streams_gpu.py, tests/test_mvdrn_streams_hard_gpu.py).
 *   - AGAINST THE ORACLE AND THE BATCH.  A stream's spans, concatenated over its calls, are held to the oracle's stream
 *     of all its blocks at _process's bars (precast within 1e-5 of the stream's peak, int16 within 1 LSB, the same
 *     samples finite, flags equal).  Against jdsp_mvdrn_batch of ONE utterance of all its blocks the int16 and the
 *     finite float samples are equal as bytes while the utterance has at most 128 estimation frames: both then add one
 *     frame at a time from zero through the same code (loading > 0; at loading 0 from the n_mics-th estimation frame
 *     on, see above).  Beyond 128 the batch regroups its sums and only the bars are
 *     promised.  Sign and payload of a NaN in precast are not part of any comparison between different kernels.
 *   - A stream with no chunk in a call, or with a chunk of 0 blocks, is not touched.
 *   - jdsp_mvdrn_streams_reserve(h, n_streams, max_blocks_total) is the only call that allocates, and it synchronises.
 *     All streams start fresh; calling it again discards every stream.  Before it the other entries return JDSP_EINVAL
 *     with a text.  Per stream 533,516 bytes of state, each part held once: the covariance [513][8][8] complex FP64
 *     (525,312), the last block of 8 microphones (8,192), the count (8) and a word with the quiet bit and the
 *     estimation frames so far, saturated at 8 (4).  Per call a workspace for
 *     max_blocks_total blocks: per block, as jdsp_mvdrn_batch_reserve, one spectrum set and one weight set, (n_mics + 8)
 *     x 513 x 8 bytes (65.7 KB at 8 microphones), and 9 bytes of flag, weight-row index and event list; per stream one
 *     more weight set (32.8 KB: every chunk's first row solves the matrix carried in) and 4 bytes.  The weight table of
 *     a call has n_blocks_total + n_chunks rows.  A call beyond the reservation is JDSP_EINVAL.
 *   - jdsp_mvdrn_streams_dev and jdsp_mvdrn_streams_reset_dev only enqueue on the context's stream: no allocation, no
 *     host synchronisation, no host read of the arrays.  Graph-capturable, class D (Conventions): n_chunks / n_ids,
 *     n_blocks_total, chan_stride and the pointers are baked; ids, offsets and PCM are read at replay, and every replay
 *     advances the named streams from where they stand.  Checked on the host: n_chunks <= n_streams, n_blocks_total <=
 *     the reservation, the alignment.  The caller's contract on the device: ids in [0, n_streams) and distinct within a
 *     call; block_first[0] = 0, non-decreasing, block_first[n_chunks] = n_blocks_total; sample_first even; the spans
 *     disjoint and inside every plane and the outputs.
 *   - flags [n_blocks_total] uint8: the VAD decision of every block on microphone 0, in concatenated block order.  Any
 *     of the three output pointers may be NULL; with all of them NULL the state advances exactly as with them.
 *     n_chunks == 0 or n_blocks_total == 0 launches nothing and changes nothing.  reset_dev: the n_ids listed streams
 *     fresh again; stream_id_dev NULL: all of them.
 *   - jdsp_mvdrn_streams (host pointers, synchronous) checks all of that, duplicate ids and overlapping spans included,
 *     with sample_first ascending as in jdsp_mvdrn_batch, and on a violation returns JDSP_EINVAL with a jdsp_last_error
 *     text and leaves every stream as it was.  pcm is n_mics planes chan_stride >= n_samples apart; out and precast are
 *     n_samples long and ZERO wherever the device entry would not write.
 *   - jdsp_mvdrn_streams_state: blocks_seen [n_ids] int64 and cov [n_ids][513][8][8] complex as interleaved doubles in
 *     the handle's own layout (row, column; zeros for a fresh or reset stream).  Synchronises; either may be NULL. */
int jdsp_mvdrn_streams_reserve(jdsp_mvdrn *h, long n_streams, long max_blocks_total);
int jdsp_mvdrn_streams_reset_dev(jdsp_mvdrn *h, const int64_t *stream_id_dev, long n_ids);   /* NULL: all */
int jdsp_mvdrn_streams_dev(jdsp_mvdrn *h, const int16_t *pcm_dev, long chan_stride, const int64_t *stream_id_dev,
                           const int64_t *sample_first_dev, const int64_t *block_first_dev, long n_chunks,
                           long n_blocks_total, int16_t *out_dev, float *precast_dev, uint8_t *flags_dev);
int jdsp_mvdrn_streams(jdsp_mvdrn *h, const int16_t *pcm_host, long chan_stride, long n_samples,
                       const int64_t *stream_id_host, const int64_t *sample_first_host,
                       const int64_t *block_first_host, long n_chunks,
                       int16_t *out_host, float *precast_host, uint8_t *flags_host);       /* host path, synchronous */
int jdsp_mvdrn_streams_state(jdsp_mvdrn *h, const int64_t *stream_id_host, long n_ids,
                             int64_t *blocks_seen_host, double *cov_host);   /* synchronises; either may be NULL */

/* ---- MFCC ---------------------------------------------------------------------- */
/* MFCCFeatureExtraction_auto_version1.cpp.  The #defines at :23-33 become a runtime
 * configuration; jdsp_mfcc_native_cfg() fills in the reference's values
 * (window 1024, hop 512, 1024-FFT, first 512 bins, 38 channels over 0..22050 Hz,
 * 12 cepstra c1..c12, lifter 22, pre-emphasis 0.96).  n_fft may be 1024 or 512
 * (bins used: n_fft/2), win_len <= n_fft, n_chan <= 64, n_cep <= 32. */
typedef struct {
    int win_len, hop, n_fft, n_chan, n_cep, lifter;
    double half_rate, preemph;
} jdsp_mfcc_cfg;
typedef struct jdsp_mfcc jdsp_mfcc;
int jdsp_mfcc_native_cfg(jdsp_mfcc_cfg *cfg);
/* Runs MelFilterBankInit (:118-152) on the host for cfg and uploads the tables. */
int jdsp_mfcc_create(jdsp_ctx *ctx, const jdsp_mfcc_cfg *cfg, jdsp_mfcc **out);
int jdsp_mfcc_destroy(jdsp_mfcc *h);
/* MelFilterBankInit's three arrays (host): rgdMelFreqs[n_chan+1], rgdFiBins[n_fft/2],
 * rgdFilterBank[n_fft/2].  Any pointer may be NULL. */
int jdsp_mfcc_tables(const jdsp_mfcc *h, double *mel_freqs, int *fi_bins, double *fbank);
/* MFCCFeatureExtraction (:194-231) for n_frames frames: frame j = win_len samples at
 * pcm[frame_start[j]] (frame_start NULL: hop*j), x[0] of every frame is 0 as at :208.
 * feats: n_frames * n_cep doubles -- the reference's on-disk vector format (:99). */
int jdsp_mfcc_frames_dev(jdsp_mfcc *h, const int16_t *pcm_dev, const int64_t *frame_start_dev, long n_frames,
                         double *feats_dev);
int jdsp_mfcc_frames(jdsp_mfcc *h, const int16_t *pcm_host, long n_samples, const int64_t *frame_start_host,
                     long n_frames, double *feats_host);

/* The sub-steps of MFCCFeatureExtraction as functions of their own, for callers that keep the reference's
 * structure (jeicyboodsp_amd/compat: MelFilterBank, DCT, Liftering with the reference's signatures).  FP64 and the
 * reference's operation order; n_rows independent rows per call; host pointers.
 *   MelFilterBank (:154-174): abs = |X| of the first n_fft/2 bins per row -> mel = ln of the n_chan channel sums
 *   DCT           (:176-183): cep[n_cep] += sqrt(2/C) sum_k mel[k-1] cos(PI i (k-0.5)/C) -- ACCUMULATES into cep like
 *                             the reference (its caller zeroes dMFCCFeature first, :224)
 *   Liftering     (:185-192): cep[i-1] *= 1 + 0.5 L sin(PI i / L), in place */
int jdsp_mfcc_melfilterbank(jdsp_mfcc *h, const double *abs_host, long n_rows, double *mel_host);
int jdsp_mfcc_dct(jdsp_mfcc *h, const double *mel_host, long n_rows, double *cep_inout_host);
int jdsp_mfcc_liftering(jdsp_mfcc *h, double *cep_inout_host, long n_rows);

/* ---- GMM scoring / HMM recursion on MFCC vectors ------------- */
/* GMMAlgorithm_Test_Auto_ver2.cpp and Viterbi_version1.cpp consume the 12-double vectors the MFCC program
 * writes (MFCC:99); here they are read where jdsp_mfcc_frames_dev left them, in HBM.  The parameter records
 * are the programs' own (GMMTest:29-34; Viterbi:30-40), byte for byte, so a parameter file (GMMTest:76,
 * Viterbi:80) can be read straight into an array of them.  Everything is FP64 like the reference.
 * A batch is a set of utterances: utterance u owns the vectors utt_first[u] .. utt_first[u+1]-1
 * (n_utts + 1 offsets, non-decreasing). */
typedef struct {
    double alpa[4];
    double mean[4][12];
    double covariance[4][12][12];
    double eigenVector[4][12][4];
} jdsp_gmm_param;
typedef struct {
    jdsp_gmm_param gMMParam[6];
    double transProb[6][6];
} jdsp_hmm_param;

typedef struct jdsp_gmm jdsp_gmm;
/* classes: n_classes (1..256) records; what probability() reads of them (GMMTest:216-235) is packed and
 * uploaded: eigenVector, mean[k][0..3], covariance[k][i][i] for i < 4. */
int jdsp_gmm_create(jdsp_ctx *ctx, const jdsp_gmm_param *classes, int n_classes, jdsp_gmm **out);
int jdsp_gmm_destroy(jdsp_gmm *h);
/* "evaluation": 0 (default) evaluates probability() in the reference's operation order (un-fused products
 * and sums, IEEE division, four exp per mixture: GMMTest:228-233); 1 fuses it (FMA projection, -0.5/var
 * precomputed, one exp per mixture) -- about a third of the instructions, equal to a few 1e-16 relative
 * except where a mixture density is itself denormal. */
int jdsp_gmm_set_option(jdsp_gmm *h, const char *name, long value);
/* Recognition() (GMMTest:151-162) of every utterance against every class and main()'s arg-max
 * (GMMTest:113-127: `dMax < score`, first maximum wins).  scores: [n_utts][n_classes] doubles,
 * best (may be NULL): [n_utts] 0-based class indices.  feats: n_frames vectors, 16-byte aligned; offsets
 * outside [0, n_frames] are clamped on the device (nothing outside feats is ever read).  The host entry takes
 * n_frames from utt_first_host[n_utts] and requires utt_first_host[0] == 0. */
int jdsp_gmm_score_dev(jdsp_gmm *h, const double *feats_dev, long n_frames, const int64_t *utt_first_dev,
                       long n_utts, double *scores_dev, int *best_dev);
int jdsp_gmm_score(jdsp_gmm *h, const double *feats_host, const int64_t *utt_first_host, long n_utts,
                   double *scores_host, int *best_host);

/* probability() (GMMAlgorithm_Test_Auto_ver2.cpp:164-236, the live branch :216-235; = Viterbi_version1.cpp:248-267)
 * on its own: the density of n 12-double vectors under ONE mixture component given as the reference passes it --
 * pdMean (12 doubles, first 4 read), rgdCovariance[12][12] (diagonal entries 0..3 read), rgdEigenVector[12][4].
 * FP64, the reference's operation order.  Host pointers. */
int jdsp_gmm_probability(jdsp_ctx *ctx, const double *feats_host, long n, const double *mean12, const double *cov144,
                         const double *eig48, double *prob_host);

typedef struct jdsp_hmm jdsp_hmm;
/* models: n_models (1..1024) six-state records; log(transProb) is taken here, on the host (Viterbi:196). */
int jdsp_hmm_create(jdsp_ctx *ctx, const jdsp_hmm_param *models, int n_models, jdsp_hmm **out);
int jdsp_hmm_destroy(jdsp_hmm *h);
/* "evaluation": 0 (default) / 1, as jdsp_gmm_set_option, for the state densities. */
int jdsp_hmm_set_option(jdsp_hmm *h, const char *name, long value);
/* Sizes the emission scratch (n_frames * n_models * 6 doubles) ahead of time, e.g. before a graph capture. */
int jdsp_hmm_reserve(jdsp_hmm *h, long n_frames);
/* HMMRecognition() (Viterbi:157-246) as the reference computes it, quirks included (see
 * oracle/jdsp_oracle.h: log of the accumulated log probability at :196; the "decoding result" is the
 * per-frame arg-max state; the returned value is the frame-1 maximum).  n_frames = total vectors; every
 * utt_first offset must lie in [0, n_frames].  scores (may be NULL): [n_utts][n_models]; best (may be NULL):
 * [n_utts] arg-max model (Viterbi:119-126); path (may be NULL): [n_models][n_frames] states, 0 at each
 * utterance's first frame; trellis (may be NULL): [n_models][6][n_frames] = sProb.dHMMProb. */
int jdsp_hmm_viterbi_dev(jdsp_hmm *h, const double *feats_dev, long n_frames, const int64_t *utt_first_dev,
                         long n_utts, double *scores_dev, int *best_dev, int *path_dev, double *trellis_dev);
/* host entry: utt_first_host[0] must be 0 and utt_first_host[n_utts] is the total number of vectors */
int jdsp_hmm_viterbi(jdsp_hmm *h, const double *feats_host, const int64_t *utt_first_host, long n_utts,
                     double *scores_host, int *best_host, int *path_host, double *trellis_host);

/* ---- GMM training on MFCC vectors (GMMAlgorithm_Train_Auto_ver2.cpp) -------------- */
/* The reference's training program (Train:49-172) on vectors that are already in HBM: a class is trained from its
 * files in order.  First file of a class: mean[j] = frame[4j] (Train:120-124), KmeansAlogorithm (Train:342-438),
 * alpa[k] = 1/4 (Train:129-131).  Every file, the first included: EmAlgorithmBasedGmmParameter (Train:255-340),
 * exactly three iterations.  The record (Train:160) is PCADiagonalizeCovarianceMatrix (Train:456-518) of the state.
 * FP64 throughout; the reference's quirks are kept because they define the output:
 *   - k-means: Selection[i][j] is never cleared, so a frame counts for every cluster it was ever nearest to; the
 *     arg-min runs j = 0..3 with `>=` (a tie goes to the LAST index); the loop goes on while
 *     pass == 1 || fabs(cost - cost_before) >= 1.0; on exit the covariance is taken around the means that produced
 *     the last assignment, divided by the accumulated selection count.  An empty cluster keeps a zero mean and gets
 *     a 0/0 = NaN covariance (which then makes the whole class NaN through the E-step, as in the reference).
 *     Option "kmeans_max_passes" (default 10,000) bounds the loop: pass number max takes the exit branch whatever
 *     the cost did, and the class's stats.kmeans_capped is set.
 *   - EM: w[i][k] = probability_k(x_i) alpa[k] / sum_k (0/0 = NaN when all four are 0); alpa[k] += sum_i w[i][k]
 *     onto the OLD alpa, nOfKey[k] = alpa[k], alpa[k] /= n; mean[k] += sum_i w[i][k] x_i onto the OLD mean,
 *     then /= nOfKey[k]; covariance around the NEW mean, / nOfKey[k].  The print-only log-likelihood pass
 *     (Train:326-332) is not computed.
 *   - probability() (Train:189-253): the top 8 eigenpairs of the full 12x12 covariance, ranked as Train:218-235
 *     (rank = number of strictly larger eigenvalues; a missing rank keeps the previous pick), and
 *     prod_{i<8} (1/sqrt(2*3.141592)) (1/sqrt(l_i)) exp(-0.5 (y_i - m_i)^2 / l_i) with y = x^T E, m = mean^T E.  The
 *     decomposition does not depend on x: it is computed once per (class, mixture, EM iteration) on the device
 *     (cyclic Jacobi, at most 32 sweeps; a matrix with a non-finite entry gives NaN eigenpairs).
 *   - eigenvectors are defined up to sign: every kept column is made canonical -- its largest-magnitude component
 *     (first index on ties) is positive.  Column and projected mean flip together; no density changes.
 * Every sum over frames is ordered by frame index alone (64-frame tiles in ascending order), so results are
 * bit-identical across "threads_per_class" and however the files are cut into calls.  Differences from the
 * reference's ascending loops are rounding-level.  Defined here where the reference is not: the E-step buffer is
 * sized per file (Train:106 sizes it by the first file); an empty file and a first file of fewer than 13 frames are
 * errors. */
typedef struct {                        /* Train:26-32 with PCA_LEN 8: 8,096 bytes */
    double alpa[4];
    double mean[4][12];
    double covariance[4][12][12];
    double eigenVector[4][12][8];
} jdsp_gmm_train_param;
/* Per class: k-means passes of the class's first file, whether the pass cap ended it, the accumulated selection
 * counts and the final cost; files = files trained since reset; status = OR of JDSP_GMM_TRAIN_* flags recorded by
 * the _dev entry since reset (offsets outside [0, n_frames] clamped, files skipped).  A file whose class is out of
 * range belongs to no class: it is skipped and flagged in class 0's status.  Offsets that decrease anywhere are
 * flagged JDSP_GMM_TRAIN_UNORDERED in class 0's status: files whose (clamped) ranges then overlap share per-vector
 * workspace, and the results of their classes are unspecified -- nothing outside feats is read either way. */
typedef struct { int kmeans_passes, kmeans_capped, selected[4], files, status; double kmeans_cost; } jdsp_gmm_train_stats;
enum { JDSP_GMM_TRAIN_CLAMPED = 1, JDSP_GMM_TRAIN_BAD_CLASS = 2, JDSP_GMM_TRAIN_EMPTY_FILE = 4,
       JDSP_GMM_TRAIN_SHORT_FIRST = 8, JDSP_GMM_TRAIN_UNORDERED = 16 };
typedef struct jdsp_gmm_trainer jdsp_gmm_trainer;
int jdsp_gmm_train_create(jdsp_ctx *ctx, int n_classes, jdsp_gmm_trainer **out);   /* 1..1024 classes */
int jdsp_gmm_train_destroy(jdsp_gmm_trainer *h);
int jdsp_gmm_train_reset(jdsp_gmm_trainer *h);   /* every class back to "no file seen" (enqueued, no sync) */
/* "kmeans_max_passes" (>= 1, default 10,000); "threads_per_class" 256 / 512 / 1024 (default 256): workgroup size,
 * a tuning and testing knob -- the output does not depend on it. */
int jdsp_gmm_train_set_option(jdsp_gmm_trainer *h, const char *name, long value);
/* Sizes the per-frame workspace (selection bits and E-step weights: 33 bytes per vector) ahead of a graph capture.
 * max_files is accepted for symmetry with the other reserve entries and not used: nothing is sized by files. */
int jdsp_gmm_train_reserve(jdsp_gmm_trainer *h, long max_frames, long max_files);
/* Files f = 0..n_files-1: vectors file_first[f] .. file_first[f+1]-1 of feats (n_frames x double[12], 16-byte
 * aligned), belonging to class file_class[f]; the files of one class are trained in ascending f, after every file
 * that class received in earlier calls.  The _dev entry clamps offsets to [0, n_frames], skips empty files, files of
 * an out-of-range class and a class's first file when it has fewer than 13 vectors, and records each in stats; it
 * never reads outside feats.  The host entry rejects all of these with JDSP_EINVAL (file_first[0] must be 0). */
int jdsp_gmm_train_files_dev(jdsp_gmm_trainer *h, const double *feats_dev, long n_frames,
                             const int64_t *file_first_dev, const int32_t *file_class_dev, long n_files);
int jdsp_gmm_train_files(jdsp_gmm_trainer *h, const double *feats_host, const int64_t *file_first_host,
                         const int32_t *file_class_host, long n_files);   /* host pointers, synchronous */
/* PCADiagonalizeCovarianceMatrix (Train:456-518) of a COPY of each class's state: the state is unchanged and
 * training may go on.  mean[k][0..7] = projected mean, [8..11] = 0; covariance rows 0..7 zero with l_i on the
 * diagonal, rows 8..11 kept; eigenVector[k] = the 8 sorted, sign-canonical eigenvectors.  out: n_classes records.
 * The host entry's out_host and stats_host (n_classes each) may each be NULL. */
int jdsp_gmm_train_params_dev(jdsp_gmm_trainer *h, jdsp_gmm_train_param *out_dev);
int jdsp_gmm_train_params(jdsp_gmm_trainer *h, jdsp_gmm_train_param *out_host, jdsp_gmm_train_stats *stats_host);
/* Host only (no GPU needed): the PCA_LEN 4 record the test and Viterbi programs read (GMMTest:216-235) -- the first
 * four eigenvector columns, everything else copied.  in and out: n records. */
int jdsp_gmm_param_from_train(const jdsp_gmm_train_param *in, int n, jdsp_gmm_param *out);

/* ---- stream filters: layout common to jdsp_geq_* and jdsp_nlms_* ---------------------------- */
/* A handle filters n_streams independent streams, each with its own state; a call hands every stream its next
 * n_samples samples.  Stream s occupies elements s*pitch .. s*pitch + n_samples - 1 of every buffer of the call
 * (a buffer need not extend past the last stream's last sample); pitch >= n_samples and pitch is a multiple of 8,
 * device pointers are 16-byte aligned.  n_samples need not be a multiple of anything; n_samples == 0 is a successful
 * no-op.  A stream may be cut into calls anywhere: the results do not depend on the cut, on the number of streams or
 * on a stream's neighbours.  Everything is FP64 with every product and sum rounded on its own (no fused multiply-add),
 * as the reference's build rounds them. */

/* ---- 7-band graphic equaliser (7Band_GEQ.cpp) ------------------------------------------------ */
/* Host only, no GPU: CalcCoefficient (7Band_GEQ.cpp:136-257).  coeff[k] = {{b0, b1, b2}, {0, a1, a2}} of band k at
 * 44, 125, 250, 500, 2000, 6000, 11313 Hz (:47), 48 kHz, Q 4.318, PI 3.141592; gain_db NULL = the reference's +12,
 * +12, 0, 0, +3, 0, -12 dB (:51-57).  The reference chooses the boost or cut formulas at compile time; here the branch
 * follows the run-time sign of the gain (boost when > 0), and the formulas are the reference's as written: V inverted
 * when below 1 (:139-142), K of the band BELOW in every peaking a2 (:231, :247), the bass-cut branch's K where V is
 * meant (:173-174).  Only the reference's own gains are pinned to the compiled reference (bit for bit, with the C
 * library's tan, pow and sqrt); other gains follow the same text.  A non-finite gain is JDSP_EINVAL. */
int jdsp_geq_design(const double gain_db[7], double coeff[7][2][3]);
/* ApplyIirGEQ (7Band_GEQ.cpp:259-332) as a cascade of n_sections biquads (1 .. 16; the reference's is 7) over
 * n_streams (>= 1) streams.  coeff: [n_sections][2][3] as above ([k][1][0] is not read); NULL = jdsp_geq_design(NULL)
 * and needs n_sections == 7.  Per section, in the reference's order (:280-283):
 *   d = 0; d += b2 in[t-2]; d -= a2 out[t-2]; d += b1 in[t-1]; d -= a1 out[t-1]; d += b0 in[t];  out[t] = (short)d
 * Every section's output is cast to int16 before the next section reads it, as the reference's short buffers do; the
 * cast is the project's: truncate toward zero to int32, keep the low 16 bits (a loud stream wraps with the
 * reference's gains, exactly as the compiled reference does).  JDSP_EINVAL: n_sections or n_streams out of range, a
 * non-finite coefficient, or a section with |b0|+|b1|+|b2|+|a1|+|a2| >= 2^15 (the bound keeps every pre-cast value
 * inside int32, where the cast is defined). */
typedef struct jdsp_geq jdsp_geq;
int jdsp_geq_create(jdsp_ctx *ctx, const double *coeff, int n_sections, long n_streams, jdsp_geq **out);
int jdsp_geq_destroy(jdsp_geq *h);
int jdsp_geq_reset(jdsp_geq *h);                 /* every stream back to the zero keep (:261-262); enqueued, no sync */
/* out: int16 per sample; precast (may be NULL): the last section's d before its cast.  The _dev entry allocates
 * nothing and does not synchronise.  JDSP_EINVAL for a bad pitch or alignment. */
int jdsp_geq_process_dev(jdsp_geq *h, const int16_t *pcm_dev, long n_samples, long pitch, int16_t *out_dev,
                         double *precast_dev);
int jdsp_geq_process(jdsp_geq *h, const int16_t *pcm_host, long n_samples, long pitch, int16_t *out_host,
                     double *precast_host);
/* The state between calls, host int16 [n_streams][n_sections + 1][2], {older, newer}: row 0 the input's last two
 * samples, row k + 1 the last two outputs of section k (which are the input keep of section k + 1, :288-300).
 * Synchronous. */
int jdsp_geq_get_state(jdsp_geq *h, int16_t *state_host);
int jdsp_geq_set_state(jdsp_geq *h, const int16_t *state_host);

/* ---- normalised LMS adaptive filter (NormalLMS.cpp) ------------------------------------------ */
/* LMSFilter (NormalLMS.cpp:96-136), one sample at a time, for filter_len L = 64, 128 or 256 (the reference: 256), step
 * mu and regulariser compensation (the reference: 0.0001 both, :32-33).  With x = the kept L-1 samples followed by the
 * call's input and c the L coefficients (zero at first), sample i is
 *   sum = sum over j < L of c[L-1-j] x[i+j];  est[i] = (short)sum;  e = reference[i] - est[i] in int;  err[i] = (short)e
 *   c[m] += ((2.0 x[i+m]) mu) (double)e / (sum over j of x[i+j]^2 + compensation)          for every m < L  (:125)
 * The reference adds the L products in ascending j; here the order is fixed by L alone: with T = L/64, leaf l < 64 adds
 * the products j = T l .. T l + T - 1 in ascending j, and a balanced pairwise tree over the 64 leaves follows (adjacent
 * leaves first).  The sum reaches everything else only through its cast, the norm is an exact integer and the update
 * is per coefficient with a correctly rounded division, so the two orders can differ only at a sample whose sum lies
 * within rounding of an integer; on the committed reference streams they do not differ at all.  The cast of est is
 * the project's (truncate toward zero to int32, keep the low 16 bits); a filter driven past int32 is unspecified, as
 * in the reference.  precast (may be NULL) = sum.  Every sample gets its outputs: the reference's "first call returns
 * FALSE" (:132-135) is the caller's business.  JDSP_EINVAL: filter_len, n_streams < 1, non-finite mu or compensation,
 * a bad pitch or alignment. */
typedef struct jdsp_nlms jdsp_nlms;
int jdsp_nlms_create(jdsp_ctx *ctx, int filter_len, double mu, double compensation, long n_streams, jdsp_nlms **out);
int jdsp_nlms_destroy(jdsp_nlms *h);
int jdsp_nlms_reset(jdsp_nlms *h);               /* zero coefficients and keep (:98-99); enqueued, no sync */
int jdsp_nlms_process_dev(jdsp_nlms *h, const int16_t *input_dev, const int16_t *reference_dev, long n_samples,
                          long pitch, int16_t *est_dev, int16_t *err_dev, double *precast_dev);
int jdsp_nlms_process(jdsp_nlms *h, const int16_t *input_host, const int16_t *reference_host, long n_samples,
                      long pitch, int16_t *est_host, int16_t *err_host, double *precast_host);
/* coefficients: host double [n_streams][L] (rgsdCoefficient, :99); keep: host int16 [n_streams][L-1], oldest first
 * (rgssKeepInput, :98).  get: either may be NULL.  Synchronous. */
int jdsp_nlms_get_state(jdsp_nlms *h, double *coef_host, int16_t *keep_host);
int jdsp_nlms_set_state(jdsp_nlms *h, const double *coef_host, const int16_t *keep_host);

#ifdef __cplusplus
}
#endif
#endif /* JDSP_H */
