"""The scenes, delays and matrices white noise does not reach, for the two-microphone MVDR (jdsp_mvdr_*, include/jdsp.h):
the scenes, two numpy restatements of oracle/jdsp_oracle.c's orc_mvdr_stream (and of orc_mvdr_process_block under one
caller matrix), four mutants of the FP64 one, three blocks on the VAD's threshold and the bars.  No GPU import:
tests/test_mvdr_hard_cpu.py shows on the CPU that every scene is sized for the bar and sees what `white` at whole-sample
delays cannot, tests/test_mvdr_hard_gpu.py holds the three block paths to the bar on them.

Bars (the header's): precast within 1e-5 of the stream's own finite peak, int16 within 1 LSB modulo 2^16 (with a delay
the chain has gain above 1 and a full-scale stream leaves int16: both sides keep the low 16 bits), finite masks equal,
all against the C oracle.  On top, the tight bar: plain FP32 arithmetic (ref32: a radix-2 transform, weights rounded
from FP64) takes 0.013 to 0.047 of the 1e-5 bar here, so a kernel is also held to max(TIGHT x that share, 0.1)."""
import numpy as np

from mvdrn_cases import _fft32

FS = 16000.0
TOL = 1e-5
N_BLOCKS = 30                       # blocks of 512 samples
QUIET = ((0, 9), (18, 5))           # (first block, blocks) without the source
DELAYS = [0.0, 2.5e-4, 1e-4, 1.37 * 6.25e-5, -2.5e-3, 1e-2]     # none, 4 samples, 1.6, 1.37, -40, 160 (wraps over the bins)
SCENES = ["white", "gain_mismatch", "quiet_right", "quiet_left", "always_quiet", "dead_right_in_pauses", "dc", "hum",
          "lowpassed", "full_scale", "identical", "tone"]
NEW_SCENES = SCENES[1:]
NEVER_LOUD = ("quiet_left", "always_quiet")          # the VAD's channel never speaks: every block but the first an event
# The kernel's share of the bar may be this many times plain FP32's (or 0.1 of the bar, whichever is larger): a margin
# for another radix and the packed real transform over the 1.6x the n-microphone kernels measured against the same
# kind of model (profiles/r23_mvdrn_hard.txt).
TIGHT = 4.0
TIGHT_FLOOR = 0.1
MUTANTS = ["no_quirk", "stale", "swap", "mirror_conj"]
MATRICES = {
    "hand": (4e6, 1.5e5, -2.5e5, 3e6),
    "diag_1e15": (1e15, 0.0, 0.0, 1.0),
    "skew": (2e6, 8e5, -8e5, 1e6),
    "neg_offdiag": (3e6, -2.9e6, -2.9e6, 3e6),
    "near_singular": (1e6, 1e6 * (1 - 1e-6), 1e6 * (1 - 1e-6), 1e6),
    "tiny": (3e-6, 1e-7, 1e-7, 2e-6),
}
APPLY_DELAYS = [0.0, 1e-4, -2.5e-3]
VAD_SUMS = (716799, 716800, 716801)                  # 700 x 1024 and its neighbours: quiet, quiet, voice


def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _loud(n_blocks):
    loud = np.ones(n_blocks * 512)
    for b0, nb in QUIET:
        loud[b0 * 512:(b0 + nb) * 512] = 0
    return loud


def scene(name, seed=1, n_blocks=N_BLOCKS):
    """(L, R) int16 of n_blocks blocks.  The source is white, sd 3000, silent in QUIET; L hears it as it is, R at 0.7
    and two samples later (`its source`).
      white                 L + N(0,45) + N(0,300) while loud, R + N(0,60) + N(0,400) while loud: today's scene
      gain_mismatch         R = 1e-2 (its source + N(0,60)): R11 four decades under R00
      quiet_right           R = 1e-3 its source + N(0,0.6): +-1 LSB, eight decades on the diagonal
      quiet_left            L = 1e-3 src + N(0,1), R = its source + N(0,3000) always: the VAD's channel never speaks
      always_quiet          L = N(0,20), R = N(0,5000): the same, R carrying a full signal into the matrix
      dead_right_in_pauses  R = its source only, exactly 0 in the pauses: R11 = 0, det = 0, nothing finite
      dc                    + 10 + N(0,1) on L, - 15 + N(0,1) on R: pause energy in bin 0
      hum                   + 60 sin(2 pi 50 t / fs) + N(0,0.5), on R three samples later: a tonal pause
      lowpassed             + N(0,150) through a 32-tap mean, independent per channel: matrix versions that move
      full_scale            10 src (clipped) + N(0,45), 10 its source (clipped) + N(0,60)
      identical             L = R = src + N(0,45): a = d exactly
      tone                  12000 sin(2 pi 1000.3 t / fs) while loud + N(0,45); 9000 of it two samples later + N(0,60)"""
    n = n_blocks * 512
    rng = np.random.default_rng(seed)
    loud = np.tile(_loud(N_BLOCKS), -(-n_blocks // N_BLOCKS))[:n]
    t = np.arange(n)
    src = rng.normal(0, 3000, n)
    its = 0.7 * np.roll(src, 2) * loud                   # silent in the pauses too: nothing of it rolls into one
    src = src * loud
    if name == "white":
        L = src + rng.normal(0, 45, n) + rng.normal(0, 300, n) * loud
        R = its + rng.normal(0, 60, n) + rng.normal(0, 400, n) * loud
    elif name == "gain_mismatch":
        L = src + rng.normal(0, 45, n)
        R = 1e-2 * (its + rng.normal(0, 60, n))
    elif name == "quiet_right":
        L = src + rng.normal(0, 45, n)
        R = 1e-3 * its + rng.normal(0, 0.6, n)
    elif name == "quiet_left":
        L = 1e-3 * src + rng.normal(0, 1, n)
        R = its + rng.normal(0, 3000, n)
    elif name == "always_quiet":
        L = rng.normal(0, 20, n)
        R = rng.normal(0, 5000, n)
    elif name == "dead_right_in_pauses":
        L = src + rng.normal(0, 45, n)
        R = its
    elif name == "dc":
        L = src + 10 + rng.normal(0, 1, n)
        R = its - 15 + rng.normal(0, 1, n)
    elif name == "hum":
        L = src + 60 * np.sin(2 * np.pi * 50 * t / FS) + rng.normal(0, 0.5, n)
        R = its + 60 * np.sin(2 * np.pi * 50 * (t - 3) / FS) + rng.normal(0, 0.5, n)
    elif name == "lowpassed":
        L = src + np.convolve(rng.normal(0, 150, n + 31), np.ones(32) / 32, "valid")
        R = its + np.convolve(rng.normal(0, 150, n + 31), np.ones(32) / 32, "valid")
    elif name == "full_scale":
        L = np.clip(10 * src, -32768, 32767) + rng.normal(0, 45, n)
        R = np.clip(10 * its, -32768, 32767) + rng.normal(0, 60, n)
    elif name == "identical":
        L = src + rng.normal(0, 45, n)
        R = L
    elif name == "tone":
        L = 12000 * np.sin(2 * np.pi * 1000.3 * t / FS) * loud + rng.normal(0, 45, n)
        R = 9000 * np.sin(2 * np.pi * 1000.3 * (t - 2) / FS) * loud + rng.normal(0, 60, n)
    else:
        raise KeyError(name)
    return _i16(L), _i16(R)


_scenes = {}


def cached_scene(name, n_blocks=N_BLOCKS):
    """scene(name, 1, n_blocks), built once and read-only"""
    key = (name, n_blocks)
    if key not in _scenes:
        L, R = scene(name, 1, n_blocks)
        L.setflags(write=False)
        R.setflags(write=False)
        _scenes[key] = (L, R)
    return _scenes[key]


def loud_blocks(L, R):
    """blocks 9..17, the first loud stretch (the keep buffers start from silence, eight blocks come out)"""
    b0, b1 = QUIET[0][1], QUIET[1][0]
    return L[b0 * 512:b1 * 512], R[b0 * 512:b1 * 512]


def pause_frames(x, flags):
    """the [previous block, block] frames of the stream's estimation events, [n, 1024]"""
    quiet = np.asarray(flags) == 0
    ev = np.flatnonzero(quiet[1:] & quiet[:-1]) + 1
    return np.stack([x[(b - 1) * 512:(b + 1) * 512] for b in ev])


# ---- the restatements -----------------------------------------------------------------------------------------------
_WIN = 0.54 - 0.46 * np.cos(2 * 3.141592 * np.arange(1024) / 1023)


def vad_sums(blocks):
    """BF:207-242's energy sum of every block [n, 512]: the frame is [511 zeros, block, 0], every sample is windowed
    and truncated back to short, the squares are summed (an integer); voice iff sum / 1024 > 700.0"""
    x = np.asarray(blocks, np.float64).reshape(-1, 512)
    return (np.trunc(x * _WIN[511:1023]) ** 2).sum(1).astype(np.int64)


def _steer(d_time, mutant=None):
    """(cos, sin)(2 PI i fs / N dTime) for i = 0 .. 1023, PI = 3.141592 (:164-165): the angle keeps growing above bin 512"""
    i = np.arange(1024)
    if mutant == "mirror_conj":
        i = np.where(i > 512, i - 1024, i)
    return np.exp(1j * (2 * 3.141592 * i * (FS / 1024) * d_time))


def _frames(x):
    """[511 samples of the previous block (silence in front of the first) | block | 0] per block, [nb, 1024] float64"""
    nb = x.size // 512
    blocks = np.asarray(x, np.float64).reshape(nb, 512)
    f = np.zeros((nb, 1024))
    f[1:, :511] = blocks[:-1, :511]
    f[:, 511:1023] = blocks
    return f


def _process(L, R, R4, d_time, fp32, mutant=None):
    """ProcessMVDR (:124-205) on every block with the matrix R4[b] (row-major, [nb, 4]).  Returns (the emitted samples
    before the cast: blocks 1 .. nb - 1, |den| [nb, 1024])."""
    nb = L.size // 512
    s1 = _steer(d_time, mutant)[None, :]
    with np.errstate(all="ignore"):
        a, b, c, d = (R4[:, k, None] for k in range(4))
        invdet = 1.0 / (a * d - b * c)                                   # mxAutoCorr.inverse() (:170)
        i00, i01, i10, i11 = d * invdet, -b * invdet, -c * invdet, a * invdet
        w0, w1 = i00 + i01 * s1, i10 + i11 * s1
        den = w0 + np.conj(s1) * w1                                      # :171
        w0, w1 = w0 / den, w1 / den
        if mutant == "swap":
            w0, w1 = w1, w0
        lw0, lw1, rw0, rw1 = w0.real, -w0.imag, w1.real, -w1.imag        # :175-178
        if fp32:
            FL, FR = _fft32(_frames(L).astype(np.float32)), _fft32(_frames(R).astype(np.float32))
            lw0, lw1, rw0, rw1 = (w.astype(np.float32) for w in (lw0, lw1, rw0, rw1))
        else:
            FL, FR = np.fft.fft(_frames(L), axis=-1), np.fft.fft(_frames(R), axis=-1)
        # :180-183 -- the imaginary part is formed from the ALREADY OVERWRITTEN real part
        lre = FL.real * lw0 - FL.imag * lw1
        lim = (FL.real if mutant == "no_quirk" else lre) * lw1 + FL.imag * lw0
        rre = FR.real * rw0 - FR.imag * rw1
        rim = (FR.real if mutant == "no_quirk" else rre) * rw1 + FR.imag * rw0
        mre, mim = lre + rre, lim + rim                                  # :184-185
        if fp32:
            # the real part of the inverse transform = the inverse transform of the Hermitian part
            mirror = (-np.arange(1024)) % 1024
            half = np.float32(0.5)
            herm = (half * (mre + mre[:, mirror])) + 1j * (half * (mim - mim[:, mirror]))
            y = np.conj(_fft32(np.conj(herm.astype(np.complex64)))).real * np.float32(1.0 / 1024)
        else:
            y = np.fft.ifft(mre + 1j * mim, axis=-1).real
    return np.asarray(y[1:, 511:1023], np.float64).reshape(-1), np.abs(den)


def _stream(L, R, d_time, fp32, mutant=None):
    L, R = np.asarray(L), np.asarray(R)
    nb = L.size // 512
    sums = vad_sums(L)
    flags = (sums / 1024.0 > 700.0).astype(np.uint8)                     # :233, the energy alone decides
    quiet = flags == 0
    event = np.zeros(nb, bool)
    event[1:] = quiet[1:] & quiet[:-1]                                   # the run counter (:191-219) beyond 1
    el = (np.asarray(L, np.float64) ** 2).reshape(nb, 512).sum(1)
    er = (np.asarray(R, np.float64) ** 2).reshape(nb, 512).sum(1)
    delta = np.zeros((nb, 4))
    delta[1:, 0] = (el[1:] + el[:-1]) * event[1:]                        # :263-268 by Parseval: (sum l^2, 0, 0, sum r^2)
    delta[1:, 3] = (er[1:] + er[:-1]) * event[1:]
    trace = np.cumsum(delta, axis=0)                                     # the update in front of the apply
    used = trace
    if mutant == "stale":
        used = np.concatenate([np.zeros((1, 4)), trace[:-1]])
    pre, den = _process(L, R, used, d_time, fp32, mutant)
    return {"pre": pre, "flags": flags, "sums": sums, "events": int(event.sum()), "trace": trace, "corr": trace[-1], "den": den}


def ref64(L, R, d_time, mutant=None):
    """FP64 restatement of orc_mvdr_stream.  A dict: pre (the emitted samples before the cast), flags and sums (the
    VAD's decision and energy sum per block), events, trace (the matrix in effect per block), corr (the last one).
    mutant: "no_quirk" forms the imaginary part from the real part as it was, "stale" processes an estimation block with
    the weights from before its own update, "swap" exchanges the two weights, "mirror_conj" takes the steering of a bin
    above 512 as the conjugate of its mirror's (the reference's angle keeps growing)."""
    return _stream(L, R, d_time, False, mutant)


def ref32(L, R, d_time):
    """The same chain in plain FP32: radix-2 FP32 transforms of the frames, weights formed in FP64 and rounded, apply,
    merge and Hermitian part in FP32, an FP32 inverse transform times 1 / 1024."""
    return _stream(L, R, d_time, True)


def _apply(L, R, corr4, d_time, fp32):
    L, R = np.asarray(L), np.asarray(R)
    R4 = np.tile(np.asarray(corr4, np.float64).reshape(1, 4), (L.size // 512, 1))
    pre, den = _process(L, R, R4, d_time, fp32)
    return {"pre": pre, "den": den[0]}


def apply_ref64(L, R, corr4, d_time):
    """orc_mvdr_process_block on every block with one caller matrix (oracle.mvdr_apply); den is |c^H R^-1 c| per bin"""
    return _apply(L, R, corr4, d_time, False)


def apply_ref32(L, R, corr4, d_time):
    return _apply(L, R, corr4, d_time, True)


# ---- three blocks on the VAD's threshold ----------------------------------------------------------------------------
def vad_edge_blocks(seed=7):
    """int16 [3, 512]: blocks whose windowed, truncated energy sums are exactly VAD_SUMS.  A seeded greedy search: N(0,
    58) with one sample in eight set to zero lies below the target; then one sample's truncated value is raised by one
    step (its square by 2 |t| + 1) at a time, the sample drawn among those whose step still fits.  Each block continues
    the one before it, so two neighbours differ in one sample."""
    rng = np.random.default_rng(seed)
    w = _WIN[511:1023]
    x = np.rint(rng.normal(0, 58, 512))
    x[rng.random(512) < 0.125] = 0
    sign = np.where(x < 0, -1.0, 1.0)
    t = np.abs(np.trunc(x * w))
    assert (t ** 2).sum() < VAD_SUMS[0] - 5000
    out = []
    for target in VAD_SUMS:
        while True:
            left = target - int((t ** 2).sum())
            if left == 0:
                break
            step = 2 * t + 1
            fits = np.flatnonzero((step <= left) & ((t >= 8) | (left < 4000)))
            assert fits.size, left
            i = fits[rng.integers(fits.size)]
            t[i] += 1
            x[i] = sign[i] * np.ceil(t[i] / w[i])                       # the smallest magnitude that truncates to t
            assert abs(np.trunc(x[i] * w[i])) == t[i]
        out.append(x.astype(np.int16))
    blocks = np.stack(out)
    assert np.abs(blocks).max() < 2000
    return blocks


def vad_edge_stream():
    """`white` with the 716,800 block as every block of L's first pause and the 716,801 block as block 20, in the
    second: (L, R, the flags that follow).  Block 20 is voice and resets the run counter: block 21 is no event."""
    L, R = (x.copy() for x in cached_scene("white"))
    edge = vad_edge_blocks()
    for b in range(QUIET[0][1]):
        L[b * 512:(b + 1) * 512] = edge[1]
    L[20 * 512:21 * 512] = edge[2]
    flags = (_loud(N_BLOCKS)[::512] > 0).astype(np.uint8)
    flags[20] = 1
    return L, R, flags


# ---- the bars -------------------------------------------------------------------------------------------------------
def share(pre, o_pre):
    """(the share of the 1e-5 bar the worst sample finite on both sides takes, whether the finite masks agree)"""
    pre, o_pre = np.asarray(pre, np.float64), np.asarray(o_pre, np.float64)
    fin = np.isfinite(o_pre)
    same = np.array_equal(np.isfinite(pre), fin)
    both = fin & np.isfinite(pre)
    if not both.any():
        return 0.0, same
    return float(np.abs(pre[both] - o_pre[both]).max() / (TOL * max(np.abs(o_pre[fin]).max(), 1.0))), same


def check(out, pre, o_out, o_pre, plain_share=None):
    """The header's bars, and with plain_share (ref32's share of the bar on the same case) the tight one.  Returns the
    share of the 1e-5 bar."""
    out, pre = np.asarray(out), np.asarray(pre)
    assert out.shape == o_out.shape and pre.shape == o_pre.shape and out.dtype == np.int16
    s, same = share(pre, o_pre)
    assert same, "finite masks differ"
    assert s <= 1.0, s
    fin = np.isfinite(o_pre)
    peak = max(np.abs(o_pre[fin]).max(), 1.0) if fin.any() else 1.0
    if out.size and TOL * peak <= 0.5:                   # above that the bar itself is more than an LSB
        diff = ((out.astype(np.int64) - o_out.astype(np.int64) + 32768) % 65536) - 32768     # modulo 2^16: both sides wrap
        assert np.abs(diff).max() <= 1, np.abs(diff).max()
    if plain_share is not None:
        assert s <= max(TIGHT * plain_share, TIGHT_FLOOR), (s, plain_share)
    return s
