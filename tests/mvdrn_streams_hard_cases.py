"""The cases the hard-scene tests of the live n-microphone MVDR streams share (jdsp_mvdrn_streams*, include/jdsp.h): the
plans that cut the 30-block scenes of tests/mvdrn_cases.py where a live stream has state of its own to carry, the streams
of the loading-0 rule on 2, 5 and 8 microphones, and the figure and the bar the carried covariance is held to.  The
scenes, the restatements and the output bars are tests/mvdrn_cases.py's (H), the packing and the check
tests/mvdrn_batch_cases.py's (K), the delivery tests/mvdrn_streams_cases.py's (S).  No GPU import:
tests/test_mvdrn_streams_hard_cpu.py shows with the oracle and the restatements alone that the GPU comparisons of
tests/test_mvdrn_streams_hard_gpu.py are not vacuous.

H.QUIET makes blocks 1 .. 8 and 19 .. 22 of every scene the estimation frames, so event k of the first pause is block k."""
import numpy as np

import mvdrn_batch_cases as K
import mvdrn_cases as H
import mvdrn_streams_cases as S
from mvdrn_batch_cases import B

N = H.N_BLOCKS
EVENTS = list(range(1, 9)) + list(range(19, 23))          # the estimation frames of every scene (the CPU test asserts it)
FIRST_PAUSE = H.QUIET[0][1]                               # blocks 0 .. 8: a chunk that ends with block 8 ends the first pause
CUT_SCENES = ["coherent", "hum", "dc", "near", "quiet_mic0", "steering_frac"]
CUT_LOADINGS = [1e-6, 0.0]
RULE_MICS = [2, 5, 8]                                     # 3 microphones: S.loading0_stream
COV_MARGIN = 4.0                                          # over ref32's own figure, see cov_bar()
MUTANT_FACTOR = 100.0                                     # a wrong covariance misses the bar by this much at the least


# ---- plans over the 30-block scenes -----------------------------------------------------------------------------------
def opens(n_mics):
    """the blocks that open a chunk of edges(n_mics), block 0 aside:
      1        the first estimation frame: behind a chunk that is block 0 alone, the one a life emits nothing for
      n_mics   the n_mics-th estimation frame is a chunk's block 0: it reads the carried block of every microphone and
               the carried quiet bit, the carried count is n_mics - 1, and at loading 0 it is the first finite block
      9        a loud block behind a quiet one; the chunk in front of it ends with block 8, the first pause's last
      18       quiet behind a loud block: no estimation frame
      19       an estimation frame through the carried quiet bit and the carried block 18 alone
      20       one more, a chunk of one block between two cuts
      23       loud behind a quiet block"""
    return sorted({1, n_mics, 9, 18, 19, 20, 23})


def edges(n_mics):
    """the chunk sizes of the plan that opens a chunk at every block of opens(n_mics), a chunk of 0 blocks in front of
    the one that opens at block 19"""
    at = [0] + opens(n_mics) + [N]
    sizes = [b - a for a, b in zip(at[:-1], at[1:])]
    sizes.insert(at.index(19), 0)
    return sizes


def cuts(kind, n_mics):
    return {"whole": [N], "each": S.cuts_each(N), "random": S.cuts_random(7 + n_mics, N), "edges": edges(n_mics)}[kind]


def chunk_opens(sizes):
    """the block every chunk of non-zero size opens at"""
    at = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    return [int(a) for a, n in zip(at, sizes) if n > 0]


def calls_upto(sizes, block):
    """the number of leading chunks that end with `block`"""
    ends = np.cumsum(sizes).tolist()
    return ends.index(block + 1) + 1


# ---- the rule streams ---------------------------------------------------------------------------------------------------
def rule_stream(n_mics, seed=91):
    """n_mics + 9 blocks, blocks 0 .. n_mics + 2 quiet: the estimation frames are blocks 1 .. n_mics + 2, the n_mics-th
    is block n_mics, two more follow it, and six loud blocks close the stream.  S.loading0_stream at other counts."""
    return K.utterance(seed + n_mics, n_mics, n_mics + 9, quiet=((0, n_mics + 3),))


def rule_events(n_mics):
    return list(range(1, n_mics + 3))


def rule_held(flags, n_mics):
    """bool per emitted sample: n_mics or more estimation frames seen, counted from the VAD flags (the oracle's), never
    from an output.  It leaves out the n_mics - 1 emitted blocks 1 .. n_mics - 1 of the n_mics + 8: 1, 4 and 7.
    (H.held_mask has the same rule under a ceiling table without a key 5.)"""
    held = H.events_upto(flags)[1:] >= n_mics
    assert held.size == n_mics + 8 and np.count_nonzero(~held) == n_mics - 1, (held.tolist(), n_mics)
    assert not held[:n_mics - 1].any() and held[n_mics - 1:].all()
    return np.repeat(held, B)


def rule_plans(n_mics):
    """one chunk; cut so that the n_mics-th estimation frame opens the second chunk; one block per call"""
    n = n_mics + 9
    return {"whole": [n], "cut": [n_mics, n - n_mics], "each": S.cuts_each(n)}


RULE_LATE = 3                                             # the second stream of rule_pair_plan starts this many calls later


def rule_pair_plan(n, late=RULE_LATE):
    """two streams of n blocks one block per call, stream 1 `late` calls behind stream 0: in every call that holds both
    their counts of estimation frames differ"""
    return [[(0, 1)] * (k < n) + [(1, 1)] * (late <= k) for k in range(n + late)]


# ---- the covariance -----------------------------------------------------------------------------------------------------
def frame_spectra(pcm, blocks, mode="64", before=None):
    """X [len(blocks), bins, n_mics] complex128 of the estimation frames [block b - 1 | block b] as H._run forms them
    (mode "64": FP64; "32": an FP32 radix-2 transform, the spectrum rounded to FP32).  before: {b: int16 [n_mics, 512]}
    puts something else in the place of block b - 1 (the mutants of the CPU test)."""
    out = []
    for b in blocks:
        frame = np.array(pcm[:, (b - 1) * B:(b + 1) * B])
        if before is not None and b in before:
            frame[:, :B] = before[b]
        out.append(H._spectra(frame, mode).astype(complex).T)
    return np.array(out).reshape(len(blocks), B + 1, pcm.shape[0])


def covariance_of(X):
    """the running sum of X X^H / 1024 over the frames of frame_spectra, in H._run's order and arithmetic: R[k, i, j] =
    sum X_i conj(X_j) / 1024, row i, column j"""
    R = np.zeros(X.shape[1:] + X.shape[2:], complex)
    for x in X:
        R += x[:, :, None] * x[:, None, :].conj() / (2 * B)
    return R


def covariance(pcm, n_blocks=None, mode="64"):
    """the covariance a stream carries after its first n_blocks blocks (all of them by default), its estimation frames
    taken from EVENTS.  Bit for bit H.ref64(pcm[:, :512 n_blocks], ...)["R"] (H.ref32's with mode "32")."""
    n_blocks = pcm.shape[1] // B if n_blocks is None else n_blocks
    return covariance_of(frame_spectra(pcm, [e for e in EVENTS if e < n_blocks], mode))


def cov_figure(C, R):
    """the largest over bins and entries of |C[k, i, j] - R[k, i, j]| / sqrt(R[k, i, i] R[k, j, j]): per entry and per
    bin.  (A figure relative to the largest diagonal over all bins says nothing on `dc`, where bin 0 dominates.)"""
    d = np.sqrt(np.einsum("kii->ki", R).real)
    return float((np.abs(C - R) / (d[:, :, None] * d[:, None, :])).max())


_bars = {}


def cov_ref32_figure(name, n_mics):
    """the figure of plain FP32's covariance at the end of the scene (H.ref32's R: FP32 radix-2 transforms, FP64 sums)
    against ref64's; with it ref64's R, both computed once"""
    key = (name, n_mics)
    if key not in _bars:
        pcm = H.cached_scene(name, n_mics)[0]
        R = covariance(pcm)
        R.setflags(write=False)
        _bars[key] = (cov_figure(covariance(pcm, mode="32"), R), R)
    return _bars[key]


def cov_bar(name, n_mics):
    """The bar of a carried covariance on a scene: COV_MARGIN x the figure of ref32 against ref64, from the two
    restatements and never from the kernel.  The margin: the kernel's transform has ref32's order of rounding error but
    not its pattern -- radix-8 passes, a split real transform and a 0.5 prescale against radix 2 on a zero imaginary
    part -- and 4 x a reference's own error is what the LPC tests give a kernel over theirs."""
    return COV_MARGIN * cov_ref32_figure(name, n_mics)[0]


def cov_ref64(name, n_mics, n_blocks=None):
    """ref64's covariance of the scene after n_blocks blocks (None: at its end)"""
    if n_blocks is None:
        return cov_ref32_figure(name, n_mics)[1]
    return covariance(H.cached_scene(name, n_mics)[0], n_blocks)


def check_cov(cov, R, n_mics, bar):
    """A carried covariance [513, 8, 8] against ref64's R [513, n_mics, n_mics]; returns its share of the bar.
    Rows and columns from n_mics on are exactly zero, every diagonal entry has imaginary part exactly 0, and
    cov[k, i, j] == conj(cov[k, j, i]) exactly (-0 counts as 0): mvn_row_add forms entry (i, j) as
    (xi.x xj.x + xi.y xj.y) / 1024 and (xi.y xj.x - xi.x xj.y) / 1024 from FP32 values in FP64, where every product is
    exact, so (i, j) and (j, i) are the same exact sums, one the negative of the other in the imaginary part, rounded once,
    scaled by a power of two and accumulated in the same order."""
    assert cov.shape == (B + 1, 8, 8) and R.shape == (B + 1, n_mics, n_mics)
    assert not cov[:, n_mics:, :].any() and not cov[:, :, n_mics:].any(), "rows and columns past n_mics"
    assert not np.einsum("kii->ki", cov).imag.any(), "a diagonal with an imaginary part"
    assert np.array_equal(cov, np.conj(np.swapaxes(cov, 1, 2))), "not Hermitian bit for bit"
    s = cov_figure(cov[:, :n_mics, :n_mics], R) / bar
    assert s < 1.0, s
    return s
