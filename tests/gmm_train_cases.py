"""Synthetic training data for the GMM trainer's tests and bench leg: every class is drawn from 4 anisotropic
Gaussian clusters (covariance eigenvalues a factor of 2 apart, random axes), far from the origin and from each other,
so that no k-means decision or kept eigen-subspace sits near a tie.  The first 16 vectors of every file come from
clusters 0,0,0,0,1,1,1,1,2,... so that the k-means start (vectors 0, 4, 8, 12: Train:120-124) has one vector per
cluster.

overlapping_models and wide_models leave that safety on purpose (several k-means passes, rows with several selection
bits, soft E-step weights, wide spectra): the scenes built on them (HARD_SCENES) are held to their regimes and to the
restatement's margins in tests/test_gmm_train_hard_cpu.py."""
import numpy as np


def class_models(rng, n_classes):
    """-> centres [C, 4, 12], square roots of the covariances [C, 4, 12, 12]"""
    centres = np.empty((n_classes, 4, 12))
    roots = np.empty((n_classes, 4, 12, 12))
    for c in range(n_classes):
        offset = rng.normal(0.0, 1.0, 12)
        offset *= 80.0 / np.linalg.norm(offset)
        for k in range(4):
            d = rng.normal(0.0, 1.0, 12)
            centres[c, k] = offset + 40.0 * d / np.linalg.norm(d)
            q, _ = np.linalg.qr(rng.normal(0.0, 1.0, (12, 12)))
            lam = rng.uniform(4.0, 16.0) * 2.0 ** -np.arange(12.0)
            roots[c, k] = q * np.sqrt(lam)
    return centres, roots


def _cluster_models(rng, n_classes, offset_norm, sep, lam):
    """Per class one offset of norm offset_norm, four centres at offset + sep * unit vector, every covariance
    Q diag(lam) Q' with its own random orthogonal Q."""
    centres = np.empty((n_classes, 4, 12))
    roots = np.empty((n_classes, 4, 12, 12))
    for c in range(n_classes):
        offset = rng.normal(0.0, 1.0, 12)
        offset *= offset_norm / np.linalg.norm(offset)
        for k in range(4):
            d = rng.normal(0.0, 1.0, 12)
            centres[c, k] = offset + sep * d / np.linalg.norm(d)
            q, _ = np.linalg.qr(rng.normal(0.0, 1.0, (12, 12)))
            roots[c, k] = q * np.sqrt(lam)
    return centres, roots


def overlapping_models(rng, n_classes, sep, lam_hi, ratio):
    """Clusters that overlap (class_models' sit 40 apart with spreads of at most 4): centres `sep` from a class
    offset of norm 30, eigenvalues lam_hi * ratio**-j.  k-means then moves vectors between clusters over several
    passes (rows carry more than one selection bit), and the E-step's weights are soft."""
    return _cluster_models(rng, n_classes, 30.0, sep, lam_hi * ratio ** -np.arange(12.0))


def wide_models(rng, n_classes, decades, offset, sep):
    """Covariance eigenvalues 100 * 10**(-decades j / 11), j = 0..11, on centres at norm `offset` from the origin: a
    wide spectrum whose small end is far below the square of the data's size."""
    return _cluster_models(rng, n_classes, offset, sep, 100.0 * 10.0 ** (-decades * np.arange(12.0) / 11.0))


# The scenes of tests/test_gmm_train_hard_{cpu,gpu}.py: name -> (models, arguments, seed, classes, files per class,
# shortest and longest file).  One default_rng(seed) draws the models and then the files.
HARD_SCENES = {
    "overlap6": ("overlapping", dict(sep=6.0, lam_hi=9.0, ratio=1.5), 1, 6, 3, 300, 700),
    "overlap3": ("overlapping", dict(sep=3.0, lam_hi=9.0, ratio=1.3), 3, 6, 3, 300, 700),
    "wide60": ("wide", dict(decades=6, offset=1000.0, sep=60.0), 1, 3, 2, 300, 500),
    "wide15": ("wide", dict(decades=6, offset=1000.0, sep=15.0), 2, 3, 2, 300, 500),
}

# file lengths at and around the trainer's 64-frame tiles and 256-frame rounds
TILE_EDGE_LENGTHS = [64, 65, 128, 255, 256, 257, 512, 513, 63, 127, 192, 320, 768, 1024, 100, 64, 256, 512]


def hard_scene(name):
    """-> feats, file_first, file_class, n_classes, models"""
    kind, kw, seed, n_classes, fpc, lo, hi = HARD_SCENES[name]
    rng = np.random.default_rng(seed)
    models = (overlapping_models if kind == "overlapping" else wide_models)(rng, n_classes, **kw)
    feats, ff, fc = make_files(rng, n_classes, fpc, lambda r: r.integers(lo, hi), models=models)
    return feats, ff, fc, n_classes, models


def unreachable_frame(name, cls, row=20):
    """hard_scene(name) with one vector of class cls's second file moved to a cluster centre + 1e4 in every feature:
    every exponent of its densities is below -1e6, so all four are exactly 0 (no denormal in between) and its weights
    are 0/0.  -> feats, file_first, file_class, n_classes"""
    feats, ff, fc, n_classes, (centres, _) = hard_scene(name)
    f = int(np.nonzero(fc == cls)[0][1])
    feats[ff[f] + row] = centres[cls, 0] + 1e4
    return feats, ff, fc, n_classes


def held_out(name, seed, files_per_class=3, lo=100, hi=300):
    """files of hard_scene(name)'s models that the training never saw"""
    n_classes, models = hard_scene(name)[3:]
    return make_files(np.random.default_rng(seed), n_classes, files_per_class, lambda r: r.integers(lo, hi),
                      models=models)


def tile_edge_files(seed):
    """6 separated classes x 3 files whose lengths are TILE_EDGE_LENGTHS, handed out in make_files' shuffled order."""
    rng = np.random.default_rng(seed)
    lengths = iter(TILE_EDGE_LENGTHS)
    return make_files(rng, 6, 3, lambda r: next(lengths))


def many_files(seed):
    """2 separated classes x 150 files of 64..160 vectors: more files than one 256-file window of the trainer."""
    rng = np.random.default_rng(seed)
    return make_files(rng, 2, 150, lambda r: r.integers(64, 161))


def draw_file(rng, centres, roots, n):
    lab = rng.integers(0, 4, n)
    lab[:min(n, 16)] = np.arange(min(n, 16)) // 4
    z = rng.normal(0.0, 1.0, (n, 12))
    return centres[lab] + np.einsum("nij,nj->ni", roots[lab], z)


def make_files(rng, n_classes, files_per_class, lengths, models=None):
    """Files interleaved across classes (a class's files keep their order): feats [N, 12], file_first [F + 1] int64,
    file_class [F] int32.  files_per_class: int or per-class list; lengths: callable (rng) -> int."""
    centres, roots = models if models is not None else class_models(rng, n_classes)
    fpc = [files_per_class] * n_classes if np.isscalar(files_per_class) else list(files_per_class)
    order = np.concatenate([np.full(fpc[c], c) for c in range(n_classes)])
    rng.shuffle(order)
    chunks, first, cls = [], [0], []
    for c in order:
        x = draw_file(rng, centres[c], roots[c], int(lengths(rng)))
        chunks.append(x)
        first.append(first[-1] + len(x))
        cls.append(c)
    return (np.ascontiguousarray(np.concatenate(chunks)), np.asarray(first, np.int64), np.asarray(cls, np.int32))


def bench_files(seed=7, n_classes=25, files_per_class=400):
    """The gmmtrain bench leg's data: the gmm leg's ragged utterance lengths (98..598 vectors, 10,000 of them) as
    25 classes x 400 files, drawn from anisotropic clusters."""
    rng = np.random.default_rng(seed)
    return make_files(rng, n_classes, files_per_class, lambda r: r.integers(98, 599))


def pcm_sources(rng, n_classes):
    """Per class 4 sound sources, each a band of noise (random centre and width) plus a tone: [C][4] dicts."""
    out = []
    for _ in range(n_classes):
        srcs = []
        for _ in range(4):
            lo = rng.uniform(150.0, 6000.0)
            srcs.append(dict(lo=lo, hi=lo * rng.uniform(1.3, 2.5), tone=rng.uniform(100.0, 8000.0),
                             tone_amp=rng.uniform(0.2, 1.5), gain=rng.uniform(600.0, 4000.0)))
        out.append(srcs)
    return out


def pcm_utterance(rng, srcs, n_frames, hop=512, win=1024, fs=44100.0):
    """int16 PCM of n_frames MFCC frames (native framing): runs of 20..60 frames, each from one source (the first
    four runs from sources 0, 1, 2, 3), the source's gain varied per run by up to +-6 dB."""
    n = hop * (n_frames - 1) + win
    x = np.zeros(n)
    t0, k = 0, 0
    while t0 < n:
        src = srcs[k % 4] if k < 4 else srcs[int(rng.integers(0, 4))]
        m = min(hop * int(rng.integers(20, 61)), n - t0)
        spec = np.fft.rfft(rng.normal(0.0, 1.0, m))
        f = np.fft.rfftfreq(m, 1.0 / fs)
        spec[(f < src["lo"]) | (f > src["hi"])] = 0.0
        seg = np.fft.irfft(spec, m)
        seg /= max(np.std(seg), 1e-12)
        seg += src["tone_amp"] * np.sqrt(2.0) * np.sin(2 * np.pi * src["tone"] * np.arange(m) / fs + rng.uniform(0, 6.3))
        x[t0:t0 + m] = seg * src["gain"] * 10 ** (rng.uniform(-0.3, 0.3))
        t0 += m
        k += 1
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)
