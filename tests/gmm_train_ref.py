"""FP64 numpy restatement of GMMAlgorithm_Train_Auto_ver2.cpp's training (cited as Train:<line>), the yardstick of the
device trainer (jdsp_gmm_train_*).

It cannot be pinned to compiled reference code: the reference needs Eigen (and Windows' <conio.h>), which no machine
this project runs on has.  Eigen's EigenSolver is therefore replaced by numpy.linalg.eigh, followed by the reference's
own rank rule (Train:218-238) and the canonical eigenvector sign the device uses (largest-magnitude component of each
kept column positive, first index on ties).  It lives under tests/ because oracle/ is frozen.

Besides the records it reports, for fixture hygiene, how close the data came to flipping a discrete decision:
  kmeans_gap  smallest relative gap between the best and the second-best k-means distance, over all passes
  cost_gap    smallest | |cost - cost_before| - 1.0 | of the k-means loop test (Train:379)
  eig_gap     smallest relative gap between eigenvalues 8 and 9 of every decomposition (it decides the kept subspace)
  eig_gap_in  smallest relative gap between adjacent eigenvalues among the top 8 (it decides how well eigenvectors
              compare; the parity tests scale their eigenvector tolerance by its inverse)
and which regime the data reached (a fixture built to reach a regime asserts these):
  passes_min, passes_max  fewest and most k-means passes of any class
  multi_bit_rows          per k-means run, in the order run: rows that end with more than one selection bit (also kept
                          in the class's state)
  soft_min                smallest per-file fraction of E-step rows (the three iterations together) whose largest
                          weight is below 1 - 1e-6
  zero_density            frames whose four weighted densities sum to exactly 0 (their weights are 0/0)

train(), em(), params() and sorted_eigen() take eigh=: another symmetric eigen-solver with numpy.linalg.eigh's
interface (ascending eigenvalues, eigenvectors in columns), for measuring how much the records depend on the solver.
"""
import numpy as np

FEATURE_LEN, NUM_OF_MIXTURE, PCA_LEN = 12, 4, 8        # Train:20-23
PI = 3.141592                                          # Train:21
THRESHOLD_OF_DISTANCE = 1.0                            # Train:25

# Train:27-32 with PCA_LEN 8 (8,096 bytes) -- the same layout as jeicyboodsp_amd.GMM_TRAIN_PARAM
TRAIN_PARAM = np.dtype([("alpa", "<f8", (4,)), ("mean", "<f8", (4, 12)), ("covariance", "<f8", (4, 12, 12)),
                        ("eigenVector", "<f8", (4, 12, 8))])


class Margins:
    def __init__(self):
        self.kmeans_gap = np.inf
        self.cost_gap = np.inf
        self.eig_gap = np.inf
        self.eig_gap_in = np.inf
        self.passes_min = np.inf
        self.passes_max = 0
        self.multi_bit_rows = []
        self.soft_min = np.inf
        self.zero_density = 0


class ClassState:
    """What main() keeps in rgGmmParameter[i] between files (Train:104), plus the k-means stats."""

    def __init__(self):
        self.seen = False
        self.alpa = np.zeros(4)
        self.mean = np.zeros((4, 12))
        self.cov = np.zeros((4, 12, 12))
        self.kmeans_passes = 0
        self.kmeans_capped = 0
        self.selected = np.zeros(4, np.int64)
        self.kmeans_cost = 0.0
        self.files = 0
        self.multi_bit_rows = 0


def sorted_eigen(cov, margins=None, eigh=None):
    """Train:214-238 (= :483-506): the top PCA_LEN eigenpairs, ranked by the number of strictly larger eigenvalues;
    a rank nobody has keeps the previous pick.  A matrix with a non-finite entry gives NaN eigenpairs."""
    if not np.all(np.isfinite(cov)):
        return np.full(PCA_LEN, np.nan), np.full((FEATURE_LEN, PCA_LEN), np.nan)
    lam, vec = (eigh or np.linalg.eigh)(cov)
    rank = [int((lam[j] < lam).sum()) for j in range(FEATURE_LEN)]          # Train:218-224
    arg, picks = 0, []
    for j in range(PCA_LEN):                                                # Train:226-238
        for m in range(FEATURE_LEN):
            if rank[m] == j:
                arg = m
                break
        picks.append(arg)
    E = vec[:, picks].copy()
    for j in range(PCA_LEN):                                                # canonical sign
        big = int(np.argmax(np.abs(E[:, j])))
        if E[big, j] < 0:
            E[:, j] = -E[:, j]
    if margins is not None:
        top = np.sort(lam)[::-1][:PCA_LEN + 1]
        gaps = (top[:-1] - top[1:]) / np.maximum(np.abs(top[:-1]), 1e-300)
        margins.eig_gap = min(margins.eig_gap, float(gaps[-1]))
        margins.eig_gap_in = min(margins.eig_gap_in, float(gaps[:-1].min()))
    return lam[picks].copy(), E


def probability(X, mean, lam, E):
    """probability() (Train:189-253) of every row of X, the decomposition hoisted out."""
    y = X @ E                                                               # Train:245
    m = mean @ E                                                            # Train:246
    p = np.ones(len(X))
    for i in range(PCA_LEN):                                                # Train:248-250
        d = y[:, i] - m[i]
        p = p * ((1.0 / np.sqrt(2.0 * PI)) * (1.0 / np.sqrt(lam[i])) * np.exp(((-1 / 2.0) * (d * d)) / lam[i]))
    return p


def distances(X, mean):
    """DistanceToCenter (Train:440-447) of every row against the four means, features added in order."""
    D = np.zeros((len(X), NUM_OF_MIXTURE))
    for j in range(NUM_OF_MIXTURE):
        for i in range(FEATURE_LEN):
            t = X[:, i] - mean[j, i]
            D[:, j] = D[:, j] + t * t
    return D


def kmeans(X, st, max_passes, margins):
    """KmeansAlogorithm (Train:342-438), quirks kept.  Pass number max_passes takes the exit branch whatever the cost
    did (the device's "kmeans_max_passes"; the reference has no cap)."""
    n = len(X)
    sel = np.zeros((n, NUM_OF_MIXTURE), bool)                               # Train:351-352, never cleared
    cost_before, count = 0.0, 0
    rows = np.arange(n)
    while True:
        count += 1
        D = distances(X, st.mean)
        best, arg = D[:, 0].copy(), np.zeros(n, np.int64)
        for j in range(NUM_OF_MIXTURE):                                     # Train:358-364: `>=`, last index wins ties
            take = best >= D[:, j]
            arg[take] = j
            best[take] = D[take, j]
        Ds = np.sort(D, axis=1)
        gap = (Ds[:, 1] - Ds[:, 0]) / np.maximum(Ds[:, 1], 1e-300)
        margins.kmeans_gap = min(margins.kmeans_gap, float(gap.min()))
        sel[rows, arg] = True                                               # Train:365
        cost = float(np.where(sel, D, 0.0).sum())                           # Train:370-376
        if count > 1:
            margins.cost_gap = min(margins.cost_gap, abs(abs(cost - cost_before) - THRESHOLD_OF_DISTANCE))
        go_on = count == 1 or abs(cost - cost_before) >= THRESHOLD_OF_DISTANCE   # Train:379
        if go_on and count < max_passes:
            cost_before = cost
            mean = np.zeros((NUM_OF_MIXTURE, FEATURE_LEN))                  # Train:414-434
            for j in range(NUM_OF_MIXTURE):
                c = int(sel[:, j].sum())
                if c:
                    mean[j] = X[sel[:, j]].sum(axis=0) / c
            st.mean = mean
            continue
        cnt = sel.sum(axis=0)                                               # Train:385-410
        with np.errstate(invalid="ignore", divide="ignore"):
            for j in range(NUM_OF_MIXTURE):
                d = X[sel[:, j]] - st.mean[j]
                st.cov[j] = (d.T @ d) / float(cnt[j])
        st.kmeans_passes, st.kmeans_capped, st.selected, st.kmeans_cost = count, int(go_on), cnt.astype(np.int64), cost
        st.multi_bit_rows = int((sel.sum(axis=1) > 1).sum())
        margins.passes_min, margins.passes_max = min(margins.passes_min, count), max(margins.passes_max, count)
        margins.multi_bit_rows.append(st.multi_bit_rows)
        return


def em(X, st, margins, iterations=3, eigh=None):
    """EmAlgorithmBasedGmmParameter (Train:255-340): three iterations (Train:333); the print-only log-likelihood pass
    (Train:326-332) is not computed."""
    n = len(X)
    soft = 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _ in range(iterations):
            P = np.empty((n, NUM_OF_MIXTURE))
            for k in range(NUM_OF_MIXTURE):                                 # Train:270-276
                lam, E = sorted_eigen(st.cov[k], margins, eigh)
                P[:, k] = probability(X, st.mean[k], lam, E) * st.alpa[k]
            s = P[:, 0] + P[:, 1] + P[:, 2] + P[:, 3]
            W = P / s[:, None]                                              # Train:277-280
            soft += int((W.max(axis=1) < 1.0 - 1e-6).sum())
            margins.zero_density += int((s == 0.0).sum())
            nkey = st.alpa + W.sum(axis=0)                                  # Train:289-293
            st.alpa = nkey / n                                              # Train:294
            st.mean = (st.mean + W.T @ X) / nkey[:, None]                   # Train:297-304
            for k in range(NUM_OF_MIXTURE):                                 # Train:305-325
                d = X - st.mean[k]
                st.cov[k] = ((d * W[:, k:k + 1]).T @ d) / nkey[k]
    if iterations:
        margins.soft_min = min(margins.soft_min, soft / float(iterations * n))


def train(feats, file_first, file_class, n_classes, states=None, max_passes=10000, margins=None, eigh=None):
    """main()'s file loop (Train:87-146) for files in order; `states` carries on from earlier calls."""
    states = states if states is not None else [ClassState() for _ in range(n_classes)]
    margins = margins if margins is not None else Margins()
    for f in range(len(file_class)):
        st = states[int(file_class[f])]
        X = np.asarray(feats[file_first[f]:file_first[f + 1]], np.float64)
        if len(X) == 0:
            raise ValueError("empty file")
        if not st.seen:
            if len(X) < 13:
                raise ValueError("a class's first file needs >= 13 vectors")
            st.mean = X[[0, 4, 8, 12]].copy()                               # Train:120-124
            kmeans(X, st, max_passes, margins)                              # Train:127
            st.alpa = np.full(NUM_OF_MIXTURE, 1.0 / NUM_OF_MIXTURE)         # Train:129-131
            st.seen = True
        em(X, st, margins, eigh=eigh)                                       # Train:138
        st.files += 1
    return states, margins


def params(states, margins=None, eigh=None):
    """PCADiagonalizeCovarianceMatrix (Train:456-518) of each state -> TRAIN_PARAM records (the states unchanged)."""
    out = np.zeros(len(states), TRAIN_PARAM)
    for c, st in enumerate(states):
        out[c]["alpa"] = st.alpa
        for k in range(NUM_OF_MIXTURE):
            lam, E = sorted_eigen(st.cov[k], margins, eigh)
            mean = np.zeros(FEATURE_LEN)
            mean[:PCA_LEN] = st.mean[k] @ E                                 # Train:508-511
            cov = st.cov[k].copy()
            cov[:PCA_LEN] = 0.0                                             # Train:512-513
            cov[np.arange(PCA_LEN), np.arange(PCA_LEN)] = lam
            out[c]["mean"][k] = mean
            out[c]["covariance"][k] = cov
            out[c]["eigenVector"][k] = E                                    # Train:514-516
    return out


def to_score(records):
    """The first four eigenvector columns, as GMMAlgorithm_Test_Auto_ver2.cpp:216-235 reads them."""
    dt = np.dtype([("alpa", "<f8", (4,)), ("mean", "<f8", (4, 12)), ("covariance", "<f8", (4, 12, 12)),
                   ("eigenVector", "<f8", (4, 12, 4))])
    out = np.zeros(len(records), dt)
    for name in ("alpa", "mean", "covariance"):
        out[name] = records[name]
    out["eigenVector"] = records["eigenVector"][..., :4]
    return out
