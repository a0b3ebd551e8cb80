"""CPU tests of the GMM training restatement (tests/gmm_train_ref.py) on hand-checkable cases, the record layouts, and
the host-only conversion jdsp_gmm_param_from_train through ctypes."""
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gmm_train_ref as gtr  # noqa: E402


def _line(values):
    """vectors on the first axis only (the other 11 features zero)"""
    X = np.zeros((len(values), 12))
    X[:, 0] = values
    return X


def _kmeans(X, max_passes=10000):
    st = gtr.ClassState()
    st.mean = X[[0, 4, 8, 12]].copy()
    gtr.kmeans(X, st, max_passes, gtr.Margins())
    return st


def test_selection_accumulates_across_passes():
    # means start at 0, 10, 20, 30.  Pass 1 gives the 6s and vector 13 (= 14.9: 24.01 to 10 against 26.01 to 20) to
    # cluster 1, whose mean then drops to 8.58 = (10 + 6 + 6 + 6 + 14.9) / 5, so pass 2 gives vector 13 to cluster 2 --
    # and it stays counted for cluster 1 too (Train:365 never clears a bit).
    members1 = (10, 6, 6, 6, 14.9)
    X = _line([0, 0, 0, 0, 10, 6, 6, 6, 20, 20, 20, 20, 30, 14.9, 30, 30])
    st = _kmeans(X)
    assert list(st.selected) == [4, 5, 5, 3]
    assert int(st.selected.sum()) == len(X) + 1
    # cluster 1's mean and covariance are over all five vectors it ever held, vector 13 included
    m1 = sum(members1) / 5
    assert abs(st.mean[1, 0] - m1) < 1e-12
    assert abs(st.cov[1][0, 0] - sum((v - m1) ** 2 for v in members1) / 5) < 1e-12
    assert abs(st.mean[2, 0] - (80 + 14.9) / 5) < 1e-12
    assert st.kmeans_passes == 4 and st.kmeans_capped == 0


def test_tie_goes_to_the_last_index():
    # vector 2 (= 5) is exactly between the means 0 and 10: `>=` from j = 0 gives it to cluster 1
    X = _line([0, 0, 5, 0, 10, 10, 10, 10, 100, 100, 100, 100, 200, 200, 200, 200])
    st = gtr.ClassState()
    st.mean = X[[0, 4, 8, 12]].copy()
    gtr.kmeans(X, st, 1, gtr.Margins())
    assert list(st.selected) == [3, 5, 4, 4]
    assert st.kmeans_passes == 1 and st.kmeans_capped == 1


def test_empty_cluster_zero_mean_nan_covariance():
    # vectors 0 and 4 coincide: every vector equal to them goes to cluster 1, cluster 0 is never selected
    X = _line([50, 50, 50, 50, 50, 51, 52, 51, 100, 101, 102, 100, 200, 201, 202, 200])
    st = _kmeans(X)
    assert st.selected[0] == 0
    assert np.all(st.mean[0] == 0.0)
    assert np.all(np.isnan(st.cov[0])) and np.all(np.isfinite(st.cov[1:]))
    lam, E = gtr.sorted_eigen(st.cov[0])
    assert np.all(np.isnan(lam)) and np.all(np.isnan(E))


def test_em_accumulates_onto_the_old_alpa_and_mean():
    rng = np.random.default_rng(3)
    X = rng.normal(0.0, 1.0, (40, 12)) * np.linspace(3.0, 0.5, 12)
    st = gtr.ClassState()
    st.alpa = np.array([0.1, 0.2, 0.3, 0.4])
    st.mean = rng.normal(0.0, 0.3, (4, 12))
    st.cov = np.stack([np.diag(np.linspace(9.0, 0.25, 12) * (1 + 0.1 * k)) for k in range(4)])
    a0, m0, c0 = st.alpa.copy(), st.mean.copy(), st.cov.copy()
    # one E-step by hand (Train:270-284), then the reference's update formulas (Train:289-304)
    P = np.stack([gtr.probability(X, m0[k], *gtr.sorted_eigen(c0[k])) * a0[k] for k in range(4)], axis=1)
    W = P / P.sum(axis=1, keepdims=True)
    nkey = a0 + W.sum(axis=0)
    mean = (m0 + W.T @ X) / nkey[:, None]
    cov0 = ((X - mean[0]) * W[:, :1]).T @ (X - mean[0]) / nkey[0]
    gtr.em(X, st, gtr.Margins(), iterations=1)
    assert np.allclose(st.alpa, nkey / len(X), rtol=1e-13, atol=0)
    assert np.allclose(st.mean, mean, rtol=1e-12, atol=1e-14)
    assert np.allclose(st.cov[0], cov0, rtol=1e-12, atol=1e-14)
    assert not np.allclose(st.alpa, W.sum(axis=0) / len(X))                  # the old alpa is part of it
    assert not np.allclose(st.mean, (W.T @ X) / W.sum(axis=0)[:, None])      # ... and the old mean


def test_pca_keeps_rows_8_to_11():
    rng = np.random.default_rng(4)
    st = gtr.ClassState()
    st.alpa = np.full(4, 0.25)
    st.mean = rng.normal(0.0, 1.0, (4, 12))
    for k in range(4):
        q, _ = np.linalg.qr(rng.normal(0.0, 1.0, (12, 12)))
        st.cov[k] = (q * (2.0 * 1.25 ** -np.arange(12.0))) @ q.T
    rec = gtr.params([st])[0]
    for k in range(4):
        lam, E = gtr.sorted_eigen(st.cov[k])
        assert np.all(np.diff(lam) < 0)
        assert np.array_equal(rec["covariance"][k][8:], st.cov[k][8:])
        assert np.array_equal(rec["covariance"][k][:8], np.pad(np.diag(lam), ((0, 0), (0, 4))))
        assert np.allclose(rec["mean"][k][:8], st.mean[k] @ E) and np.all(rec["mean"][k][8:] == 0)
        big = np.argmax(np.abs(E), axis=0)
        assert np.all(E[big, np.arange(8)] > 0)                    # canonical sign
        assert np.allclose(E.T @ E, np.eye(8), atol=1e-12)


def test_record_sizes_and_offsets():
    import jeicyboodsp_amd as j
    assert j.GMM_TRAIN_PARAM.itemsize == 8096 == gtr.TRAIN_PARAM.itemsize
    assert j.GMM_PARAM.itemsize == 6560
    assert [j.GMM_TRAIN_PARAM.fields[n][1] for n in ("alpa", "mean", "covariance", "eigenVector")] == [0, 32, 416, 5024]
    assert j.GMM_TRAIN_STATS.itemsize == 40
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    assert "double eigenVector[4][12][8];" in txt


def test_param_from_train_through_ctypes():
    import jeicyboodsp_amd as j
    rng = np.random.default_rng(9)
    rec = np.zeros(3, j.GMM_TRAIN_PARAM)
    for name in ("alpa", "mean", "covariance", "eigenVector"):
        rec[name] = rng.normal(0.0, 1.0, rec[name].shape)
    out = j.to_score_params(rec)
    assert out.dtype == j.GMM_PARAM
    for name in ("alpa", "mean", "covariance"):
        assert np.array_equal(out[name], rec[name])
    assert np.array_equal(out["eigenVector"], rec["eigenVector"][..., :4])
    assert out.tobytes() == gtr.to_score(rec).tobytes()
    from jeicyboodsp_amd._lib import lib
    assert lib.jdsp_gmm_param_from_train(None, -1, None) != 0
    assert lib.jdsp_gmm_param_from_train(None, 0, None) == 0
    assert C.sizeof(C.c_double) * 1012 == 8096


def test_header_gmm_train_entries_are_bound():
    txt = open(os.path.join(ROOT, "include", "jdsp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(jdsp_gmm_(?:train_[a-z_]+|param_from_train))\s*\(", txt)))
    assert len(names) == 10
    src = open(os.path.join(ROOT, "jeicyboodsp_amd", "_lib.py")).read()
    assert not [n for n in names if '"%s"' % n not in src]
