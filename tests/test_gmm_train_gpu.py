"""GMM training on the device (jdsp_gmm_train_*) against the numpy restatement of GMMAlgorithm_Train_Auto_ver2.cpp
(tests/gmm_train_ref.py): parity, bit-identical invariance across call cuts and launch geometry, the bench-size run,
the empty-cluster case, errors, and scoring with the trained records."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gmm_train_cases as gtc  # noqa: E402
import gmm_train_ref as gtr  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-9


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ragged():
    """25 classes, 1..8 files each, 120..600 vectors per file, interleaved.  Not from 13: a file must give each of
    the 4 mixtures at least 13 vectors, or its covariance is singular and the discarded eigenvalues are decided by
    rounding, where no 1e-9 parity is defined (the restatement's margins then fail).  Lengths that are not a multiple
    of 64 (partial tiles) are most of these; a 13-vector first file has a test of its own (its k-means)."""
    rng = np.random.default_rng(11)
    feats, ff, fc = gtc.make_files(rng, 25, [1 + (c * 3) % 8 for c in range(25)], lambda r: r.integers(120, 601))
    states, margins = gtr.train(feats, ff, fc, 25)
    ref = gtr.params(states, margins)
    return feats, ff, fc, states, margins, ref


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _check_parity(rec, st, states, margins, ref):
    assert margins.kmeans_gap > 1e-9 and margins.cost_gap > 1e-9 and margins.eig_gap > 1e-3, vars(margins)
    for c, s in enumerate(states):
        assert st[c]["kmeans_passes"] == s.kmeans_passes, c
        assert list(st[c]["selected"]) == list(s.selected), c
        assert st[c]["kmeans_capped"] == 0 and st[c]["status"] == 0 and st[c]["files"] == s.files
        assert abs(st[c]["kmeans_cost"] - s.kmeans_cost) <= REL * abs(s.kmeans_cost), c
    assert _rel(rec["alpa"], ref["alpa"]) <= REL
    lam_d = rec["covariance"][:, :, np.arange(8), np.arange(8)]
    lam_r = ref["covariance"][:, :, np.arange(8), np.arange(8)]
    assert _rel(lam_d, lam_r) <= REL
    # projected means: relative to the vector's size (a component may be near zero)
    scale = np.abs(ref["mean"][:, :, :8]).max(axis=2, keepdims=True)
    assert float(np.max(np.abs(rec["mean"][:, :, :8] - ref["mean"][:, :, :8]) / scale)) <= REL
    assert np.all(rec["mean"][:, :, 8:] == 0.0)
    off = ~np.eye(12, dtype=bool)[:8]
    assert np.all(rec["covariance"][:, :, :8][:, :, off] == 0.0)
    rows = ref["covariance"][:, :, 8:]
    assert float(np.max(np.abs(rec["covariance"][:, :, 8:] - rows)) / np.abs(rows).max()) <= REL
    tol_v = 1e-8 * max(1.0, 1e-2 / margins.eig_gap_in)
    assert float(np.max(np.abs(rec["eigenVector"] - ref["eigenVector"]))) <= tol_v


def test_gmm_train_parity_ragged(eng, ragged):
    feats, ff, fc, states, margins, ref = ragged
    tr = eng.gmm_trainer(25)
    tr.train(feats, ff, fc)
    _check_parity(tr.params(), tr.stats(), states, margins, ref)
    tr.close()


def _trained(eng, feats, ff, fc, cuts=None, threads=256, by_class=False, dev=False, n_classes=25):
    import torch
    tr = eng.gmm_trainer(n_classes)
    tr.set_option("threads_per_class", threads)
    if by_class:
        for c in range(n_classes):
            idx = np.nonzero(fc == c)[0]
            sub = np.concatenate([feats[ff[f]:ff[f + 1]] for f in idx])
            lens = ff[idx + 1] - ff[idx]
            tr.train(sub, np.concatenate([[0], np.cumsum(lens)]), np.full(len(idx), c, np.int32))
    else:
        bounds = [0] + list(cuts or []) + [len(fc)]
        for a, b in zip(bounds[:-1], bounds[1:]):
            x = feats[ff[a]:ff[b]]
            first = ff[a:b + 1] - ff[a]
            if dev:
                tr.train(torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(first).cuda(),
                         torch.from_numpy(fc[a:b].copy()).cuda())
                torch.cuda.synchronize()
            else:
                tr.train(x, first, fc[a:b])
    rec, st = tr.params(), tr.stats()
    tr.close()
    return rec, st


def test_gmm_train_bit_identical_across_cuts_and_geometry(eng, ragged):
    feats, ff, fc = ragged[:3]
    base, bst = _trained(eng, feats, ff, fc)
    for kw in (dict(cuts=[7, 30, 31, 80]), dict(by_class=True), dict(threads=512), dict(threads=1024),
               dict(cuts=[50], dev=True)):
        rec, st = _trained(eng, feats, ff, fc, **kw)
        assert rec.tobytes() == base.tobytes(), kw
        assert st.tobytes() == bst.tobytes(), kw


def test_gmm_train_params_is_a_copy(eng, ragged):
    feats, ff, fc = ragged[:3]
    half = len(fc) // 2
    tr = eng.gmm_trainer(25)
    tr.train(feats[:ff[half]], ff[:half + 1], fc[:half])
    a, b = tr.params(), tr.params()
    assert a.tobytes() == b.tobytes()
    tr.train(feats[ff[half]:], ff[half:] - ff[half], fc[half:])
    once, _ = _trained(eng, feats, ff, fc)
    assert tr.params().tobytes() == once.tobytes()
    tr.reset()
    tr.train(feats, ff, fc)
    assert tr.params().tobytes() == once.tobytes()
    tr.close()


def test_gmm_train_params_dev(eng, ragged):
    import torch
    feats, ff, fc = ragged[:3]
    import jeicyboodsp_amd
    tr = eng.gmm_trainer(25)
    tr.train(feats, ff, fc)
    out = torch.zeros(25 * jeicyboodsp_amd.GMM_TRAIN_PARAM.itemsize, dtype=torch.uint8, device="cuda")
    tr.params(out=out)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == tr.params().tobytes()
    tr.close()


def test_gmm_train_bench_size(eng):
    feats, ff, fc = gtc.bench_files()
    tr = eng.gmm_trainer(25)
    t0 = time.perf_counter()
    tr.train(feats, ff, fc)
    rec, st = tr.params(), tr.stats()
    assert time.perf_counter() - t0 < 60.0
    tr.close()
    states, margins = gtr.train(feats, ff, fc, 25)
    _check_parity(rec, st, states, margins, gtr.params(states, margins))


def _empty_cluster_case():
    """Class 3's first file: vectors 0 and 4 coincide, so the `>=` tie rule gives both to cluster 1 and cluster 0 is
    never selected; every vector is far from the origin, so cluster 0's zeroed mean attracts none later."""
    rng = np.random.default_rng(5)
    feats, ff, fc = gtc.make_files(rng, 6, 2, lambda r: r.integers(150, 300))
    f0 = int(np.nonzero(fc == 3)[0][0])
    feats[ff[f0] + 4] = feats[ff[f0]]
    return feats, ff, fc


def test_gmm_train_empty_cluster_is_nan_and_confined(eng):
    feats, ff, fc = _empty_cluster_case()
    states, _ = gtr.train(feats, ff, fc, 6)
    ref = gtr.params(states)
    assert states[3].selected[0] == 0
    lam = np.arange(8)
    assert np.all(np.isnan(ref[3]["alpa"])) and np.all(np.isnan(ref[3]["covariance"][:, lam, lam]))
    tr = eng.gmm_trainer(6)
    tr.train(feats, ff, fc)
    rec, st = tr.params(), tr.stats()
    tr.close()
    assert st[3]["selected"][0] == 0 and st[3]["kmeans_capped"] == 0
    assert st[3]["kmeans_passes"] == states[3].kmeans_passes
    for name in ("alpa", "mean", "covariance", "eigenVector"):
        assert np.array_equal(np.isnan(rec[3][name]), np.isnan(ref[3][name])), name
    others = [c for c in range(6) if c != 3]
    assert np.all(np.isfinite(rec[others]["covariance"]))
    ref_o = ref[others]
    assert _rel(rec[others]["alpa"], ref_o["alpa"]) <= REL
    lam = np.arange(8)
    assert _rel(rec[others]["covariance"][:, :, lam, lam], ref_o["covariance"][:, :, lam, lam]) <= REL


def test_gmm_train_kmeans_cap(eng, ragged):
    feats, ff, fc = ragged[:3]
    tr = eng.gmm_trainer(25)
    tr.set_option("kmeans_max_passes", 1)
    tr.train(feats, ff, fc)
    rec, st = tr.params(), tr.stats()
    tr.close()
    states, _ = gtr.train(feats, ff, fc, 25, max_passes=1)
    ref = gtr.params(states)
    assert np.all(st["kmeans_passes"] == 1) and np.all(st["kmeans_capped"] == 1)
    assert all(s.kmeans_capped == 1 for s in states)
    # the covariance on exit is taken around the starting means (vectors 0, 4, 8, 12)
    assert np.all(np.isfinite(ref["alpa"]))
    assert _rel(rec["alpa"], ref["alpa"]) <= REL


def test_gmm_train_errors(eng, ragged):
    import jeicyboodsp_amd
    from jeicyboodsp_amd import JdspError
    feats, ff, fc = ragged[:3]
    for n in (0, 1025):
        with pytest.raises(JdspError):
            eng.gmm_trainer(n)
    tr = eng.gmm_trainer(25)
    bad = fc.copy()
    bad[3] = 25
    with pytest.raises(JdspError):
        tr.train(feats, ff, bad)
    with pytest.raises(JdspError):                              # first file of a class < 13 vectors
        tr.train(feats[:12], np.array([0, 12]), np.array([0], np.int32))
    with pytest.raises(JdspError):                              # empty file
        tr.train(feats[:200], np.array([0, 100, 100, 200]), np.array([0, 1, 1], np.int32))
    with pytest.raises(JdspError):                              # decreasing offsets
        tr.train(feats[:200], np.array([0, 150, 100, 200]), np.array([0, 1, 1], np.int32))
    with pytest.raises(JdspError):
        tr.set_option("threads_per_class", 128)
    with pytest.raises(JdspError):
        tr.set_option("kmeans_max_passes", 0)
    with pytest.raises(JdspError):
        tr.set_option("nope", 1)
    assert np.all(tr.stats()["files"] == 0)                     # nothing was trained by the rejected calls
    tr.close()
    assert jeicyboodsp_amd.GMM_TRAIN_PARAM.itemsize == 8096


def test_gmm_train_dev_entry_clamps_and_flags(eng, ragged):
    import torch
    feats, ff, fc = ragged[:3]
    n = int(ff[1])
    x = torch.from_numpy(np.ascontiguousarray(feats[:n])).cuda()
    tr = eng.gmm_trainer(4)
    # file 0: class 3, offsets past both ends (clamped to the whole of file 0 of the fixture); file 1: class 9 (out
    # of range); file 2: empty; file 3: 5 vectors as a first file.  The offsets decrease after file 0 (flagged)
    first = torch.tensor([-7, n + 50, 3, 3, 8], dtype=torch.int64, device="cuda")
    cls = torch.tensor([3, 9, 1, 2], dtype=torch.int32, device="cuda")
    tr.train(x, first, cls)
    st = tr.stats()
    assert st[0]["status"] == 2 | 16 and st[0]["files"] == 0     # out-of-range class; n + 50 -> 3 decreases
    assert st[1]["status"] == 4 and st[1]["files"] == 0
    assert st[2]["status"] == 8 and st[2]["files"] == 0
    assert st[3]["status"] == 1 and st[3]["files"] == 1
    rec = tr.params()
    tr.close()
    # decreasing offsets: flagged in class 0's status (the backwards file is also clamped to empty)
    tr = eng.gmm_trainer(2)
    tr.train(x, torch.tensor([0, 60, 50, 110], dtype=torch.int64, device="cuda"),
             torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda"))
    st2 = tr.stats()
    tr.close()
    assert st2[0]["status"] == 16 and st2[0]["files"] == 2
    assert st2[1]["status"] == 1 | 4 and st2[1]["files"] == 0
    states, _ = gtr.train(feats[:n], np.array([0, n]), np.array([0], np.int32), 1)
    assert _rel(rec[3]["alpa"], gtr.params(states)[0]["alpa"]) <= REL


def test_gmm_train_13_vector_first_file(eng, ragged):
    """The shortest first file the reference can start from (vectors 0, 4, 8, 12: Train:120-124) is accepted and its
    k-means matches the restatement exactly (a single partial tile).  Its EM works on singular 12x12 covariances
    (at most 4 vectors per mixture), where no parity is defined, so only the k-means result is compared."""
    feats, ff, fc = ragged[:3]
    x = np.ascontiguousarray(feats[ff[0]:ff[0] + 13])
    tr = eng.gmm_trainer(1)
    tr.train(x, np.array([0, 13]), np.array([0], np.int32))
    st = tr.stats()[0]
    tr.close()
    margins = gtr.Margins()
    s = gtr.ClassState()
    s.mean = x[[0, 4, 8, 12]].copy()
    gtr.kmeans(x, s, 10000, margins)
    assert margins.kmeans_gap > 1e-9 and margins.cost_gap > 1e-9
    assert st["files"] == 1 and st["status"] == 0
    assert st["kmeans_passes"] == s.kmeans_passes and list(st["selected"]) == list(s.selected)
    assert abs(st["kmeans_cost"] - s.kmeans_cost) <= REL * abs(s.kmeans_cost)


def test_gmm_train_records_score(eng):
    """train -> to_score_params -> jdsp_gmm_score: held-out utterances go to their own class, and the scores equal
    those of the restatement-trained records."""
    import jeicyboodsp_amd
    rng = np.random.default_rng(21)
    models = gtc.class_models(rng, 5)
    feats, ff, fc = gtc.make_files(rng, 5, 3, lambda r: r.integers(200, 400), models=models)
    tr = eng.gmm_trainer(5)
    tr.train(feats, ff, fc)
    dev = jeicyboodsp_amd.to_score_params(tr.params())
    tr.close()
    states, _ = gtr.train(feats, ff, fc, 5)
    ref = gtr.to_score(gtr.params(states))
    held, hf, hc = gtc.make_files(rng, 5, 4, lambda r: r.integers(100, 300), models=models)
    g = eng.gmm(dev)
    s_dev, best = g.score(held, hf)
    g.close()
    g = eng.gmm(ref)
    s_ref, _ = g.score(held, hf)
    g.close()
    assert np.array_equal(best, hc)
    # other classes' densities underflow to 0 on these far-apart clusters: log 0 = -inf on both sides
    fin = np.isfinite(s_ref)
    assert np.array_equal(np.isfinite(s_dev), fin) and np.all(s_dev[~fin] == s_ref[~fin])
    assert fin.sum() >= len(hc) and _rel(s_dev[fin], s_ref[fin]) <= REL


def test_gmmtrain_driver(eng, tmp_path):
    """jdsp_gmmtrain class_lists.txt params.bin (Train:49-172): one 8,096-byte record per class of each group, equal to
    jdsp_gmm_train_params bit for bit."""
    import subprocess
    compat = os.path.join(ROOT, "jeicyboodsp_amd", "compat")
    if not os.path.exists(os.path.join(compat, "jdsp_gmmtrain")):
        subprocess.check_call(["make", "-s", "-C", compat])
    rng = np.random.default_rng(31)
    C = 3
    feats, ff, fc = gtc.make_files(rng, C, [2, 3, 1], lambda r: r.integers(150, 350))
    lists = []
    for c in range(C):
        names = []
        for k, f in enumerate(np.nonzero(fc == c)[0]):
            p = tmp_path / ("c%d_%d.mfc" % (c, k))
            feats[ff[f]:ff[f + 1]].tofile(p)
            names.append(str(p))
        lp = tmp_path / ("class%d.txt" % c)
        lp.write_text("\n".join(names) + "\n")
        lists.append(str(lp))
    (tmp_path / "lists.txt").write_text("\n".join(lists) + "\n")
    env = dict(os.environ, JDSP_NUM_OF_CLASS=str(C))
    subprocess.run([os.path.join(compat, "jdsp_gmmtrain"), str(tmp_path / "lists.txt"), str(tmp_path / "p.bin")],
                   check=True, env=env, stdout=subprocess.DEVNULL, timeout=300)
    got = np.fromfile(tmp_path / "p.bin", gtr.TRAIN_PARAM)
    assert len(got) == C
    # the driver trains the files of class c in list order: the same order as the files of class c here
    tr = eng.gmm_trainer(C)
    tr.train(feats, ff, fc)
    want, st = tr.params(), tr.stats()
    tr.close()
    assert got.tobytes() == want.tobytes()
    states, margins = gtr.train(feats, ff, fc, C)
    _check_parity(got, st, states, margins, gtr.params(states, margins))


def test_gmm_train_pcm_mfcc_train_score_on_device(eng):
    """The recognition path end to end without leaving the device: synthetic PCM for 5 spectrally distinct classes
    (each 4 sources: a noise band plus a tone, gain varied per run) -> jdsp_mfcc_frames_dev (native configuration)
    -> jdsp_gmm_train_files_dev -> to_score_params -> jdsp_gmm_score_dev on held-out utterances.  Real MFCC
    statistics (covariance eigenvalues over about 3.5 decades here) are held to the restatement's margins and then to
    the same parity as the synthetic fixtures; held-out utterances must go to their own class, with scores equal to
    those of the restatement-trained records."""
    import torch
    import jeicyboodsp_amd
    rng = np.random.default_rng(1)
    C = 5
    srcs = gtc.pcm_sources(rng, C)
    m = eng.mfcc()

    def utterances(reps, lo, hi):
        out, cls = [], []
        for _ in range(reps):
            for c in range(C):
                nf = int(rng.integers(lo, hi))
                pcm = gtc.pcm_utterance(rng, srcs[c], nf)
                f = m.frames(torch.from_numpy(pcm).cuda())
                assert f.shape == (nf, 12)
                out.append(f)
                cls.append(c)
        first = np.concatenate([[0], np.cumsum([len(f) for f in out])]).astype(np.int64)
        return torch.cat(out).contiguous(), first, np.asarray(cls, np.int32)

    feats, ff, fc = utterances(3, 250, 400)
    held, hf, hc = utterances(2, 150, 250)
    m.close()
    tr = eng.gmm_trainer(C)
    tr.train(feats, torch.from_numpy(ff).cuda(), torch.from_numpy(fc).cuda())
    rec, st = tr.params(), tr.stats()
    tr.close()
    x = feats.cpu().numpy()
    states, margins = gtr.train(x, ff, fc, C)
    ref = gtr.params(states, margins)
    lam = ref["covariance"][:, :, np.arange(8), np.arange(8)]
    assert lam.max() / lam.min() > 100.0                        # MFCC statistics, not an isotropic toy
    _check_parity(rec, st, states, margins, ref)
    hf_d = torch.from_numpy(hf).cuda()
    scores = []
    for records in (jeicyboodsp_amd.to_score_params(rec), gtr.to_score(ref)):
        g = eng.gmm(records)
        s, best = g.score(held, hf_d)                           # torch tensors: jdsp_gmm_score_dev
        torch.cuda.synchronize()
        scores.append((s.cpu().numpy(), best.cpu().numpy()))
        g.close()
    (s_dev, b_dev), (s_ref, b_ref) = scores
    assert np.all(np.isfinite(s_dev))
    assert np.array_equal(b_dev, hc) and np.array_equal(b_ref, hc)
    assert _rel(s_dev, s_ref) <= REL
