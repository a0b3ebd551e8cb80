"""The device trainer (jdsp_gmm_train_*) where the separated fixtures of test_gmm_train_gpu.py never take it: k-means
that moves vectors between clusters over many passes (rows that carry several selection bits, a cost summed over every
set bit), a pass cap that strikes in mid-flight, E-step weights that are soft, file lengths at and around the 64-frame
tile and the 256-frame round, more files than one 256-file window in a call, covariance spectra over 3 to 4 kept
decades on data 1000 from the origin, and a frame no mixture reaches.  Every fixture's regime and margins, and the
1e-9 bar's footing on these scenes, are checked on the CPU in test_gmm_train_hard_cpu.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gmm_train_cases as gtc  # noqa: E402
import gmm_train_ref as gtr  # noqa: E402
from test_gmm_train_gpu import REL, _check_parity, _rel, _trained  # noqa: E402

pytestmark = pytest.mark.gpu

I8 = np.arange(8)
_cache = {}


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def _scene(name):
    """-> feats, ff, fc, n_classes, states, margins, ref; the restatement runs once per scene"""
    if name not in _cache:
        if name.startswith("tile"):
            data = gtc.tile_edge_files(int(name[4:])) + (6,)
        elif name.startswith("many"):
            data = gtc.many_files(int(name[4:])) + (2,)
        else:
            data = gtc.hard_scene(name)[:4]
        states, margins = gtr.train(*data)
        _cache[name] = data + (states, margins, gtr.params(states, margins))
    return _cache[name]


def _device(eng, name, **kw):
    """rec, stats of one scene; the plain run (one call, 256 threads) is made once and shared"""
    feats, ff, fc, n_classes = _scene(name)[:4]
    if kw:
        return _trained(eng, feats, ff, fc, n_classes=n_classes, **kw)
    if ("dev", name) not in _cache:
        _cache["dev", name] = _trained(eng, feats, ff, fc, n_classes=n_classes)
    return _cache["dev", name]


def _first_and_later_lengths(ff, fc):
    first, later = {}, []
    for f, c in enumerate(fc):
        n = int(ff[f + 1] - ff[f])
        if int(c) in first:
            later.append(n)
        else:
            first[int(c)] = n
    return first, later


@pytest.mark.parametrize("name", ("overlap6", "overlap3"))
def test_gmm_train_overlapping_parity(eng, name):
    feats, ff, fc, n_classes, states, margins, ref = _scene(name)
    rec, st = _device(eng, name)
    _check_parity(rec, st, states, margins, ref)
    # the device really carried rows with several selection bits (and _check_parity held their count and the cost
    # summed over every set bit to the restatement's)
    first, _ = _first_and_later_lengths(ff, fc)
    for c in range(n_classes):
        assert int(st[c]["selected"].sum()) > first[c], c
    assert int(st["kmeans_passes"].max()) >= 5


def test_gmm_train_overlapping_bit_identical_across_cuts_and_geometry(eng):
    """sel is rewritten over up to 14 passes and wbuf holds soft weights: neither, nor the tile order, may depend on
    how the files arrive or on the workgroup size."""
    base, bst = _device(eng, "overlap3")
    assert int(bst["kmeans_passes"].max()) >= 10
    for kw in (dict(cuts=[1, 5, 6, 13]), dict(by_class=True), dict(threads=512), dict(threads=1024),
               dict(cuts=[9], dev=True)):
        rec, st = _device(eng, "overlap3", **kw)
        assert rec.tobytes() == base.tobytes(), kw
        assert st.tobytes() == bst.tobytes(), kw


def test_gmm_train_kmeans_cap_in_mid_flight(eng):
    """kmeans_max_passes = 4 where every class wants 7 or more: pass 4 takes the exit branch with what the selection
    has accumulated so far."""
    feats, ff, fc, n_classes, full = _scene("overlap3")[:5]
    assert min(s.kmeans_passes for s in full) >= 5
    tr = eng.gmm_trainer(n_classes)
    tr.set_option("kmeans_max_passes", 4)
    tr.train(feats, ff, fc)
    rec, st = tr.params(), tr.stats()
    tr.close()
    states, margins = gtr.train(feats, ff, fc, n_classes, max_passes=4)
    ref = gtr.params(states, margins)
    assert margins.kmeans_gap > 1e-9 and margins.eig_gap > 1e-3, vars(margins)
    assert np.all(st["kmeans_passes"] == 4) and np.all(st["kmeans_capped"] == 1)
    for c, s in enumerate(states):
        assert s.kmeans_passes == 4 and s.kmeans_capped == 1
        assert list(st[c]["selected"]) == list(s.selected), c
        assert abs(st[c]["kmeans_cost"] - s.kmeans_cost) <= REL * abs(s.kmeans_cost), c
    assert np.all(np.isfinite(ref["alpa"]))
    assert _rel(rec["alpa"], ref["alpa"]) <= REL
    assert _rel(rec["covariance"][:, :, I8, I8], ref["covariance"][:, :, I8, I8]) <= REL


TILE_SEEDS = (1, 2, 3)


@pytest.mark.parametrize("seed", TILE_SEEDS)
def test_gmm_train_tile_and_round_edges(eng, seed):
    """Files of exactly one tile (64), one round (256), one frame into a new round (257) and their neighbours, as a
    class's first file (k-means and EM) and as a later one (EM on a carried state)."""
    feats, ff, fc, n_classes, states, margins, ref = _scene("tile%d" % seed)
    rec, st = _device(eng, "tile%d" % seed)
    _check_parity(rec, st, states, margins, ref)


def test_gmm_train_tile_edge_seeds_cover_the_edges():
    first, later = set(), set()
    for seed in TILE_SEEDS:
        feats, ff, fc = gtc.tile_edge_files(seed)
        a, b = _first_and_later_lengths(ff, fc)
        assert sorted(list(a.values()) + b) == sorted(gtc.TILE_EDGE_LENGTHS)
        first |= set(a.values())
        later |= set(b)
        if seed == 2:                                   # one seed alone has the three essential ones on both sides
            assert set(a.values()) >= {64, 256, 257} and set(b) >= {64, 256, 512}
    assert first >= {63, 64, 65, 128, 255, 256, 257, 512, 513}
    assert later >= {63, 64, 100, 127, 128, 192, 256, 257, 320, 512, 513, 768, 1024}


@pytest.mark.parametrize("seed", (1, 2))
def test_gmm_train_more_than_256_files_in_one_call(eng, seed):
    """300 files of 2 classes: the 256-file window loop and the files[] compaction run a second time, on a class
    whose chain continues across the window edge."""
    feats, ff, fc, n_classes, states, margins, ref = _scene("many%d" % seed)
    assert len(fc) == 300 and fc[255] == fc[256]
    rec, st = _device(eng, "many%d" % seed)
    _check_parity(rec, st, states, margins, ref)
    if seed == 1:
        for cuts in ([256], [100, 257]):
            r2, s2 = _device(eng, "many1", cuts=cuts)
            assert r2.tobytes() == rec.tobytes(), cuts
            assert s2.tobytes() == st.tobytes(), cuts


@pytest.mark.parametrize("name", ("wide60", "wide15"))
def test_gmm_train_wide_spectrum_far_from_the_origin(eng, name):
    feats, ff, fc, n_classes, states, margins, ref = _scene(name)
    rec, st = _device(eng, name)
    _check_parity(rec, st, states, margins, ref)
    lam = rec["covariance"][:, :, I8, I8]
    assert float((lam[..., 0] / lam[..., 7]).min()) >= 1e3


def test_gmm_train_unreachable_frame_is_nan_and_confined(eng):
    """One frame of class 2's second file at which all four densities are exactly 0: its weights are 0/0, the class's
    record takes the restatement's NaN pattern, and no other class notices."""
    cls = 2
    feats, ff, fc, n_classes = gtc.unreachable_frame("overlap6", cls)
    states, margins = gtr.train(feats, ff, fc, n_classes)
    ref = gtr.params(states)
    assert margins.zero_density == 1
    assert np.all(np.isnan(ref[cls]["alpa"])) and np.all(np.isnan(ref[cls]["covariance"][:, I8, I8]))
    rec, st = _trained(eng, feats, ff, fc, n_classes=n_classes)
    for field in ("alpa", "mean", "covariance", "eigenVector"):
        assert np.array_equal(np.isnan(rec[cls][field]), np.isnan(ref[cls][field])), field
    assert st[cls]["files"] == states[cls].files and st[cls]["status"] == 0
    assert st[cls]["kmeans_passes"] == states[cls].kmeans_passes
    assert list(st[cls]["selected"]) == list(states[cls].selected)
    base, bst = _device(eng, "overlap6")
    others = [c for c in range(n_classes) if c != cls]
    assert np.all(np.isfinite(rec[others]["covariance"]))
    assert rec[others].tobytes() == base[others].tobytes()
    assert st[others].tobytes() == bst[others].tobytes()


@pytest.mark.parametrize("name", ("overlap6", "overlap3"))
def test_gmm_train_soft_records_score(eng, name):
    """train -> to_score_params -> jdsp_gmm_score on held-out files of the same overlapping models: the scores and the
    decisions equal those of the restatement-trained records.  (That the decision is the true class is not asserted:
    these classes overlap by design.)"""
    import jeicyboodsp_amd
    ref = _scene(name)[6]
    rec, _ = _device(eng, name)
    held, hf, hc = gtc.held_out(name, 77)
    out = []
    for records in (jeicyboodsp_amd.to_score_params(rec), gtr.to_score(ref)):
        g = eng.gmm(records)
        out.append(g.score(held, hf))
        g.close()
    (s_dev, b_dev), (s_ref, b_ref) = out
    fin = np.isfinite(s_ref)
    assert np.array_equal(np.isfinite(s_dev), fin) and np.all(s_dev[~fin] == s_ref[~fin])
    assert fin.sum() >= len(hc) and _rel(s_dev[fin], s_ref[fin]) <= REL
    assert np.array_equal(b_dev, b_ref)
