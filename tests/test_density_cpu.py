"""hs_density_tree_edges / hs_density_tree_cut (host only, no GPU): the density-tree rule of include/hsearch.h against
tests/density_ref.py on random weighted graphs -- heavy ties, cliques of weight 0, every presentation of one edge list,
min_pts = 1 against hs_msf_edges, cuts on and around edge weights and core distances against hs_dbscan_edges, every
invalid input, the empty cases -- and the new exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hsearch_amd
from hsearch_amd import capi
from tests import density_ref as dr
from tests import msf_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NEW = ["hs_core_distance", "hs_core_distance_dev", "hs_density_tree", "hs_density_tree_dev", "hs_density_tree_edges",
        "hs_density_tree_cut"]
_MIN_PTS = (1, 2, 3, 5, 8)


def _random_graph(rng, n, m, values):
    """m random weighted pairs; one weight per UNORDERED pair, drawn from `values` (heavy ties)."""
    ei = rng.integers(0, n, m)
    ej = rng.integers(0, n, m)
    w = {}
    d = np.array([w.setdefault((min(x, y), max(x, y)), float(rng.choice(values))) for x, y in zip(ei, ej)])
    return ei.astype(np.uint32), ej.astype(np.uint32), d


def _check(got, n, ei, ej, d, min_pts):
    want = dr.tree_from_edges(n, ei, ej, d, min_pts)
    assert dr.same_result(got, want)
    assert (got["rounds"], got["resident"], got["self_joins"]) == (0, 0, 0)
    assert (got["lo"] < got["hi"]).all()
    return want


def test_library_exports_the_density_symbols():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    declared = re.findall(r"HS_API\s+[\w\s\*]+?\b(hs_\w+)\s*\(", header)
    lib = hsearch_amd.load()
    for name in _NEW:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(capi._DensityInfo) == 48


@pytest.mark.parametrize("n,m,values", [(60, 150, (1.0, 2.0, 2.5)), (300, 900, (0.0, 1.0, 1.5, 7.0)),
                                        (300, 200, (3.0, 3.5, 4.0)), (40, 700, (0.5, 1.0, 2.0))])
def test_random_graphs_with_heavy_ties(n, m, values):
    rng = np.random.default_rng(n + m)
    ei, ej, d = _random_graph(rng, n, m, values)
    sizes = set()
    for min_pts in _MIN_PTS:
        want = _check(capi.density_tree_edges(ei, ej, d, n, min_pts), n, ei, ej, d, min_pts)
        assert len(np.unique(want["w"])) <= len(values)
        sizes.add((want["n_core"], len(want["lo"])))
    assert max(s[1] for s in sizes) > 10
    assert len(sizes) >= 3 or m > 2 * n          # min_pts shows (where the mean degree is below the largest min_pts)


def test_cliques_of_weight_zero_count_with_multiplicity():
    # a 5-clique of weight 0 (vertices 0..4) hanging on vertex 5 at distance 2, a 3-clique of weight 0 (6..8)
    ei, ej = np.nonzero(np.triu(np.ones((5, 5), dtype=bool), 1))
    ei, ej, d = list(ei), list(ej), [0.0] * len(ei)
    for x, y, w in ((0, 5, 2.0), (1, 5, 2.0), (6, 7, 0.0), (6, 8, 0.0), (7, 8, 0.0), (8, 5, 3.0)):
        ei.append(x), ej.append(y), d.append(w)
    n = 9
    for min_pts, core0, core2, core6 in ((2, 0.0, 0.0, 0.0), (3, 0.0, 0.0, 0.0), (4, 0.0, 0.0, np.inf),
                                         (5, 0.0, 0.0, np.inf), (6, 2.0, np.inf, np.inf)):
        got = capi.density_tree_edges(ei, ej, d, n, min_pts)
        _check(got, n, ei, ej, d, min_pts)
        assert (got["core"][0], got["core"][2], got["core"][6]) == (core0, core2, core6), min_pts
    got = capi.density_tree_edges(ei, ej, d, n, 3)
    assert got["core"].tolist() == [0.0] * 5 + [2.0] + [0.0, 0.0, 0.0]      # 8 has {0, 0, 3}: the second smallest is 0
    assert got["lo"].tolist()[:4] == [0, 0, 0, 0] and got["w"].tolist()[:4] == [0.0] * 4
    assert (got["n_core"], got["n_clusters"], got["n_tree_edges"]) == (9, 1, 8)


def test_every_presentation_of_one_edge_list():
    rng = np.random.default_rng(3)
    n = 120
    ei, ej, d = _random_graph(rng, n, 400, (1.0, 2.0, 3.0))
    lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
    for min_pts in (1, 3, 5):
        want = _check(capi.density_tree_edges(lo, hi, d, n, min_pts), n, lo, hi, d, min_pts)
        forms = {"reversed": (hi, lo, d),
                 "both": (np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([d, d])),
                 "repeated": (np.concatenate([ei, ei, ej]), np.concatenate([ej, ej, ei]), np.concatenate([d, d, d])),
                 "self pairs": (np.concatenate([ei, np.arange(n)]), np.concatenate([ej, np.arange(n)]),
                                np.concatenate([d, np.full(n, 0.25)]))}
        for what, (x, y, w) in forms.items():
            p = np.random.default_rng(7).permutation(len(x))
            assert dr.same_result(capi.density_tree_edges(x[p], y[p], w[p], n, min_pts), want), (what, min_pts)


@pytest.mark.parametrize("seed", [0, 1])
def test_min_pts_one_is_the_spanning_forest(seed):
    rng = np.random.default_rng(seed)
    n = 200
    ei, ej, d = _random_graph(rng, n, 500, (0.0, 1.0, 1.5, 2.0, 4.0))
    got = capi.density_tree_edges(ei, ej, d, n, 1)
    msf = capi.msf_edges(ei, ej, d, n, want_label=True)
    assert mr.same_tree(dict(lo=got["lo"], hi=got["hi"], dist=got["w"]), msf)
    assert np.array_equal(got["label"], msf["label"]) and (got["core"].view(np.uint64) == 0).all()
    assert (got["n_core"], got["n_clusters"], got["n_graph_edges"]) == (n, msf["n_components"], msf["n_graph_edges"])


@pytest.mark.parametrize("min_pts", [2, 3, 5])
def test_cut_ladder_against_dbscan(min_pts):
    rng = np.random.default_rng(9 + min_pts)
    n = 150
    ei, ej, _ = _random_graph(rng, n, 420, (1.0,))
    w = {}
    d = np.array([w.setdefault((min(x, y), max(x, y)), float(rng.integers(1, 40)) / 7.0) for x, y in zip(ei, ej)])
    tree = capi.density_tree_edges(ei, ej, d, n, min_pts)
    finite = tree["core"][np.isfinite(tree["core"])]
    marks = np.unique(np.concatenate([tree["w"], finite, d]))          # values that ARE weights and core distances
    assert len(marks) >= 10 and np.isin(finite, d).all()
    radii = [0.0, np.inf, marks[-1] * 2]
    for v in marks:
        radii += [v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)]
    n_clusters = set()
    for r in sorted(radii):
        got = capi.density_tree_cut(tree, r)
        want = dr.cut(n, tree["lo"], tree["hi"], tree["w"], tree["core"], r)
        assert np.array_equal(got["label"], want), r
        keep = d <= r
        db = capi.dbscan_edges(ei[keep], ej[keep], n, min_pts, want_degree=True)
        is_core = db["degree"].astype(np.int64) + 1 >= min_pts
        assert np.array_equal(is_core, (tree["core"] <= r) & np.isfinite(tree["core"])), r
        assert np.array_equal(got["label"][is_core], db["label"][is_core]), r
        assert (got["label"][~is_core] == capi.NOISE).all(), r
        assert got["n_clusters"] == db["n_clusters"] == len(np.unique(got["label"][is_core])), r
        n_clusters.add(got["n_clusters"])
    assert len(n_clusters) >= 4
    assert np.array_equal(capi.density_tree_cut(tree, np.inf)["label"], tree["label"])


def _raw_edges(ei, ej, d, n, min_pts, cap, lo, hi, w, label, core):
    info = capi._DensityInfo(7, 7, 7, 7, 7, 7, 7)
    st = capi.load().hs_density_tree_edges(capi._vp(ei), capi._vp(ej), capi._vp(d), len(ei), n, min_pts, capi._vp(lo),
                                           capi._vp(hi), capi._vp(w), cap, capi._vp(label), capi._vp(core),
                                           C.byref(info))
    return st, info


def _info_tuple(info):
    return tuple(getattr(info, f[0]) for f in capi._DensityInfo._fields_)


def test_invalid_edge_lists_leave_the_outputs_untouched():
    n = 6
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    good = (u32(0, 1, 2, 1), u32(1, 2, 3, 0), np.array([1.0, 2.0, 0.5, 1.0]))
    bad = {"id >= n": (u32(0, 6), u32(1, 2), np.array([1.0, 1.0]), 2),
           "id >= n on the j side": (u32(0, 1), u32(1, 7), np.array([1.0, 1.0]), 2),
           "NaN": (good[0], good[1], np.array([1.0, np.nan, 0.5, 1.0]), 2),
           "negative": (good[0], good[1], np.array([1.0, 2.0, -0.5, 1.0]), 2),
           "NaN on a self pair": (u32(0, 2), u32(1, 2), np.array([1.0, np.nan]), 2),
           "one pair, two distances": (good[0], good[1], np.array([1.0, 2.0, 0.5, np.nextafter(1.0, 2.0)]), 2),
           "one pair, two distances, same direction": (u32(0, 3, 0), u32(1, 4, 1), np.array([1.0, 1.0, 1.5]), 2),
           "min_pts = 0": (*good, 0)}
    for what, (ei, ej, d, min_pts) in bad.items():
        lo, hi = np.full(n, 77, dtype=np.uint32), np.full(n, 78, dtype=np.uint32)
        w, label, core = np.full(n, 7.5), np.full(n, 79, dtype=np.uint32), np.full(n, 8.5)
        st, info = _raw_edges(ei, ej, d, n, min_pts, n, lo, hi, w, label, core)
        assert st == capi.HS_ERR_INVALID, what
        assert (lo == 77).all() and (hi == 78).all() and (w == 7.5).all() and (label == 79).all(), what
        assert (core == 8.5).all() and _info_tuple(info) == (0,) * 7, what
        with pytest.raises(capi.HsError) as e:
            capi.density_tree_edges(ei, ej, d, n, min_pts)
        assert e.value.status == capi.HS_ERR_INVALID, what
    assert capi.density_tree_edges(*good, n, 2)["n_tree_edges"] == 3
    # the capacity pattern: the counts, nothing written; then the call with room
    lo, hi, w = np.full(2, 77, dtype=np.uint32), np.full(2, 78, dtype=np.uint32), np.full(2, 7.5)
    label, core = np.full(n, 79, dtype=np.uint32), np.full(n, 8.5)
    st, info = _raw_edges(*good, n, 2, 2, lo, hi, w, label, core)
    assert st == capi.HS_ERR_CAPACITY and _info_tuple(info) == (3, 1, 4, 6, 0, 0, 0)
    assert (lo == 77).all() and (hi == 78).all() and (w == 7.5).all() and (label == 79).all() and (core == 8.5).all()
    with pytest.raises(capi.HsError) as e:
        capi.density_tree_edges(*good, n, 2, cap=1)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == 3
    got = capi.density_tree_edges(*good, n, 2, cap=3)
    assert got["lo"].tolist() == [2, 0, 1] and got["w"].tolist() == [0.5, 1.0, 2.0]
    assert got["core"].tolist() == [1.0, 1.0, 0.5, 0.5, np.inf, np.inf]
    assert got["label"].tolist() == [0, 0, 0, 0, capi.NOISE, capi.NOISE]


def test_invalid_cuts_leave_the_labels_untouched():
    n = 5
    core = [1.0, 1.0, 2.0, 0.5, 0.5]
    good = dict(lo=[0, 1, 3], hi=[1, 2, 4], w=[1.0, 2.0, 0.5], core=core)
    bad = {"id >= n": dict(lo=[0, 1], hi=[1, 5], w=[1.0, 2.0], core=core),
           "self pair": dict(lo=[0, 2], hi=[1, 2], w=[1.0, 2.0], core=core),
           "cycle": dict(lo=[0, 1, 0], hi=[1, 2, 2], w=[2.0, 2.0, 2.0], core=core),
           "repeated edge": dict(lo=[0, 1, 0], hi=[1, 2, 1], w=[2.0, 2.0, 2.0], core=core),
           "repeated edge, mirrored": dict(lo=[0, 1], hi=[1, 0], w=[1.0, 1.0], core=core),
           "NaN weight": dict(lo=[0, 1], hi=[1, 2], w=[1.0, np.nan], core=core),
           "NaN core": dict(good, core=[1.0, np.nan, 2.0, 0.5, 0.5]),
           "negative core": dict(good, core=[1.0, 1.0, 2.0, -0.5, 0.5]),
           "weight below the lo end's core": dict(good, core=[1.0, 1.0, 2.0, 0.75, 0.5]),
           "weight below the hi end's core": dict(good, w=[1.0, np.nextafter(2.0, 0.0), 0.5]),
           "edge at a k-mer without a core distance": dict(good, core=[1.0, 1.0, np.inf, 0.5, 0.5])}
    for what, tree in bad.items():
        out = np.full(n, 79, dtype=np.uint32)
        with pytest.raises(capi.HsError) as e:
            capi.density_tree_cut(tree, 1.0, out=out)
        assert e.value.status == capi.HS_ERR_INVALID and (out == 79).all(), what
    out = np.full(n, 79, dtype=np.uint32)
    with pytest.raises(capi.HsError) as e:
        capi.density_tree_cut(good, np.nan, out=out)
    assert e.value.status == capi.HS_ERR_INVALID and (out == 79).all()
    got = capi.density_tree_cut(good, 1.0)
    assert got["label"].tolist() == [0, 0, capi.NOISE, 3, 3] and got["n_clusters"] == 2
    got = capi.density_tree_cut(dict(good, core=[1.0, 1.0, 2.0, 0.5, np.inf], lo=[0, 1], hi=[1, 2], w=[1.0, 2.0]), 9.0)
    assert got["label"].tolist() == [0, 0, 0, 3, capi.NOISE] and got["n_clusters"] == 2


def test_empty_cases():
    none = np.empty(0, dtype=np.uint32)
    for n in (0, 1, 4):
        for min_pts in (1, 2):
            got = capi.density_tree_edges(none, none, np.empty(0), n, min_pts)
            assert got["n_tree_edges"] == 0 and len(got["lo"]) == len(got["hi"]) == len(got["w"]) == 0
            core = min_pts == 1
            assert got["n_core"] == got["n_clusters"] == (n if core else 0) and got["n_graph_edges"] == 0
            assert np.array_equal(got["label"], np.arange(n) if core else np.full(n, capi.NOISE))
            assert np.array_equal(got["core"], np.zeros(n) if core else np.full(n, np.inf))
            cut = capi.density_tree_cut(got, 1.0)
            assert np.array_equal(cut["label"], got["label"]) and cut["n_clusters"] == got["n_clusters"]
    got = capi.density_tree_edges([0, 1], [0, 1], [1.0, 2.0], 2, 2)           # only self pairs: no edge
    assert got["n_tree_edges"] == 0 and got["n_core"] == 0 and got["n_graph_edges"] == 0
    with pytest.raises(capi.HsError):
        capi.density_tree_edges([0], [1], [1.0], 0, 2)                        # any id is >= n = 0
