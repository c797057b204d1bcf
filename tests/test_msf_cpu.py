"""hs_msf_edges / hs_msf_cut (host only, no GPU): the spanning-forest rule of include/hsearch.h against the plain Kruskal
of tests/msf_ref.py -- heavy ties, cliques of weight 0, every presentation of one edge list, the merge of forests,
cuts on and just below a merge height, every invalid input, the empty cases."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import capi
from tests import components_ref as cr
from tests import msf_ref as mr


def _random_graph(rng, n, m, values):
    """m random weighted pairs; one weight per UNORDERED pair, drawn from `values` (heavy ties)."""
    ei = rng.integers(0, n, m)
    ej = rng.integers(0, n, m)
    w = {}
    d = np.array([w.setdefault((min(x, y), max(x, y)), float(rng.choice(values))) for x, y in zip(ei, ej)])
    return ei.astype(np.uint32), ej.astype(np.uint32), d


def _check(got, n, ei, ej, d):
    want = mr.msf_from_edges(n, ei, ej, d)
    assert mr.same_tree(got, want)
    assert np.array_equal(got["label"], want["label"]) and got["label"].dtype == np.uint32
    assert got["n_tree_edges"] == len(want["lo"]) == n - got["n_components"]
    assert got["n_components"] == cr.n_components(want["label"])
    assert got["n_graph_edges"] == want["n_graph_edges"]
    assert (got["rounds"], got["resident"]) == (0, 0)
    assert (got["lo"] < got["hi"]).all()
    return want


@pytest.mark.parametrize("n,m,values", [(60, 150, (1.0, 2.0, 2.5)), (300, 500, (0.0, 1.0, 1.5, 7.0)),
                                        (300, 200, (3.0, 3.5, 4.0)), (40, 700, (0.5, 1.0, 2.0))])
def test_random_graphs_with_heavy_ties(n, m, values):
    rng = np.random.default_rng(n + m)
    ei, ej, d = _random_graph(rng, n, m, values)
    want = _check(capi.msf_edges(ei, ej, d, n, want_label=True), n, ei, ej, d)
    assert len(want["lo"]) > 10 and len(np.unique(want["dist"])) <= len(values)


def test_clique_of_weight_zero():
    ei, ej = np.nonzero(~np.eye(5, dtype=bool))
    got = capi.msf_edges(ei, ej, np.zeros(len(ei)), 5, want_label=True)
    assert got["lo"].tolist() == [0, 0, 0, 0] and got["hi"].tolist() == [1, 2, 3, 4]
    assert got["dist"].tolist() == [0.0] * 4 and got["label"].tolist() == [0] * 5
    assert (got["n_tree_edges"], got["n_components"], got["n_graph_edges"]) == (4, 1, 20)


def test_every_presentation_of_one_edge_list():
    rng = np.random.default_rng(3)
    n = 120
    ei, ej, d = _random_graph(rng, n, 400, (1.0, 2.0, 3.0))
    lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
    want = _check(capi.msf_edges(lo, hi, d, n, want_label=True), n, lo, hi, d)                 # once, lo first
    forms = {"reversed": (hi, lo, d),
             "both": (np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([d, d])),
             "repeated": (np.concatenate([ei, ei, ej]), np.concatenate([ej, ej, ei]), np.concatenate([d, d, d])),
             "self pairs": (np.concatenate([ei, np.arange(n)]), np.concatenate([ej, np.arange(n)]),
                            np.concatenate([d, np.full(n, 0.25)]))}
    for what, (x, y, w) in forms.items():
        for seed in range(2):
            p = np.random.default_rng(seed).permutation(len(x))
            got = capi.msf_edges(x[p], y[p], w[p], n, want_label=True)
            assert mr.same_tree(got, want) and np.array_equal(got["label"], want["label"]), what
            assert got["n_graph_edges"] == want["n_graph_edges"], what


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_merge_of_forests_is_the_forest_of_the_whole(seed):
    rng = np.random.default_rng(seed)
    n = 200
    ei, ej, d = _random_graph(rng, n, 900, (1.0, 1.5, 2.0, 4.0))
    whole = capi.msf_edges(ei, ej, d, n, want_label=True)
    part = rng.integers(0, 3, len(ei))
    forests = [capi.msf_edges(ei[part == r], ej[part == r], d[part == r], n) for r in range(3)]
    assert all(0 < f["n_tree_edges"] for f in forests) and sum(f["n_tree_edges"] for f in forests) > whole["n_tree_edges"]
    merged = capi.msf_edges(np.concatenate([f["lo"] for f in forests]), np.concatenate([f["hi"] for f in forests]),
                            np.concatenate([f["dist"] for f in forests]), n, want_label=True)
    assert mr.same_tree(merged, whole) and np.array_equal(merged["label"], whole["label"])
    assert merged["n_components"] == whole["n_components"]


def test_cuts_on_and_just_below_a_merge_height():
    rng = np.random.default_rng(9)
    n = 150
    ei, ej, _ = _random_graph(rng, n, 260, (1.0,))
    w = {}
    d = np.array([w.setdefault((min(x, y), max(x, y)), float(rng.integers(1, 40)) / 7.0) for x, y in zip(ei, ej)])
    tree = capi.msf_edges(ei, ej, d, n, want_label=True)
    heights = np.unique(tree["dist"])
    assert len(heights) >= 10
    radii = [0.0, np.inf, heights[-1] * 2]
    for hgt in heights:
        radii += [hgt, np.nextafter(hgt, -np.inf)]
    prev = None
    for r in sorted(radii):
        got = capi.msf_cut(tree, r)
        want = mr.cut(n, tree["lo"], tree["hi"], tree["dist"], r)
        assert np.array_equal(got["label"], want) and got["n_components"] == cr.n_components(want), r
        # ... which is what the whole graph's edges up to r give, and taking the first edges of the list
        assert np.array_equal(want, cr.labels_from_edges(n, ei[d <= r], ej[d <= r])), r
        k = int((tree["dist"] <= r).sum())
        assert got["n_components"] == n - k
        first_k = dict(lo=tree["lo"][:k], hi=tree["hi"][:k], dist=tree["dist"][:k])
        assert np.array_equal(capi.msf_cut(first_k, np.inf, n=n)["label"], want), r
        assert prev is None or got["n_components"] <= prev
        prev = got["n_components"]
    assert np.array_equal(capi.msf_cut(tree, np.inf)["label"], tree["label"])
    on, below = capi.msf_cut(tree, heights[3]), capi.msf_cut(tree, np.nextafter(heights[3], -np.inf))
    assert on["n_components"] < below["n_components"]


def _raw_edges(ei, ej, d, n, cap, lo, hi, od, label):
    info = capi._MsfInfo(7, 7, 7, 7, 7)
    st = capi.load().hs_msf_edges(capi._vp(ei), capi._vp(ej), capi._vp(d), len(ei), n, capi._vp(lo), capi._vp(hi),
                                  capi._vp(od), cap, capi._vp(label), C.byref(info))
    return st, info


def test_invalid_edge_lists_leave_the_outputs_untouched():
    n = 6
    good = (np.array([0, 1, 2, 1], dtype=np.uint32), np.array([1, 2, 3, 0], dtype=np.uint32), np.array([1.0, 2.0, 0.5, 1.0]))
    bad = {"id >= n": (np.array([0, 6], dtype=np.uint32), np.array([1, 2], dtype=np.uint32), np.array([1.0, 1.0])),
           "id >= n on the j side": (np.array([0, 1], dtype=np.uint32), np.array([1, 7], dtype=np.uint32), np.array([1.0, 1.0])),
           "NaN": (good[0], good[1], np.array([1.0, np.nan, 0.5, 1.0])),
           "negative": (good[0], good[1], np.array([1.0, 2.0, -0.5, 1.0])),
           "NaN on a self pair": (np.array([0, 2], dtype=np.uint32), np.array([1, 2], dtype=np.uint32), np.array([1.0, np.nan])),
           "one pair, two distances": (good[0], good[1], np.array([1.0, 2.0, 0.5, np.nextafter(1.0, 2.0)])),
           "one pair, two distances, same direction": (np.array([0, 3, 0], dtype=np.uint32), np.array([1, 4, 1], dtype=np.uint32),
                                                       np.array([1.0, 1.0, 1.5]))}
    for what, (ei, ej, d) in bad.items():
        lo, hi = np.full(n, 77, dtype=np.uint32), np.full(n, 78, dtype=np.uint32)
        od, label = np.full(n, 7.5), np.full(n, 79, dtype=np.uint32)
        st, info = _raw_edges(ei, ej, d, n, n, lo, hi, od, label)
        assert st == capi.HS_ERR_INVALID, what
        assert (lo == 77).all() and (hi == 78).all() and (od == 7.5).all() and (label == 79).all(), what
        assert (info.n_tree_edges, info.n_components, info.n_graph_edges, info.rounds, info.resident) == (0,) * 5, what
        with pytest.raises(capi.HsError) as e:
            capi.msf_edges(ei, ej, d, n)
        assert e.value.status == capi.HS_ERR_INVALID, what
    assert capi.msf_edges(*good, n)["n_tree_edges"] == 3
    # the capacity pattern: the count, nothing written; then the call with room
    lo, hi, od = np.full(2, 77, dtype=np.uint32), np.full(2, 78, dtype=np.uint32), np.full(2, 7.5)
    label = np.full(n, 79, dtype=np.uint32)
    st, info = _raw_edges(*good, n, 2, lo, hi, od, label)
    assert st == capi.HS_ERR_CAPACITY and info.n_tree_edges == 3 and info.n_components == 3
    assert (lo == 77).all() and (hi == 78).all() and (od == 7.5).all() and (label == 79).all()
    with pytest.raises(capi.HsError) as e:
        capi.msf_edges(*good, n, cap=1)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == 3
    assert capi.msf_edges(*good, n, cap=3)["lo"].tolist() == [2, 0, 1]


def test_invalid_cuts_leave_the_labels_untouched():
    n = 5
    good = dict(lo=[0, 1, 3], hi=[1, 2, 4], dist=[1.0, 2.0, 0.5])
    bad = {"id >= n": dict(lo=[0, 1], hi=[1, 5], dist=[1.0, 1.0]),
           "self pair": dict(lo=[0, 2], hi=[1, 2], dist=[1.0, 1.0]),
           "cycle": dict(lo=[0, 1, 0], hi=[1, 2, 2], dist=[1.0, 1.0, 1.0]),
           "repeated edge": dict(lo=[0, 1, 0], hi=[1, 2, 1], dist=[1.0, 1.0, 1.0]),
           "repeated edge, mirrored": dict(lo=[0, 1], hi=[1, 0], dist=[1.0, 1.0]),
           "NaN distance": dict(lo=[0, 1], hi=[1, 2], dist=[1.0, np.nan])}
    for what, tree in bad.items():
        out = np.full(n, 79, dtype=np.uint32)
        with pytest.raises(capi.HsError) as e:
            capi.msf_cut(tree, 1.0, n=n, out=out)
        assert e.value.status == capi.HS_ERR_INVALID and (out == 79).all(), what
    out = np.full(n, 79, dtype=np.uint32)
    with pytest.raises(capi.HsError) as e:
        capi.msf_cut(good, np.nan, n=n, out=out)
    assert e.value.status == capi.HS_ERR_INVALID and (out == 79).all()
    got = capi.msf_cut(good, 1.0, n=n)
    assert got["label"].tolist() == [0, 0, 2, 3, 3] and got["n_components"] == 3


def test_empty_cases():
    none = np.empty(0, dtype=np.uint32)
    for n in (0, 1, 4):
        got = capi.msf_edges(none, none, np.empty(0), n, want_label=True)
        assert got["n_tree_edges"] == 0 and len(got["lo"]) == len(got["hi"]) == len(got["dist"]) == 0
        assert got["n_components"] == n and got["n_graph_edges"] == 0 and np.array_equal(got["label"], np.arange(n))
        cut = capi.msf_cut(got, 1.0)
        assert np.array_equal(cut["label"], np.arange(n)) and cut["n_components"] == n
    # only self pairs: no edge
    got = capi.msf_edges([0, 1], [0, 1], [1.0, 2.0], 2, want_label=True)
    assert got["n_tree_edges"] == 0 and got["n_components"] == 2 and got["n_graph_edges"] == 0
    with pytest.raises(capi.HsError):
        capi.msf_edges([0], [1], [1.0], 0)                      # any id is >= n = 0
