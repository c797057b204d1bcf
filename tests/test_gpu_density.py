"""hs_core_distance / hs_density_tree on the GPU: core distances settled by threshold rounds per batch and the
mutual-reachability spanning forest by Boruvka rounds, against tests/density_ref.py applied to the edges hs_self_join
returns -- every filter path and batch cut, both sources of the pairs and the fall-back, multiplicity, the cut ladder
against hs_dbscan, the device form, the capacity pattern, errors and the handle's state."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import density_ref as dr
from tests import msf_ref as mr
from tests.test_gpu_clustering import _families
from tests.test_gpu_components import _PATHS, _SHAPES, _db, chain_case
from tests.test_gpu_msf import _BUDGETS

pytestmark = pytest.mark.gpu

_MIN_PTS = (1, 2, 3, 5, 8)


def _ref(n, edges, min_pts):
    return dr.tree_from_edges(n, edges["i"], edges["j"], edges["dist"], min_pts)


def _check(got, want, n_edges, resident, what):
    assert dr.same_result(got, want), what
    assert got["n_graph_edges"] == n_edges, what
    assert (got["lo"] < got["hi"]).all(), what
    assert got["resident"] == resident, what
    assert got["self_joins"] == (1 if resident else 2 + 2 * got["rounds"]), what


@pytest.mark.parametrize("min_pts", _MIN_PTS)
@pytest.mark.parametrize("k,K,L,W,R", _SHAPES)
def test_tree_equals_reference_of_own_edges_on_every_path(k, K, L, W, R, min_pts):
    codes = _db(k, R)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    ref = {}
    for mode, opts in _PATHS:
        eng = Engine(k, K, L, W, a, b, options=opts)
        eng.set_verify_mode(mode)
        eng.index_build(codes)
        for sq in (False, True):
            edges = eng.self_join(R, sqrt_test=sq)
            # the reference is computed once per edge list: the paths return the same one
            if sq in ref and all(np.array_equal(edges[f], ref[sq][0][f]) for f in ("i", "j")) and \
                    np.array_equal(edges["dist"].view(np.uint64), ref[sq][0]["dist"].view(np.uint64)):
                want = ref[sq][1]
            else:
                assert sq not in ref, (mode, opts, sq)
                want = _ref(n, edges, min_pts)
                ref[sq] = (edges, want)
                assert len(edges["i"]) > 1000 and 0 < want["n_core"] and len(want["lo"]) > 100
            for budget, resident in _BUDGETS:
                what = (mode, opts, sq, budget)
                eng.set_option("msf_edge_budget", budget)
                got = eng.density_tree(R, min_pts, sqrt_test=sq)
                _check(got, want, len(edges["i"]), resident, what)
                assert 1 <= got["rounds"] <= 13, what          # ceil(log2 2700) = 12
            eng.set_option("msf_edge_budget", -1)
            if min_pts == 1:
                msf = eng.msf(R, sqrt_test=sq, want_label=True)
                assert mr.same_tree(dict(lo=got["lo"], hi=got["hi"], dist=got["w"]), msf), (mode, opts, sq)
                assert np.array_equal(got["label"], msf["label"]) and got["rounds"] == msf["rounds"]
                assert got["n_clusters"] == msf["n_components"] and got["n_core"] == n
        eng.close()


def test_multiplicity_and_the_degree_threshold():
    """Five copies of one k-mer and three of another inside a family: neighbours at distance 0 count once each."""
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    rng = np.random.default_rng(21)
    fam = _families(rng, k, 12, 30, max_sub=2)
    _, inv, cnt = np.unique(fam, axis=0, return_inverse=True, return_counts=True)
    single = np.flatnonzero(cnt[inv.ravel()] == 1)                 # members no other member equals
    x, y = int(single[0]), int(single[single >= 40][0])
    codes = np.concatenate([fam, np.repeat(fam[x:x + 1], 4, axis=0), np.repeat(fam[y:y + 1], 2, axis=0),
                            synth.make_db(300, k, seed=5)])
    kx, ky = fam[x].copy(), fam[y].copy()
    rng.shuffle(codes)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    edges = eng.self_join(R)
    five = np.flatnonzero((codes == kx).all(axis=1))
    three = np.flatnonzero((codes == ky).all(axis=1))
    assert len(five) == 5 and len(three) == 3
    for ids in (five, three):                                      # the data holds those cliques of weight 0
        inside = np.isin(edges["i"], ids) & np.isin(edges["j"], ids)
        assert inside.sum() == len(ids) * (len(ids) - 1) and (edges["dist"][inside] == 0.0).all()
        zero_nb = np.isin(edges["i"], ids) & (edges["dist"] == 0.0)
        assert zero_nb.sum() == inside.sum()                       # ... and no other neighbour at distance 0
    degree = np.bincount(edges["i"], minlength=n)
    assert (degree[five] >= 5).all() and (degree[three] >= 3).all()
    low = int(degree[degree > 0].min())                            # the smallest degree of a k-mer that has neighbours
    for min_pts in sorted({2, 3, 4, 5, 6, low + 1, low + 2}):
        want = _ref(n, edges, min_pts)
        got = eng.density_tree(R, min_pts)
        _check(got, want, len(edges["i"]), 1, min_pts)
        alone = eng.core_distance(R, min_pts)
        assert np.array_equal(alone["core"].view(np.uint64), want["core"].view(np.uint64))
        assert (alone["n_core"], alone["n_edges"]) == (want["n_core"], len(edges["i"]))
        core = got["core"]
        if min_pts <= 5:
            assert (core[five] == 0.0).all() and not np.signbit(core[five]).any()
        if min_pts == 6:
            assert (core[five] > 0.0).all() and np.isfinite(core[five]).all()
        if min_pts <= 3:
            assert (core[three] == 0.0).all()
        if min_pts == 4:
            assert (core[three] > 0.0).all() and np.isfinite(core[three]).all()
        # degree exactly min_pts - 1: finite; min_pts - 2: +inf
        assert np.array_equal(np.isfinite(core), degree >= min_pts - 1)
        if min_pts in (low + 1, low + 2):
            assert ((degree == low) & np.isfinite(core)).any() == (min_pts == low + 1)
            assert ((degree == low) & np.isinf(core)).any() == (min_pts == low + 2)
    assert (degree == 0).any()                                     # (degree min_pts - 2 at min_pts = 2)
    eng.close()


def _msf(eng, R):
    """Engine.msf without the field that names the source of its pairs (the budget option moves it)."""
    tree = eng.msf(R, want_label=True)
    del tree["resident"]
    return tree


def _batch_cut_case(eng, n, R, sq, min_pts_list):
    edges = eng.self_join(R, sqrt_test=sq)
    for min_pts in min_pts_list:
        want = _ref(n, edges, min_pts)
        for budget, resident in _BUDGETS:
            eng.set_option("msf_edge_budget", budget)
            _check(eng.density_tree(R, min_pts, sqrt_test=sq), want, len(edges["i"]), resident, (sq, min_pts, budget))
    return edges


def test_batch_cuts_on_chains():
    """query_batch = 16: core[b] comes from another batch than a's; chains take several Boruvka rounds."""
    codes, R, chains, isolated = chain_case()
    n, k = codes.shape
    W = 1.0e6
    a = np.random.default_rng(1).standard_normal((1, 1, 8 * k))
    b = np.full((1, 1), W / 2)
    eng = Engine(k, 1, 1, W, a, b, options=dict(query_batch=16))
    assert eng.index_build(codes)["n_buckets"] == [1]
    for sq in (True, False):
        _batch_cut_case(eng, n, R, sq, (2, 3, 4))
    got = eng.density_tree(R, 2)
    assert got["n_core"] == n - len(isolated) and got["n_clusters"] == 2 and got["rounds"] >= 1
    eng.close()


def test_batch_cuts_on_families():
    k, K, L, W, R = _SHAPES[0]
    codes = _db(k, R)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b, options=dict(query_batch=16))
    eng.index_build(codes)
    edges = _batch_cut_case(eng, len(codes), R, True, (3, 8))
    assert len(edges["i"]) > 1000
    eng.close()


def test_split_batches(monkeypatch):
    """The test build's HS_TEST_SPLIT_ABOVE: every batch above 100 queries is cut in halves; the halves bring every hit
    once and each k-mer's hits together."""
    k, K, L, W, R = _SHAPES[0]
    codes = _db(k, R)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "100")
    eng = Engine(k, K, L, W, a, b, hooks=True)
    eng.index_build(codes)
    edges = eng.self_join(R)
    for min_pts in (1, 4):
        _check(eng.density_tree(R, min_pts), _ref(n, edges, min_pts), len(edges["i"]), 1, min_pts)
    assert eng.profile()["verify_launches"] >= n // 100
    eng.close()


@pytest.mark.parametrize("min_pts", [2, 4])
def test_cut_ladder_against_dbscan(min_pts):
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _db(k, R)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    tree = eng.density_tree(R, min_pts, sqrt_test=True)
    assert tree["n_tree_edges"] > 300
    edges = eng.self_join(R)
    heights = np.unique(np.quantile(tree["w"], [0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0], method="nearest"))
    raw = np.unique(np.quantile(edges["dist"], [0.2, 0.6], method="nearest"))          # exact edge distances
    assert len(heights) >= 5 and np.isin(heights, tree["w"]).all() and np.isin(raw, edges["dist"]).all()
    n_clusters = []
    for hgt in np.concatenate([heights, raw]):
        for r in (hgt, np.nextafter(hgt, -np.inf)):
            cut = capi.density_tree_cut(tree, r)
            db = eng.dbscan(float(r), min_pts, sqrt_test=True)
            is_core = eng.degrees(float(r)).astype(np.int64) + 1 >= min_pts
            assert np.array_equal(cut["label"] != capi.NOISE, is_core), r
            assert np.array_equal(cut["label"][is_core], db["label"][is_core]), r
            assert cut["n_clusters"] == db["n_clusters"] and is_core.sum() == db["n_core"], r
            n_clusters.append(cut["n_clusters"])
    assert len(set(n_clusters)) >= 3
    full = capi.density_tree_cut(tree, R)
    assert np.array_equal(full["label"], tree["label"]) and full["n_clusters"] == tree["n_clusters"]
    # d2 <= R * R: only the whole forest is promised to match
    tree0 = eng.density_tree(R, min_pts, sqrt_test=False)
    db0 = eng.dbscan(R, min_pts, sqrt_test=False, want_degree=True)
    core0 = db0["degree"].astype(np.int64) + 1 >= min_pts
    assert np.array_equal(tree0["label"] != capi.NOISE, core0)
    assert np.array_equal(tree0["label"][core0], db0["label"][core0]) and tree0["n_clusters"] == db0["n_clusters"]
    eng.close()


def test_min_pts_above_every_degree():
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _families(np.random.default_rng(7), k, 25, 40)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    degree = eng.degrees(R)
    assert degree.max() > 10
    for budget, resident in _BUDGETS:
        eng.set_option("msf_edge_budget", budget)
        got = eng.density_tree(R, int(degree.max()) + 2)
        assert got["n_tree_edges"] == 0 and len(got["lo"]) == 0 and got["rounds"] == 0
        assert got["n_core"] == got["n_clusters"] == 0 and got["n_graph_edges"] == int(degree.sum())
        assert (got["label"] == capi.NOISE).all() and np.isinf(got["core"]).all()
        assert got["resident"] == resident and got["self_joins"] == (1 if resident else 2)
    got = eng.density_tree(R, int(degree.max()) + 1)                  # ... and exactly at it: the densest k-mers are core
    assert got["n_core"] == int((degree == degree.max()).sum())
    eng.close()


def test_device_form_capacity_errors_and_state():
    import torch
    k, K, L, W, R, min_pts = 25, 4, 3, 120.0, 50.0, 4
    codes = _families(np.random.default_rng(7), k, 25, 40)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    out = capi._DensityInfo(7, 7, 7, 7, 7, 7, 7)
    fields = [f[0] for f in capi._DensityInfo._fields_]
    lo, hi, w = np.full(n, 77, dtype=np.uint32), np.full(n, 78, dtype=np.uint32), np.full(n, 7.5)
    label, core = np.full(n, 79, dtype=np.uint32), np.full(n, 8.5)
    ptrs = (capi._vp(lo), capi._vp(hi), capi._vp(w))
    untouched = lambda: ((lo == 77).all() and (hi == 78).all() and (w == 7.5).all() and (label == 79).all()
                         and (core == 8.5).all())
    call = lambda R_, mp, cap: eng._lib.hs_density_tree(eng._h, R_, 1, mp, *ptrs, cap, capi._vp(label), capi._vp(core),
                                                        C.byref(out))
    assert call(R, min_pts, n) == capi.HS_ERR_STATE and all(getattr(out, f) == 0 for f in fields)      # no index yet
    nc, ne = C.c_uint64(7), C.c_uint64(7)
    assert eng._lib.hs_core_distance(eng._h, R, 1, min_pts, capi._vp(core), C.byref(nc), C.byref(ne)) == capi.HS_ERR_STATE
    assert (nc.value, ne.value) == (0, 0)
    eng.index_build(codes)
    out.rounds = 7
    assert call(R, 0, n) == capi.HS_ERR_INVALID and all(getattr(out, f) == 0 for f in fields)
    assert call(float("nan"), min_pts, n) == capi.HS_ERR_INVALID
    assert eng._lib.hs_density_tree(eng._h, R, 1, min_pts, *ptrs, n, None, None, None) == capi.HS_ERR_INVALID
    assert eng._lib.hs_density_tree(eng._h, R, 1, min_pts, None, None, None, n, None, None, C.byref(out)) == \
        capi.HS_ERR_INVALID                                            # room without arrays
    for bad_R, bad_mp in ((float("nan"), min_pts), (R, 0)):
        assert eng._lib.hs_core_distance(eng._h, bad_R, 1, bad_mp, capi._vp(core), C.byref(nc), C.byref(ne)) == \
            capi.HS_ERR_INVALID
    assert untouched()
    # the other reductions before ...
    before = (eng.self_join(R), eng.components(R), eng.dbscan(R, 4, want_degree=True), _msf(eng, R))
    host = eng.density_tree(R, min_pts)
    m = host["n_tree_edges"]
    assert 100 < m < n - 1 and host["resident"] == 1
    _check(host, _ref(n, before[0], min_pts), len(before[0]["i"]), 1, "host")
    # the device form, with exactly the room needed
    d_lo = torch.full((m,), 0x7fffffff, dtype=torch.int32, device="cuda")
    d_hi = torch.full((m,), 0x7fffffff, dtype=torch.int32, device="cuda")
    d_w = torch.full((m,), -1.0, dtype=torch.float64, device="cuda")
    d_label = torch.full((n,), 0x7fffffff, dtype=torch.int32, device="cuda")
    d_core = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    info = eng.density_tree_dev(d_lo.data_ptr(), d_hi.data_ptr(), d_w.data_ptr(), m, R, min_pts,
                                d_label_ptr=d_label.data_ptr(), d_core_ptr=d_core.data_ptr())
    assert info == {f: host[f] for f in fields}
    dev = dict(lo=d_lo.cpu().numpy().view(np.uint32), hi=d_hi.cpu().numpy().view(np.uint32), w=d_w.cpu().numpy())
    assert dr.same_tree(dev, host)
    assert np.array_equal(d_label.cpu().numpy().view(np.uint32), host["label"])
    assert np.array_equal(d_core.cpu().numpy().view(np.uint64), host["core"].view(np.uint64))
    d_core.fill_(-1.0)
    torch.cuda.synchronize()
    assert eng.core_distance_dev(d_core.data_ptr(), R, min_pts) == (host["n_core"], host["n_graph_edges"])
    assert np.array_equal(d_core.cpu().numpy().view(np.uint64), host["core"].view(np.uint64))
    # the two-call pattern: the count with no room (null arrays), too little room; nothing written either time
    assert eng._lib.hs_density_tree(eng._h, R, 1, min_pts, None, None, None, 0, None, None, C.byref(out)) == \
        capi.HS_ERR_CAPACITY
    assert {f: getattr(out, f) for f in fields} == info
    for t in (d_w, d_core):
        t.fill_(-1.0)
    for t in (d_lo, d_hi, d_label):
        t.fill_(0x7fffffff)
    torch.cuda.synchronize()
    with pytest.raises(capi.HsError) as e:
        eng.density_tree_dev(d_lo.data_ptr(), d_hi.data_ptr(), d_w.data_ptr(), m - 1, R, min_pts,
                             d_label_ptr=d_label.data_ptr(), d_core_ptr=d_core.data_ptr())
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == m
    assert (d_w.cpu().numpy() == -1.0).all() and (d_core.cpu().numpy() == -1.0).all()
    for t in (d_lo, d_hi, d_label):
        assert (t.cpu().numpy() == 0x7fffffff).all()
    assert call(R, min_pts, m - 1) == capi.HS_ERR_CAPACITY and out.n_tree_edges == m and untouched()
    # ... and after: identical bits, whichever source the density tree read its pairs from, and the other way round
    for budget in (0, -1):
        eng.set_option("msf_edge_budget", budget)
        again = eng.density_tree(R, min_pts)
        assert dr.same_result(again, host) and again["rounds"] == host["rounds"]
        after = (eng.self_join(R), eng.components(R), eng.dbscan(R, 4, want_degree=True), _msf(eng, R))
        for x, y in zip(before, after):
            assert x.keys() == y.keys()
            for f in x:
                assert np.array_equal(x[f], y[f]), f
    assert dr.same_result(eng.density_tree(R, min_pts), host)
    assert len(before[0]["i"]) > 1000 and before[2]["n_clusters"] >= 2
    eng.close()
