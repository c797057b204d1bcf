"""hs_msf on the GPU: the minimum spanning forest of the self-join's graph, found by Boruvka rounds on the device, against
the plain Kruskal of tests/msf_ref.py applied to the edges hs_self_join returns -- every filter path and batch cut, both
sources of the pairs (kept in HBM, re-joined per pass, and the fall-back from one to the other), heavy ties, long
chains, the cut property against hs_components, the device form, the capacity pattern, errors and the handle's state."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import msf_ref as mr
from tests.test_gpu_clustering import _families
from tests.test_gpu_components import _PATHS, _SHAPES, _db, chain_case

pytestmark = pytest.mark.gpu

# HS_OPT_MSF_EDGE_BUDGET -> info.resident: never keep the pairs; the default; a list of four pairs, which overflows
_BUDGETS = [(0, 0), (-1, 1), (64, 0)]


def _check(got, n, want, comps, n_edges, what):
    assert mr.same_tree(got, want), what
    assert got["n_tree_edges"] == len(want["lo"]) == n - got["n_components"], what
    assert got["label"].dtype == np.uint32 and np.array_equal(got["label"], comps["label"]), what
    assert np.array_equal(got["label"], want["label"]), what
    assert got["n_components"] == comps["n_components"], what
    assert got["n_graph_edges"] == n_edges == want["n_graph_edges"], what
    assert (got["lo"] < got["hi"]).all(), what


@pytest.mark.parametrize("k,K,L,W,R", _SHAPES)
def test_msf_equals_kruskal_of_own_edges_on_every_path(k, K, L, W, R):
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
            comps = eng.components(R, sqrt_test=sq)
            # the reference forest is computed once per edge list: the paths return the same one
            if sq in ref and all(np.array_equal(edges[f], ref[sq][0][f]) for f in ("i", "j")) and \
                    np.array_equal(edges["dist"].view(np.uint64), ref[sq][0]["dist"].view(np.uint64)):
                want = ref[sq][1]
            else:
                assert sq not in ref, (mode, opts, sq)
                want = mr.msf_from_edges(n, edges["i"], edges["j"], edges["dist"])
                ref[sq] = (edges, want)
                assert len(edges["i"]) > 1000
            for budget, resident in _BUDGETS:
                what = (mode, opts, sq, budget)
                eng.set_option("msf_edge_budget", budget)
                got = eng.msf(R, sqrt_test=sq, want_label=True)
                assert got["resident"] == resident, what
                _check(got, n, want, comps, len(edges["i"]), what)
                assert 1 <= got["rounds"] <= 13, what          # ceil(log2 2700) = 12
        eng.close()


def test_self_join_weights_are_the_same_bits_in_both_directions():
    for k, K, L, W, R in _SHAPES[:3]:
        codes = _db(k, R)
        a, b = synth.make_planes(k, K, L, W, seed=3)
        eng = Engine(k, K, L, W, a, b)
        eng.index_build(codes)
        for sq in (False, True):
            e = eng.self_join(R, sqrt_test=sq)
            fwd = dict(zip(zip(e["i"].tolist(), e["j"].tolist()), e["dist"].view(np.uint64).tolist()))
            assert len(fwd) == len(e["i"]) > 1000
            assert all(fwd.get((j, i)) == d for (i, j), d in fwd.items()), (k, sq)
        eng.close()


def test_ties():
    """Two cliques of weight 0 (5 copies of one k-mer, 3 of another) inside a family, and the many equal distances a
    family's one-residue substitutions give: the tie-break (lo, hi) decides most of the tree."""
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    rng = np.random.default_rng(21)
    fam = _families(rng, k, 12, 30, max_sub=2)
    codes = np.concatenate([fam, np.repeat(fam[3:4], 4, axis=0), np.repeat(fam[40:41], 2, axis=0),
                            synth.make_db(300, k, seed=5)])
    rng.shuffle(codes)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    edges = eng.self_join(R)
    once = edges["i"] < edges["j"]
    _, counts = np.unique(edges["dist"][once].view(np.uint64), return_counts=True)
    assert int((counts * (counts - 1) // 2).sum()) >= 100          # pairs of edges with equal distance bits
    zero = once & (edges["dist"] == 0.0)
    assert zero.sum() >= 10 + 3                                    # a 5-clique and a 3-clique of weight 0
    want = mr.msf_from_edges(n, edges["i"], edges["j"], edges["dist"])
    assert (want["dist"] == 0.0).sum() >= 4 + 2
    comps = eng.components(R)
    for budget, resident in _BUDGETS:
        eng.set_option("msf_edge_budget", budget)
        got = eng.msf(R, want_label=True)
        assert got["resident"] == resident
        _check(got, n, want, comps, len(edges["i"]), budget)
    eng.close()


@pytest.mark.parametrize("query_batch", [0, 16])
def test_chains(query_batch):
    """Two 200-chains and 40 isolated k-mers in one bucket: components far from cliques, whose spanning tree is
    (nearly) the chain itself and takes several rounds to assemble."""
    codes, R, chains, isolated = chain_case()
    n, k = codes.shape
    W = 1.0e6
    a = np.random.default_rng(1).standard_normal((1, 1, 8 * k))
    b = np.full((1, 1), W / 2)
    eng = Engine(k, 1, 1, W, a, b, options=dict(query_batch=query_batch) if query_batch else None)
    assert eng.index_build(codes)["n_buckets"] == [1]
    for sq in (True, False):
        edges = eng.self_join(R, sqrt_test=sq)
        want = mr.msf_from_edges(n, edges["i"], edges["j"], edges["dist"])
        comps = eng.components(R, sqrt_test=sq)
        for budget, resident in _BUDGETS:
            eng.set_option("msf_edge_budget", budget)
            got = eng.msf(R, sqrt_test=sq, want_label=True)
            assert got["resident"] == resident
            _check(got, n, want, comps, len(edges["i"]), (sq, budget))
            assert 2 <= got["rounds"] <= 10
            assert got["n_tree_edges"] == 2 * 199 and got["n_components"] == 2 + len(isolated)
            for c in chains:
                inside = np.isin(got["lo"], c) & np.isin(got["hi"], c)
                assert inside.sum() == 199 and (np.isin(got["lo"], c) == inside).all()
    eng.close()


def test_cut_property():
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _db(k, R)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    tree = eng.msf(R, sqrt_test=True, want_label=True)
    assert tree["n_tree_edges"] > 500
    heights = np.unique(np.quantile(tree["dist"], [0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0], method="nearest"))
    assert len(heights) >= 5 and np.isin(heights, tree["dist"]).all()
    n_comp = []
    for hgt in heights:
        for r in (hgt, np.nextafter(hgt, -np.inf)):
            cut = capi.msf_cut(tree, r)
            comps = eng.components(float(r), sqrt_test=True)
            assert np.array_equal(cut["label"], comps["label"]), r
            assert cut["n_components"] == comps["n_components"] == n - int((tree["dist"] <= r).sum()), r
            n_comp.append(cut["n_components"])
    assert len(set(n_comp)) >= 8                                   # on a height and just below it differ
    full = capi.msf_cut(tree, R)
    assert np.array_equal(full["label"], tree["label"]) and full["n_components"] == tree["n_components"]
    # d2 <= R * R: only the whole forest is promised to match
    tree0 = eng.msf(R, sqrt_test=False, want_label=True)
    comps0 = eng.components(R, sqrt_test=False)
    whole = capi.msf_cut(tree0, np.inf)
    assert np.array_equal(whole["label"], comps0["label"]) and whole["n_components"] == comps0["n_components"]
    eng.close()


def test_device_form_capacity_and_state():
    import torch
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _families(np.random.default_rng(7), k, 25, 40)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    before = (eng.self_join(R), eng.components(R), eng.dbscan(R, 4, want_degree=True))
    host = eng.msf(R, want_label=True)
    m = host["n_tree_edges"]
    assert 100 < m < n - 1 and host["resident"] == 1
    want = mr.msf_from_edges(n, before[0]["i"], before[0]["j"], before[0]["dist"])
    _check(host, n, want, before[1], len(before[0]["i"]), "host")
    # the device form, with exactly the room needed
    d_lo = torch.full((m,), 0x7fffffff, dtype=torch.int32, device="cuda")
    d_hi = torch.full((m,), 0x7fffffff, dtype=torch.int32, device="cuda")
    d_dist = torch.full((m,), -1.0, dtype=torch.float64, device="cuda")
    d_label = torch.full((n,), 0x7fffffff, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    info = eng.msf_dev(d_lo.data_ptr(), d_hi.data_ptr(), d_dist.data_ptr(), m, R, d_label_ptr=d_label.data_ptr())
    assert info == {f: host[f] for f in info}
    dev = dict(lo=d_lo.cpu().numpy().view(np.uint32), hi=d_hi.cpu().numpy().view(np.uint32), dist=d_dist.cpu().numpy())
    assert mr.same_tree(dev, host)
    assert np.array_equal(d_label.cpu().numpy().view(np.uint32), host["label"])
    # the two-call pattern: the count with no room (null arrays), too little room, nothing written either time
    out = capi._MsfInfo(7, 7, 7, 7, 7)
    st = eng._lib.hs_msf(eng._h, R, 1, None, None, None, 0, None, C.byref(out))
    assert st == capi.HS_ERR_CAPACITY and out.n_tree_edges == m and out.n_components == n - m
    assert out.n_graph_edges == host["n_graph_edges"]
    d_dist.fill_(-1.0)
    d_label.fill_(0x7fffffff)
    torch.cuda.synchronize()
    d_lo.fill_(0x7fffffff)
    d_hi.fill_(0x7fffffff)
    torch.cuda.synchronize()
    with pytest.raises(capi.HsError) as e:
        eng.msf_dev(d_lo.data_ptr(), d_hi.data_ptr(), d_dist.data_ptr(), m - 1, R, d_label_ptr=d_label.data_ptr())
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == m
    assert (d_dist.cpu().numpy() == -1.0).all() and (d_label.cpu().numpy() == 0x7fffffff).all()
    assert (d_lo.cpu().numpy() == 0x7fffffff).all() and (d_hi.cpu().numpy() == 0x7fffffff).all()
    lo, hi, dist = np.full(m, 77, dtype=np.uint32), np.full(m, 78, dtype=np.uint32), np.full(m, 7.5)
    label = np.full(n, 79, dtype=np.uint32)
    st = eng._lib.hs_msf(eng._h, R, 1, capi._vp(lo), capi._vp(hi), capi._vp(dist), m - 1, capi._vp(label), C.byref(out))
    assert st == capi.HS_ERR_CAPACITY and out.n_tree_edges == m
    assert (lo == 77).all() and (hi == 78).all() and (dist == 7.5).all() and (label == 79).all()
    # room without arrays is an argument error
    st = eng._lib.hs_msf(eng._h, R, 1, None, None, None, m, None, C.byref(out))
    assert st == capi.HS_ERR_INVALID and out.n_tree_edges == 0
    # a call at another radius in between leaves no trace: the state starts anew every time
    wide, tight = eng.msf(70.0, sqrt_test=False), eng.msf(5.0)
    assert wide["n_components"] <= host["n_components"] < tight["n_components"]
    assert tight["n_graph_edges"] < host["n_graph_edges"] and (tight["dist"] <= 5.0).all()
    for budget in (0, -1):
        eng.set_option("msf_edge_budget", budget)
        again = eng.msf(R, want_label=True)
        assert mr.same_tree(again, host) and np.array_equal(again["label"], host["label"])
        assert all(again[f] == host[f] for f in ("n_tree_edges", "n_components", "n_graph_edges", "rounds"))
    # ... and the other reductions of the self-join give what they gave before it
    after = (eng.self_join(R), eng.components(R), eng.dbscan(R, 4, want_degree=True))
    for x, y in zip(before, after):
        assert x.keys() == y.keys()
        for f in x:
            assert np.array_equal(x[f], y[f]), f
    assert len(before[0]["i"]) > 1000 and before[2]["n_clusters"] >= 2
    eng.close()


def test_no_edges_and_errors():
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = np.unique(synth.make_db(600, k, seed=11), axis=0)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    out = capi._MsfInfo(7, 7, 7, 7, 7)
    lo, hi, dist = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32), np.empty(n)
    args = (capi._vp(lo), capi._vp(hi), capi._vp(dist), n, None, C.byref(out))
    assert eng._lib.hs_msf(eng._h, R, 1, *args) == capi.HS_ERR_STATE                  # no index yet
    assert (out.n_tree_edges, out.n_components, out.n_graph_edges, out.rounds, out.resident) == (0,) * 5
    eng.index_build(codes)
    with pytest.raises(capi.HsError) as e:
        eng.msf(float("nan"))
    assert e.value.status == capi.HS_ERR_INVALID
    assert eng._lib.hs_msf(eng._h, R, 1, capi._vp(lo), capi._vp(hi), capi._vp(dist), n, None, None) == capi.HS_ERR_INVALID
    # distinct random k-mers and a radius of nothing: no edge, no tree, one pass over the pairs and no round
    assert len(eng.self_join(1e-3)["i"]) == 0
    for budget, resident in _BUDGETS:
        eng.set_option("msf_edge_budget", budget)
        got = eng.msf(1e-3, want_label=True)
        assert got["n_tree_edges"] == 0 and len(got["lo"]) == len(got["hi"]) == len(got["dist"]) == 0
        assert got["n_components"] == n and got["n_graph_edges"] == 0 and got["rounds"] == 0
        assert np.array_equal(got["label"], np.arange(n))
        assert got["resident"] == (1 if budget else 0)        # (nothing to keep: an empty list never overflows)
    eng.set_planes(*synth.make_planes(k, K, L, W, seed=4))                           # drops the index
    assert eng._lib.hs_msf(eng._h, R, 1, *args) == capi.HS_ERR_STATE
    eng.index_build(codes)
    edges = eng.self_join(R)
    got = eng.msf(R, want_label=True)
    _check(got, n, mr.msf_from_edges(n, edges["i"], edges["j"], edges["dist"]), eng.components(R), len(edges["i"]),
           "after new planes")
    eng.close()
