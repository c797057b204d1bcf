"""hs_degrees / hs_dbscan on the GPU: the degrees and the density clusters of the self-join's graph, reduced on the device,
against the plain Python of tests/dbscan_ref.py applied to the edges hs_self_join returns (every filter path, every
batch cut), to the CPU oracle's R-ball graph (chains, and a border k-mer between two clusters), and on duplicates,
ranges, device pointers and errors.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import dbscan_ref as dr
from tests.test_gpu_clustering import _families
from tests.test_gpu_components import _PATHS, _SHAPES, _db, chain_case

pytestmark = pytest.mark.gpu

_MIN_PTS = (1, 2, 5, 31, 10 ** 6)


@pytest.mark.parametrize("k,K,L,W,R", _SHAPES)
def test_degrees_and_dbscan_equal_the_rule_on_own_edges_on_every_path(k, K, L, W, R):
    codes = _db(k, R)   # planted families of 30 and 1 500 random k-mers
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    ref = {}
    for mode, opts in _PATHS:
        eng = Engine(k, K, L, W, a, b, options=opts)
        eng.set_verify_mode(mode)
        eng.index_build(codes)
        for sq in (False, True):
            what = (mode, opts, sq)
            edges = eng.self_join(R, sqrt_test=sq)
            # the reference is computed once per edge list: the paths return the same one
            if sq in ref and all(np.array_equal(edges[f], ref[sq][0][f]) for f in ("i", "j")):
                want = ref[sq][1]
            else:
                assert sq not in ref, what
                nbr = dr.neighbours(n, edges["i"], edges["j"])
                want = {m: dr.dbscan_from_neighbours(nbr, m) for m in _MIN_PTS}
                ref[sq] = (edges, want)
                assert len(edges["i"]) > 1000
                at5 = want[5]
                if R < 100.0:   # what the input must be for the test to mean something
                    assert at5["n_clusters"] >= 2 and at5["n_core"] >= 100 and at5["n_noise"] >= 100, what
                else:           # R = 171 chains everything into one component, dense throughout: that is a case too
                    assert (at5["n_clusters"], at5["n_core"]) == (1, n), what
                assert want[10 ** 6]["n_noise"] == n
            deg = eng.degrees(R, sqrt_test=sq)
            assert deg.dtype == np.uint32 and np.array_equal(deg, np.bincount(edges["i"], minlength=n)), what
            for m in _MIN_PTS:
                got = eng.dbscan(R, m, sqrt_test=sq, want_degree=True)
                dr.assert_same(got, want[m], what + (m,))
                assert got["n_edges"] == len(edges["i"]), what
            assert np.array_equal(eng.dbscan(R, 1, sqrt_test=sq)["label"], eng.components(R, sqrt_test=sq)["label"]), what
        eng.close()


def border_case():
    """chain_case()'s chains and isolated k-mers (ids shuffled) followed by ten rows built by hand, ids n0 .. n0 + 9:
         A0 | B0 B1 B2 B3 | x | A1 A2 A3 | y
    Group A and group B are four k-mers each that differ from their base at position 0 only (any two residues lie
    within R: 26.0 is the largest residue distance, R = 26.001).  B's base is A's with positions 1 and 2 changed,
    each by a residue pair exactly 26.0 apart, so every A is sqrt(2) x 26 or more from every B.  x is A1 with
    position 1 changed that way = B0 with position 2 changed back: 26.0 from A1 and from B0, and sqrt(26^2 + 3^2) or
    more from every other member (3.0 is the smallest distance of two different residues).  At min_pts = 4 the groups
    are two clusters (labels A0 < B0) and x, with two neighbours, is a border k-mer between them whose smallest core
    neighbour B0 is in the cluster with the LARGER label.  y is A3 with position 3 changed by such a pair: A3 is its
    one neighbour, which makes it a border k-mer at min_pts = 3 and 4 (the chains have none at 3: their steps are short
    enough for every k-mer to reach two others).  Returns (codes, R, id of x, id of A1, id of B0)."""
    codes, R, _, _ = chain_case()
    k = codes.shape[1]
    rng = np.random.default_rng(77)
    base_a = rng.integers(0, 20, size=k).astype(np.uint8)
    base_a[1], base_a[2], base_a[3] = 3, 14, 3   # residue distances (3, 17) and (14, 17) are 26.0
    base_b = base_a.copy()
    base_b[1], base_b[2] = 17, 17
    p0 = [0, 5, 9, 12]                      # the groups' residues at position 0; the first is x's
    grp_a = np.repeat(base_a[None, :], 4, axis=0)
    grp_b = np.repeat(base_b[None, :], 4, axis=0)
    grp_a[:, 0] = [p0[1], p0[0], p0[2], p0[3]]   # A0, A1 (x's residue), A2, A3
    grp_b[:, 0] = p0                             # B0 (x's residue), B1, B2, B3
    x = base_a.copy()
    x[0], x[1] = p0[0], 17
    y = grp_a[3].copy()
    y[3] = 17
    n0 = len(codes)
    rows = np.concatenate([grp_a[:1], grp_b, x[None, :], grp_a[1:], y[None, :]])
    return np.concatenate([codes, rows]), R, n0 + 5, n0 + 6, n0 + 1


@pytest.fixture(scope="module")
def border_ref(oracle):
    """The brute-force R-ball graph of border_case() from the CPU oracle and its reference clusterings, checked to
    be what the tests need, once."""
    codes, R, x, a1, b0 = border_case()
    n = len(codes)
    pts = oracle.embed_codes(codes)
    adj = np.sqrt(oracle.pairwise_square(pts, pts)) <= R
    np.fill_diagonal(adj, False)
    nbr = dr.neighbours(n, *np.nonzero(adj))
    want = {m: dr.dbscan_from_neighbours(nbr, m) for m in (2, 3, 4)}
    at3 = want[3]
    assert nbr[n - 1] == {n - 2} and at3["label"][n - 1] == at3["label"][n - 2] != dr.NOISE   # y, a border k-mer
    assert at3["n_core"] >= 300 and at3["n_border"] >= 1 and at3["n_noise"] >= 30 and at3["n_clusters"] >= 2
    # x: not core at min_pts = 4, its two neighbours core and in two different clusters, the smaller id in the
    # cluster with the larger label -- the one place where the anchor rule has a choice to make
    at4 = want[4]
    assert nbr[x] == {a1, b0} and b0 < a1
    assert at4["degree"][x] + 1 < 4 <= min(at4["degree"][a1], at4["degree"][b0]) + 1
    assert at4["label"][a1] == n - 10 and at4["label"][b0] == b0 and at4["label"][a1] < at4["label"][b0]
    assert at4["label"][x] == at4["label"][b0]
    assert at3["label"][x] == at3["label"][a1] == at3["label"][b0]   # (at 3, x is core itself and fuses them)
    return codes, R, int(adj.sum()), want


@pytest.mark.parametrize("query_batch", [0, 16])
def test_r_ball_graph_with_chains_and_a_border_between_two_clusters(border_ref, query_batch):
    """One table, one hash function, a bucket wide enough for everything: the graph is the R-ball graph."""
    codes, R, n_edges, want = border_ref
    n, k = codes.shape
    W = 1.0e6
    a = np.random.default_rng(1).standard_normal((1, 1, 8 * k))
    b = np.full((1, 1), W / 2)
    eng = Engine(k, 1, 1, W, a, b, options=dict(query_batch=query_batch) if query_batch else None)
    assert eng.index_build(codes)["n_buckets"] == [1]
    for sq in (True, False):
        for m in (2, 3, 4):
            got = eng.dbscan(R, m, sqrt_test=sq, want_degree=True)
            dr.assert_same(got, want[m], (sq, m))
            assert got["n_edges"] == n_edges
    eng.close()


def test_duplicates_at_radius_zero():
    k, K, L, W = 25, 4, 3, 120.0
    rng = np.random.default_rng(12)
    base = synth.make_db(700, k, seed=6)
    codes = np.concatenate([base, base[rng.integers(0, 700, 500)], base[:30], base[:30]])
    rng.shuffle(codes)
    n = len(codes)
    first = {}
    same = np.array([first.setdefault(row.tobytes(), i) for i, row in enumerate(codes)], dtype=np.uint32)
    mult = np.bincount(same, minlength=n)[same]
    want = np.where(mult >= 3, same, dr.NOISE).astype(np.uint32)
    assert (np.bincount(same, minlength=n) >= 3).sum() >= 30 and (mult == 2).sum() >= 50 and (mult == 1).sum() >= 50
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    for sq in (True, False):
        assert np.array_equal(eng.degrees(0.0, sqrt_test=sq), mult - 1)
        got = eng.dbscan(0.0, 3, sqrt_test=sq, want_degree=True)
        assert np.array_equal(got["label"], want) and np.array_equal(got["degree"], mult - 1)
        assert got["n_clusters"] == (np.bincount(same, minlength=n) >= 3).sum()
        assert (got["n_core"], got["n_border"], got["n_noise"]) == ((mult >= 3).sum(), 0, (mult < 3).sum())
        assert got["n_edges"] == int((mult - 1).sum())
    eng.close()


def test_degree_ranges_add_up():
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _families(np.random.default_rng(6), k, 25, 40)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    full = eng.degrees(R)
    assert np.array_equal(full, np.bincount(eng.self_join(R)["i"], minlength=n)) and full.sum() > 1000
    cuts = [0, 1, 333, 334, n]
    total = np.zeros(n, dtype=np.int64)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = eng.degrees(R, first=lo, count=hi - lo)
        assert np.array_equal(part[lo:hi], full[lo:hi]), (lo, hi)
        assert not part[:lo].any() and not part[hi:].any(), (lo, hi)
        total += part
    assert np.array_equal(total, full)
    assert not eng.degrees(R, first=n, count=0).any() and not eng.degrees(R, first=5, count=0).any()
    eng.close()


def test_device_forms_and_state():
    import torch
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _families(np.random.default_rng(7), k, 25, 40)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    qcodes = codes[::7].copy()

    def others():
        return (eng.components(R), eng.self_join(R), eng.query_codes(qcodes, R), eng.annotate(qcodes, R, codes=True))
    before = others()
    host = eng.dbscan(R, 5, want_degree=True)
    dr.assert_same(host, dr.dbscan_from_edges(n, before[1]["i"], before[1]["j"], 5))
    assert host["n_clusters"] >= 2 and host["n_edges"] > 1000

    def tensor():
        return torch.full((n,), 0x7ffffffe, dtype=torch.int32, device="cuda")
    d_label, d_degree, d_only = tensor(), tensor(), tensor()
    torch.cuda.synchronize()
    counts = eng.dbscan_dev(d_label.data_ptr(), R, 5, d_degree_ptr=d_degree.data_ptr())
    assert np.array_equal(d_label.cpu().numpy().view(np.uint32), host["label"])
    assert np.array_equal(d_degree.cpu().numpy().view(np.uint32), host["degree"])
    assert counts == {f: host[f] for f in counts} and len(counts) == 5
    d_label.fill_(0x7ffffffe)
    torch.cuda.synchronize()
    assert eng.dbscan_dev(d_label.data_ptr(), R, 5) == counts          # the degree array is optional
    assert np.array_equal(d_label.cpu().numpy().view(np.uint32), host["label"])
    assert eng.degrees_dev(d_only.data_ptr(), R) == host["n_edges"]
    assert np.array_equal(d_only.cpu().numpy().view(np.uint32), host["degree"])
    assert np.array_equal(eng.degrees(R), host["degree"])
    # calls at another radius and another min_pts in between leave no trace: every call starts from empty state
    wide, tight, dense = eng.dbscan(70.0, 5, sqrt_test=False), eng.dbscan(5.0, 2), eng.dbscan(R, 25)
    assert wide["n_edges"] >= host["n_edges"] > tight["n_edges"] and dense["n_core"] < host["n_core"]
    eng.degrees(70.0, first=3, count=100)
    again = eng.dbscan(R, 5, want_degree=True)
    dr.assert_same(again, host)
    after = others()
    for x, y in zip(before, after):
        assert x.keys() == y.keys()
        for f in x:
            assert np.array_equal(x[f], y[f]), f
    assert len(before[2]["q"]) > 1000 and len(before[3]["id"]) > 100
    assert np.array_equal(eng.dbscan(R, 1)["label"], before[0]["label"])
    eng.close()


def test_errors():
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _families(np.random.default_rng(8), k, 10, 30)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    label, degree = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
    c = capi._DbscanCounts(5, 5, 5, 5, 5)
    ne = C.c_uint64(5)

    def zeroed():
        return (c.n_clusters, c.n_core, c.n_border, c.n_noise, c.n_edges) == (0, 0, 0, 0, 0)
    st = eng._lib.hs_dbscan(eng._h, R, 1, 3, capi._vp(label), None, C.byref(c))            # no index yet
    assert st == capi.HS_ERR_STATE and zeroed()
    assert eng._lib.hs_degrees(eng._h, R, 1, capi._vp(degree), C.byref(ne)) == capi.HS_ERR_STATE and ne.value == 0
    eng.index_build(codes)
    assert eng.dbscan(R, 3)["n_edges"] > 100
    c.n_edges = c.n_core = 5
    assert eng._lib.hs_dbscan(eng._h, R, 1, 0, capi._vp(label), None, C.byref(c)) == capi.HS_ERR_INVALID and zeroed()
    assert eng._lib.hs_dbscan(eng._h, R, 1, 3, capi._vp(label), None, None) == capi.HS_ERR_INVALID
    assert eng._lib.hs_dbscan(eng._h, R, 1, 3, None, None, C.byref(c)) == capi.HS_ERR_INVALID
    assert eng._lib.hs_degrees(eng._h, R, 1, None, C.byref(ne)) == capi.HS_ERR_INVALID
    for call in (lambda: eng.dbscan(R, 0), lambda: eng.dbscan(float("nan"), 3), lambda: eng.degrees(float("nan")),
                 lambda: eng.degrees(R, first=n - 100, count=101), lambda: eng.degrees(R, first=n + 1, count=0),
                 lambda: eng.degrees(R, first=0, count=n + 1)):
        with pytest.raises(capi.HsError) as e:
            call()
        assert e.value.status == capi.HS_ERR_INVALID
    eng.set_planes(*synth.make_planes(k, K, L, W, seed=4))                                  # drops the index
    assert eng._lib.hs_dbscan(eng._h, R, 1, 3, capi._vp(label), None, C.byref(c)) == capi.HS_ERR_STATE
    assert eng._lib.hs_degrees(eng._h, R, 1, capi._vp(degree), None) == capi.HS_ERR_STATE
    eng.index_build(codes)
    edges = eng.self_join(R)
    dr.assert_same(eng.dbscan(R, 3, want_degree=True), dr.dbscan_from_edges(n, edges["i"], edges["j"], 3), "after new planes")
    eng.close()
