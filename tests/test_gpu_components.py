"""hs_components on the GPU: the connected components of the self-join's graph, united on the device, against the plain
union-find of tests/components_ref.py applied to the edges hs_self_join returns (every filter path, every batch
cut), to the CPU oracle's graph, and on inputs built to break a union-find: long chains, duplicates, ranges."""
import numpy as np
import pytest

import hsearch_amd
from hsearch_amd import Engine, capi, synth
from tests import components_ref as cr
from tests.test_gpu_clustering import _families

pytestmark = pytest.mark.gpu

_SHAPES = [(25, 4, 3, 120.0, 50.0), (39, 6, 4, 200.0, 60.0), (12, 3, 2, 90.0, 30.0), (25, 4, 3, 120.0, 171.0)]
# what forces each path (tests/test_gpu_parity.py, test_gpu_clustering.py): (verify mode, options)
_PATHS = [("auto", {}), ("stream", {}), ("join", {}), ("join16", {}), ("auto", dict(seg_mode=1)),
          ("auto", dict(seg_mode=2)), ("auto", dict(self_codes=0)), ("auto", dict(join_min_q=3, join_min_m=16)),
          ("auto", dict(query_batch=37))]


def _db(k, R):
    rng = np.random.default_rng(k + int(R))
    return np.concatenate([_families(rng, k, 40, 30), synth.make_db(1500, k, seed=4)])


def _check(got, n, edges, what):
    want = cr.labels_from_edges(n, edges["i"], edges["j"])
    assert got["label"].dtype == np.uint32 and got["label"].shape == (n,), what
    assert np.array_equal(got["label"], want), what
    assert got["n_edges"] == len(edges["i"]), what
    assert got["n_components"] == cr.n_components(want), what
    return want


@pytest.mark.parametrize("k,K,L,W,R", _SHAPES)
def test_components_equal_union_find_of_own_edges_on_every_path(k, K, L, W, R):
    codes = _db(k, R)
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
            got = eng.components(R, sqrt_test=sq)
            # the reference labelling is computed once per edge list: the paths return the same one
            if sq in ref and all(np.array_equal(edges[f], ref[sq][0][f]) for f in ("i", "j")):
                want = ref[sq][1]
            else:
                assert sq not in ref, what
                want = cr.labels_from_edges(n, edges["i"], edges["j"])
                ref[sq] = (edges, want)
                assert len(edges["i"]) > 1000   # (R = 171 joins everything into one component: that is a case too)
            assert got["label"].dtype == np.uint32 and np.array_equal(got["label"], want), what
            assert got["n_edges"] == len(edges["i"]), what
            assert got["n_components"] == cr.n_components(want), what
        eng.close()


def test_components_match_the_oracle_graph(oracle):
    """The graph of test_self_join_edges_match_bruteforce_within_buckets (tests/test_gpu_clustering.py), built the
    same way from the CPU oracle, labelled by the reference rule."""
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _families(np.random.default_rng(5), k, 25, 40)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    pts = oracle.embed_codes(codes)
    ints = oracle.hash_all(a, b, W, pts)
    d2 = oracle.pairwise_square(pts, pts)
    shared = np.zeros((n, n), dtype=bool)
    for l in range(L):
        keys = np.array([hsearch_amd.key_string(ints[i, l]) for i in range(n)])
        shared |= keys[:, None] == keys[None, :]
    adj = shared & (np.sqrt(d2) <= R)
    np.fill_diagonal(adj, False)
    ei, ej = np.nonzero(adj)
    want = cr.labels_from_edges(n, ei, ej)
    sizes = np.bincount(want, minlength=n)
    assert len(ei) > 1000 and (sizes >= 10).sum() >= 2 and (sizes == 1).sum() >= 1
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    got = eng.components(R, sqrt_test=True)
    eng.close()
    assert np.array_equal(got["label"], want)
    assert got["n_edges"] == len(ei) and got["n_components"] == cr.n_components(want)


def _chain(rng, k, steps):
    """c_0 .. c_steps: c_{t+1} differs from c_t at one position (position t mod k, a different residue)."""
    rows = [rng.integers(0, 20, size=k)]
    for t in range(steps):
        row = rows[-1].copy()
        row[t % k] = (row[t % k] + rng.integers(1, 20)) % 20
        rows.append(row)
    return np.array(rows, dtype=np.uint8)


def chain_case(seed=2):
    """Two disjoint chains of 200 k-mers and 40 isolated ones, ids shuffled: (codes, R, [ids of chain 0, of chain 1],
    ids of the isolated).  R is just above the longest single step, so that the edges are the near steps."""
    k = 12
    rng = np.random.default_rng(seed)
    parts = [_chain(rng, k, 199), _chain(rng, k, 199), rng.integers(0, 20, size=(40, k)).astype(np.uint8)]
    codes = np.concatenate(parts)
    pts = synth.embed(codes)
    step = max(float(np.sqrt(((pts[lo + 1:hi] - pts[lo:hi - 1]) ** 2).sum(axis=1)).max()) for lo, hi in ((0, 200), (200, 400)))
    perm = rng.permutation(len(codes))          # row perm[j] of the unshuffled list becomes id j
    where = np.empty(len(codes), dtype=np.int64)
    where[perm] = np.arange(len(codes))
    return codes[perm], step + 1e-3, [np.sort(where[0:200]), np.sort(where[200:400])], np.sort(where[400:])


@pytest.mark.parametrize("query_batch", [0, 16])
def test_chains(oracle, query_batch):
    """One table, one hash function, a bucket wide enough for everything: the graph is the R-ball graph, and a
    chain is a component that is far from a clique -- hooking order and path compression decide the result."""
    codes, R, chains, isolated = chain_case()
    n, k = codes.shape
    # brute force on the CPU: what the input must be for the test to mean something
    pts = oracle.embed_codes(codes)
    d = np.sqrt(oracle.pairwise_square(pts, pts))
    adj = d <= R
    np.fill_diagonal(adj, False)
    want = cr.labels_from_edges(n, *np.nonzero(adj))
    for c in chains:
        assert (want[c] == c[0]).all() and (want == c[0]).sum() == len(c)      # one component, nothing else in it
        assert d[np.ix_(c, c)].max() > R                                        # ... and not a clique
    assert want[chains[0][0]] != want[chains[1][0]] and d[np.ix_(chains[0], chains[1])].min() > R
    assert (want[isolated] == isolated).all()
    W = 1.0e6
    a = np.random.default_rng(1).standard_normal((1, 1, 8 * k))
    b = np.full((1, 1), W / 2)
    eng = Engine(k, 1, 1, W, a, b, options=dict(query_batch=query_batch) if query_batch else None)
    assert eng.index_build(codes)["n_buckets"] == [1]
    for sq in (True, False):
        got = eng.components(R, sqrt_test=sq)
        assert np.array_equal(got["label"], want), sq
        for c in chains:
            assert (got["label"][c] == c[0]).all()
        assert got["n_components"] == 2 + len(isolated) and got["n_edges"] == int(adj.sum())
    eng.close()


def test_duplicates_at_radius_zero():
    k, K, L, W = 25, 4, 3, 120.0
    rng = np.random.default_rng(12)
    base = synth.make_db(700, k, seed=6)
    codes = np.concatenate([base, base[rng.integers(0, 700, 500)], base[:30], base[:30]])
    rng.shuffle(codes)
    n = len(codes)
    first = {}
    want = np.array([first.setdefault(row.tobytes(), i) for i, row in enumerate(codes)], dtype=np.uint32)
    assert cr.n_components(want) == 700 and (np.bincount(want, minlength=n) >= 3).sum() >= 30
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    for sq in (True, False):
        got = eng.components(0.0, sqrt_test=sq)
        assert np.array_equal(got["label"], want) and got["n_components"] == 700
        assert got["n_edges"] == len(eng.self_join(0.0, sqrt_test=sq)["i"])
    eng.close()


def test_ranges_and_their_merge():
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _families(np.random.default_rng(6), k, 25, 40)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    full = eng.components(R)
    _check(full, n, eng.self_join(R), "full")
    cuts = [0, 1, 333, 334, n]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = eng.components(R, first=lo, count=hi - lo)
        _check(part, n, eng.self_join(R, first=lo, count=hi - lo), (lo, hi))
        parts.append(part)
    assert sum(p["n_edges"] for p in parts) == full["n_edges"] > 1000
    assert any(not np.array_equal(p["label"], full["label"]) for p in parts)
    for seed in range(3):
        order = np.random.default_rng(seed).permutation(len(parts))
        merged = capi.components_merge(np.stack([parts[i]["label"] for i in order]))
        assert np.array_equal(merged["label"], full["label"]) and merged["n_components"] == full["n_components"]
    empty = eng.components(R, first=n, count=0)   # an empty range: no edge, every k-mer labels itself
    assert np.array_equal(empty["label"], np.arange(n)) and empty["n_edges"] == 0 and empty["n_components"] == n
    eng.close()


def test_device_form_and_state():
    import torch
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _families(np.random.default_rng(7), k, 25, 40)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    qcodes = codes[::7].copy()
    before = (eng.query_codes(qcodes, R), eng.annotate(qcodes, R, codes=True))
    host = eng.components(R)
    d_label = torch.full((n,), 0x7fffffff, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n_comp, n_edges = eng.components_dev(d_label.data_ptr(), R)
    assert np.array_equal(d_label.cpu().numpy().view(np.uint32), host["label"])
    assert (n_comp, n_edges) == (host["n_components"], host["n_edges"])
    # a call at another radius in between leaves no trace: the forest starts from the identity every time
    wide, tight = eng.components(70.0, sqrt_test=False), eng.components(5.0)
    assert wide["n_components"] <= host["n_components"] < tight["n_components"] and tight["n_edges"] < host["n_edges"]
    again = eng.components(R)
    assert np.array_equal(again["label"], host["label"])
    assert (again["n_components"], again["n_edges"]) == (host["n_components"], host["n_edges"])
    after = (eng.query_codes(qcodes, R), eng.annotate(qcodes, R, codes=True))
    for x, y in zip(before, after):
        assert x.keys() == y.keys()
        for f in x:
            assert np.array_equal(x[f], y[f]), f
    assert len(before[0]["q"]) > 1000 and len(before[1]["id"]) > 100
    eng.close()


def test_errors():
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    codes = _families(np.random.default_rng(8), k, 10, 30)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    label = np.empty(n, dtype=np.uint32)
    import ctypes as C
    nc = C.c_uint64(5)
    st = eng._lib.hs_components(eng._h, R, 1, capi._vp(label), C.byref(nc), None)    # no index yet
    assert st == capi.HS_ERR_STATE and nc.value == 0
    eng.index_build(codes)
    assert eng.components(R)["n_edges"] > 100
    for first, count in ((n - 100, 101), (n + 1, 0), (0, n + 1)):
        with pytest.raises(capi.HsError) as e:
            eng.components(R, first=first, count=count)
        assert e.value.status == capi.HS_ERR_INVALID
    with pytest.raises(capi.HsError) as e:
        eng.components(float("nan"))
    assert e.value.status == capi.HS_ERR_INVALID
    eng.set_planes(*synth.make_planes(k, K, L, W, seed=4))                           # drops the index
    st = eng._lib.hs_components(eng._h, R, 1, capi._vp(label), C.byref(nc), None)
    assert st == capi.HS_ERR_STATE
    eng.index_build(codes)
    _check(eng.components(R), n, eng.self_join(R), "after new planes")
    eng.close()
