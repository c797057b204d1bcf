"""hs_self_knn / hs_query_topk on the GPU: the topk best hits per query, selected on the device, against the numpy rule
(tests/knn_ref.py) applied to the list the underlying call returns on the same handle -- every filter path, both hit
tests, segments of every length around topk and around the 64 entries of a chunk, ties decided by id, every batch cut,
points / codes / recognised centres / per-query radii / multi-probe / bucket partitions -- plus the two identities with
hs_degrees and hs_core_distance, the device forms, the errors, and that no other entry point moved.  Every comparison
is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import knn_ref as kr
from tests import radii_ref as rr
from tests.test_gpu_clustering import _families
from tests.test_gpu_components import _PATHS, _SHAPES, _db

pytestmark = pytest.mark.gpu

_TOPK = (1, 5, 64)


def _qcase(nq=300):
    """The family data of the graph tests as a database (tens of hits per query at R = 50), queries drawn from it as
    codes and as jittered points: (k, K, L, W, R, a, b, codes, qcodes, centers)"""
    k, K, L, W, R = _SHAPES[0]
    codes = _db(k, R)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    qcodes, _ = synth.make_query_codes(codes, nq, seed=7)
    centers, _ = synth.make_queries(codes, nq, jitter=0.25, seed=9)
    return k, K, L, W, R, a, b, codes, qcodes, centers


def _edge_rows(edges, n, topk, first=0):
    return kr.topk_rows(edges["i"].astype(np.int64) - first, edges["j"], edges["table"], edges["dist"], n, topk)


def _hit_rows(hits, nq, topk):
    return kr.topk_rows(hits["q"], hits["id"], hits["table"], hits["dist"], nq, topk)


def _tie_carriers(edges, n):
    """k-mers with two neighbours at one distance"""
    bits = edges["dist"].view(np.uint64)
    order = np.lexsort((bits, edges["i"]))
    i, d = edges["i"][order], bits[order]
    same = (i[1:] == i[:-1]) & (d[1:] == d[:-1])
    return len(np.unique(i[1:][same]))


@pytest.mark.parametrize("k,K,L,W,R", _SHAPES)
def test_self_knn_is_the_rule_on_own_edges_on_every_path(k, K, L, W, R):
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
            # the reference rows are computed once per edge list: the paths return the same one
            if sq in ref and all(np.array_equal(edges[f], ref[sq][0][f]) for f in ("i", "j", "table")) and \
                    np.array_equal(edges["dist"].view(np.uint64), ref[sq][0]["dist"].view(np.uint64)):
                want = ref[sq][1]
            else:
                assert sq not in ref, (mode, opts, sq)
                degree = np.bincount(edges["i"], minlength=n)
                if R == 171.0:
                    assert (degree > 128).sum() > 2000          # segments of many chunks
                else:
                    assert _tie_carriers(edges, n) > 500        # ties decided by id
                want = {topk: _edge_rows(edges, n, topk) for topk in _TOPK}
                ref[sq] = (edges, want)
            for topk in _TOPK:
                got = eng.self_knn(R, topk, sqrt_test=sq)
                assert kr.same_rows(got, want[topk]), (mode, opts, sq, topk)
                assert got["n_edges"] == len(edges["i"]), (mode, opts, sq, topk)
        eng.close()


_CLIQUES = (2, 5, 6, 7, 64, 65, 66, 130)


def _clique_case():
    """Cliques of identical copies of one k-mer among 300 random 25-mers, ids shuffled: (codes, the cliques' k-mers)"""
    k = 25
    rng = np.random.default_rng(77)
    base = synth.make_db(len(_CLIQUES), k, seed=78)
    lone = synth.make_db(300, k, seed=79)
    assert len(np.unique(np.concatenate([base, lone]), axis=0)) == len(base) + len(lone)
    codes = np.concatenate([lone] + [np.repeat(base[c:c + 1], m, axis=0) for c, m in enumerate(_CLIQUES)])
    rng.shuffle(codes)
    return codes, base


def test_exact_segment_lengths_on_cliques():
    """Identical k-mers share every bucket whatever the planes are; at R = 0 nothing else is a hit.  Segments of
    topk - 1, topk, topk + 1 entries for topk = 5 and 64, and of 129: three chunks with one entry in the last."""
    k, K, L, W, _ = _SHAPES[0]
    R = 0.0
    codes, base = _clique_case()
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    members = [np.flatnonzero((codes == kmer).all(axis=1)) for kmer in base]
    assert [len(m) for m in members] == list(_CLIQUES)
    in_clique = np.zeros(n, dtype=bool)
    in_clique[np.concatenate(members)] = True
    for sq in (True, False):
        edges = eng.self_join(R, sqrt_test=sq)
        assert len(edges["i"]) == sum(m * (m - 1) for m in _CLIQUES) and (edges["dist"] == 0.0).all()
        for topk in (5, 64):
            got = eng.self_knn(R, topk, sqrt_test=sq)
            assert kr.same_rows(got, _edge_rows(edges, n, topk)), (sq, topk)
            for ids in members:
                for i in ids:
                    others = ids[ids != i][:topk]                  # the other copies in id order
                    assert got["id"][i, :len(others)].tolist() == others.tolist(), (sq, topk, len(ids))
                    assert (got["id"][i, len(others):] == capi.NO_ID).all() and got["count"][i] == len(ids) - 1
                    assert (got["dist"][i, :len(others)].view(np.uint64) == 0).all()
            # a k-mer with no neighbours: a row of padding, count 0
            assert (got["count"][~in_clique] == 0).all() and (got["id"][~in_clique] == capi.NO_ID).all()
            assert (got["table"][~in_clique] == capi.NO_ID).all() and np.isposinf(got["dist"][~in_clique]).all()
    # the same cliques as queries (segments of 2, 5, 6, 7, 64, 65, 66, 130), and a query that hits nothing
    queries = np.concatenate([base, synth.make_db(1, k, seed=80)])
    hits = eng.query_codes(queries, R)
    assert np.bincount(hits["q"], minlength=len(queries)).tolist() == list(_CLIQUES) + [0]
    for topk in (5, 64):
        got = eng.query_topk(queries, topk, R=R, codes=True)
        assert kr.same_rows(got, _hit_rows(hits, len(queries), topk)), topk
        assert got["n_hits"] == len(hits["q"]) and got["count"].tolist() == list(_CLIQUES) + [0]
        for c, ids in enumerate(members):
            assert got["id"][c, :min(topk, len(ids))].tolist() == ids[:topk].tolist()
        assert (got["id"][-1] == capi.NO_ID).all() and np.isposinf(got["dist"][-1]).all()
    eng.close()


def test_the_two_identities_with_degrees_and_core_distances():
    """The multiplicity data of tests/test_gpu_density.py: five copies of one k-mer and three of another in a family."""
    k, K, L, W, R = 25, 4, 3, 120.0, 50.0
    topk = 8
    rng = np.random.default_rng(21)
    fam = _families(rng, k, 12, 30, max_sub=2)
    _, inv, cnt = np.unique(fam, axis=0, return_inverse=True, return_counts=True)
    single = np.flatnonzero(cnt[inv.ravel()] == 1)
    x, y = int(single[0]), int(single[single >= 40][0])
    codes = np.concatenate([fam, np.repeat(fam[x:x + 1], 4, axis=0), np.repeat(fam[y:y + 1], 2, axis=0),
                            synth.make_db(300, k, seed=5)])
    rng.shuffle(codes)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    for sq in (True, False):
        got = eng.self_knn(R, topk, sqrt_test=sq)
        degree = eng.degrees(R, sqrt_test=sq)
        assert np.array_equal(got["count"], degree) and got["n_edges"] == int(degree.sum())
        assert (degree == 0).any() and (degree > topk).any()
        for m in (2, 3, 5, 8, 9):
            core = eng.core_distance(R, m, sqrt_test=sq)["core"]
            assert np.array_equal(got["dist"][:, m - 2].view(np.uint64), core.view(np.uint64)), (sq, m)
            assert np.array_equal(np.isposinf(core), degree < m - 1), (sq, m)
    assert (got["dist"][:, 0] == 0.0).sum() >= 8                      # the copies see each other at distance 0
    eng.close()


def test_batch_cuts(monkeypatch):
    """Batches of 1, 16 and 37 queries, batches cut in halves by the test build, ranges: the rows of the uncut call."""
    k, K, L, W, R = _SHAPES[0]
    codes = _db(k, R)
    n = len(codes)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    edges = eng.self_join(R)
    want = {topk: _edge_rows(edges, n, topk) for topk in (5, 64)}
    for topk in (5, 64):
        assert kr.same_rows(eng.self_knn(R, topk), want[topk]), topk
    for qb in (1, 16, 37):
        eng.set_option("query_batch", qb)
        for topk in (5, 64):
            got = eng.self_knn(R, topk)
            assert kr.same_rows(got, want[topk]) and got["n_edges"] == len(edges["i"]), (qb, topk)
    eng.set_option("query_batch", 0)
    # ranges: row t is k-mer first + t; the shares concatenate to the whole
    lo, hi = eng.self_knn(R, 5, first=0, count=1000), eng.self_knn(R, 5, first=1000)
    assert lo["id"].shape == (1000, 5) and hi["id"].shape == (n - 1000, 5)
    both = {f: np.concatenate([lo[f], hi[f]]) for f in ("id", "table", "dist", "count")}
    assert kr.same_rows(both, want[5]) and lo["n_edges"] + hi["n_edges"] == len(edges["i"])
    part = eng.self_join(R, first=1000)
    assert kr.same_rows(hi, _edge_rows(part, n - 1000, 5, first=1000))
    none = eng.self_knn(R, 5, first=n, count=0)
    assert none["id"].shape == (0, 5) and none["n_edges"] == 0
    eng.close()
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "100")
    eng = Engine(k, K, L, W, a, b, hooks=True)
    eng.index_build(codes)
    for topk in (5, 64):
        got = eng.self_knn(R, topk)
        assert kr.same_rows(got, want[topk]) and got["n_edges"] == len(edges["i"]), topk
    assert eng.profile()["verify_launches"] >= n // 100
    eng.close()


def test_query_topk_is_the_rule_on_the_matching_list_call():
    k, K, L, W, R, a, b, codes, qcodes, centers = _qcase()
    nq = len(centers)
    radii = rr.draw_radii(k, nq).copy()
    radii[5], radii[77] = -40.0, -0.0                              # a negative radius behaves as in the scalar call
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    for T in (0, 4):
        eng.set_multiprobe(T)
        for qb in (0, 37):
            eng.set_option("query_batch", qb)
            lists = {"points": (eng.query(centers, R), dict(queries=centers, R=R)),
                     "codes": (eng.query_codes(qcodes, R), dict(queries=qcodes, R=R, codes=True)),
                     "k-mer centres": (eng.query_codes(qcodes, R), dict(queries=synth.embed(qcodes), R=R)),
                     "radii": (eng.query_radii(centers, radii), dict(queries=centers, radii=radii)),
                     "radii codes": (eng.query_radii(qcodes, radii, codes=True),
                                     dict(queries=qcodes, radii=radii, codes=True))}
            for what, (hits, args) in lists.items():
                assert len(hits["q"]) > 2 * nq, what
                for topk in (1, 10, 64):
                    got = eng.query_topk(topk=topk, **args)
                    assert kr.same_rows(got, _hit_rows(hits, nq, topk)), (T, qb, what, topk)
                    assert got["n_hits"] == len(hits["q"]) == int(got["count"].sum()), (T, qb, what, topk)
                if what == "k-mer centres" and T == 0:
                    assert eng.profile()["queries_recognised"] == nq
            counts = np.bincount(lists["codes"][0]["q"], minlength=nq)
            assert (counts > 10).sum() > 20 and (counts < 10).sum() > 20     # rows cut at topk = 10, rows padded
        eng.set_option("query_batch", 0)
    eng.set_multiprobe(0)
    # bucket partition: every part's rows are the rule on that part's list, and merged they are the whole's
    for topk in (3, 64):
        whole = eng.query_topk(qcodes, topk, R=R, codes=True)
        parts = []
        for part in range(3):
            eng.set_bucket_partition(part, 3)
            parts.append(eng.query_topk(qcodes, topk, R=R, codes=True))
            assert kr.same_rows(parts[-1], _hit_rows(eng.query_codes(qcodes, R), nq, topk)), (topk, part)
            assert parts[-1]["n_hits"] > 0
        eng.set_bucket_partition(0, 1)
        merged = capi.topk_merge(*[np.concatenate(x) for x in zip(*(kr.flatten(p) for p in parts))], nq, topk)
        for f in ("id", "table"):
            assert np.array_equal(merged[f], whole[f]), (topk, f)
        assert np.array_equal(merged["dist"].view(np.uint64), whole["dist"].view(np.uint64)), topk
        assert (merged["count"] <= whole["count"]).all()
    eng.close()


def _a5(torch, nbytes):
    return torch.full((max(nbytes, 8),), 0xA5, dtype=torch.uint8, device="cuda")


def _dev_rows(bufs, rows, topk):
    d_id, d_t, d_d, d_c = bufs
    e = rows * topk
    return dict(id=d_id[:e * 4].cpu().numpy().view(np.uint32).reshape(rows, topk),
                table=d_t[:e * 4].cpu().numpy().view(np.uint32).reshape(rows, topk),
                dist=d_d[:e * 8].cpu().numpy().view(np.float64).reshape(rows, topk),
                count=d_c[:rows * 4].cpu().numpy().view(np.uint32))


def test_dev_forms_define_every_word():
    import torch
    k, K, L, W, R, a, b, codes, qcodes, centers = _qcase()
    nq, n = len(centers), len(codes)
    radii = rr.draw_radii(k, nq)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    for topk in (1, 7, 64):
        for queries, codes_in, rad in ((centers, False, None), (qcodes, True, None), (centers, False, radii)):
            want = eng.query_topk(queries, topk, R=None if rad is not None else R, radii=rad, codes=codes_in)
            d_in = torch.from_numpy(queries).cuda()
            d_r = torch.from_numpy(rad).cuda() if rad is not None else None
            bufs = [_a5(torch, nq * topk * 4), _a5(torch, nq * topk * 4), _a5(torch, nq * topk * 8), _a5(torch, nq * 4)]
            torch.cuda.synchronize()
            nh = eng.query_topk_dev(d_in.data_ptr(), nq, topk, R, d_r.data_ptr() if d_r is not None else None,
                                    *[t.data_ptr() for t in bufs], codes=codes_in)
            got = _dev_rows(bufs, nq, topk)
            assert kr.same_rows(got, want) and nh == want["n_hits"], (topk, codes_in, rad is not None)
        # the k-nearest-neighbour graph, whole and as a range, with and without the tables
        Rs = R
        want = eng.self_knn(Rs, topk)
        assert want["n_edges"] > 0 and (want["count"] == 0).any()
        bufs = [_a5(torch, n * topk * 4), _a5(torch, n * topk * 4), _a5(torch, n * topk * 8), _a5(torch, n * 4)]
        torch.cuda.synchronize()
        ne = eng.self_knn_dev(*[t.data_ptr() for t in bufs], Rs, topk)
        assert kr.same_rows(_dev_rows(bufs, n, topk), want) and ne == want["n_edges"], topk
        first, count = 1234, 1000
        bufs = [_a5(torch, count * topk * 4), _a5(torch, 64), _a5(torch, count * topk * 8), _a5(torch, count * 4)]
        torch.cuda.synchronize()
        ne = eng.self_knn_dev(bufs[0].data_ptr(), None, bufs[2].data_ptr(), bufs[3].data_ptr(), Rs, topk, first=first,
                              count=count)
        got = _dev_rows([bufs[0], bufs[0], bufs[2], bufs[3]], count, topk)
        share = {f: want[f][first:first + count] for f in ("id", "table", "dist", "count")}
        assert kr.same_rows(got, share, tables=False) and ne == int(share["count"].sum()), topk
        assert bool((bufs[1] == 0xA5).all())                   # no table array: none written
    eng.close()


def test_errors_and_edges():
    import torch
    k, K, L, W, R, a, b, codes, qcodes, centers = _qcase(nq=60)
    nq, n = len(centers), len(codes)
    eng = Engine(k, K, L, W, a, b)
    lib, h = eng._lib, eng._h
    topk = 4
    out = [np.full((n, topk), 77, dtype=np.uint32), np.full((n, topk), 78, dtype=np.uint32), np.full((n, topk), 7.5),
           np.full(n, 79, dtype=np.uint32)]
    ptrs = [capi._vp(x) for x in out]
    untouched = lambda: (out[0] == 77).all() and (out[1] == 78).all() and (out[2] == 7.5).all() and (out[3] == 79).all()
    nh = C.c_uint64(5)
    # an index that was never built
    assert lib.hs_query_topk(h, capi._vp(centers), None, nq, R, None, topk, *ptrs, C.byref(nh)) == capi.HS_ERR_STATE
    assert lib.hs_self_knn(h, R, 1, topk, *ptrs, C.byref(nh)) == capi.HS_ERR_STATE
    assert nh.value == 0 and untouched()
    with pytest.raises(capi.HsError) as e:
        eng.self_knn(R, topk)
    assert e.value.status == capi.HS_ERR_STATE
    eng.index_build(codes)
    nan_r = np.full(nq, R)
    nan_r[nq // 2] = np.nan
    cases = {"topk = 0": lambda: lib.hs_query_topk(h, capi._vp(centers), None, nq, R, None, 0, *ptrs, C.byref(nh)),
             "topk = 65": lambda: lib.hs_query_topk(h, capi._vp(centers), None, nq, R, None, 65, *ptrs, C.byref(nh)),
             "self topk = 0": lambda: lib.hs_self_knn(h, R, 1, 0, *ptrs, C.byref(nh)),
             "self topk = 65": lambda: lib.hs_self_knn_range(h, 0, n, R, 1, 65, *ptrs, C.byref(nh)),
             "NaN R": lambda: lib.hs_query_topk(h, capi._vp(centers), None, nq, float("nan"), None, topk, *ptrs,
                                                C.byref(nh)),
             "self NaN R": lambda: lib.hs_self_knn(h, float("nan"), 1, topk, *ptrs, C.byref(nh)),
             "NaN radius": lambda: lib.hs_query_topk(h, capi._vp(centers), None, nq, R, capi._vp(nan_r), topk, *ptrs,
                                                     C.byref(nh)),
             "both": lambda: lib.hs_query_topk(h, capi._vp(centers), capi._vp(qcodes), nq, R, None, topk, *ptrs,
                                               C.byref(nh)),
             "neither": lambda: lib.hs_query_topk(h, None, None, nq, R, None, topk, *ptrs, C.byref(nh)),
             "range outside": lambda: lib.hs_self_knn_range(h, n - 5, 6, R, 1, topk, *ptrs, C.byref(nh))}
    for what, call in cases.items():
        nh.value = 5
        assert call() == capi.HS_ERR_INVALID, what
        assert nh.value == 0 and untouched(), what
    # the device forms: a NaN radius is found on the device, before any output is written
    bufs = [_a5(torch, nq * topk * 4), _a5(torch, nq * topk * 4), _a5(torch, nq * topk * 8), _a5(torch, nq * 4)]
    d_in, d_r = torch.from_numpy(centers).cuda(), torch.from_numpy(nan_r).cuda()
    torch.cuda.synchronize()
    for r_ptr, R_arg, tk in ((d_r.data_ptr(), R, topk), (None, float("nan"), topk), (None, R, 0), (None, R, 65)):
        with pytest.raises(capi.HsError) as e:
            eng.query_topk_dev(d_in.data_ptr(), nq, tk, R_arg, r_ptr, *[t.data_ptr() for t in bufs])
        assert e.value.status == capi.HS_ERR_INVALID
        assert all(bool((t == 0xA5).all()) for t in bufs)
    # a query code outside the alphabet, in a late batch: an error, nothing written by the host form
    broken = qcodes.copy()
    broken[-3, 4] = 31
    eng.set_option("query_batch", 7)
    assert lib.hs_query_topk(h, None, capi._vp(broken), nq, R, None, topk, *ptrs, C.byref(nh)) == capi.HS_ERR_INVALID
    assert untouched()
    eng.set_option("query_batch", 0)
    # no query: success, nothing written; a radius that yields no hit: rows of padding
    got = eng.query_topk(centers[:0], topk, R=R)
    assert got["id"].shape == (0, topk) and got["count"].shape == (0,) and got["n_hits"] == 0
    got = eng.query_topk(qcodes[:0], topk, radii=np.empty(0), codes=True)
    assert got["id"].shape == (0, topk) and got["n_hits"] == 0
    assert lib.hs_query_topk(h, capi._vp(centers), None, 0, R, None, topk, None, None, None, None,
                             C.byref(nh)) == capi.HS_OK
    assert len(eng.query(centers, 0.0)["q"]) == 0
    got = eng.query_topk(centers, topk, R=0.0)
    assert (got["id"] == capi.NO_ID).all() and (got["table"] == capi.NO_ID).all() and np.isposinf(got["dist"]).all()
    assert (got["count"] == 0).all() and got["n_hits"] == 0
    # nn_table may be NULL
    want = eng.query_topk(centers, topk, R=R)
    assert lib.hs_query_topk(h, capi._vp(centers), None, nq, R, None, topk, ptrs[0], None, ptrs[2], ptrs[3],
                             C.byref(nh)) == capi.HS_OK
    assert np.array_equal(out[0][:nq], want["id"]) and (out[1] == 78).all() and nh.value == want["n_hits"]
    assert np.array_equal(out[2][:nq].view(np.uint64), want["dist"].view(np.uint64))
    assert np.array_equal(out[3][:nq], want["count"]) and (out[3][nq:] == 79).all()
    eng.close()


def test_nothing_else_moved():
    k, K, L, W, R, a, b, codes, qcodes, centers = _qcase(nq=200)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    Rs = R

    def snapshot():
        return [eng.query(centers, R), eng.query_codes(qcodes, R), eng.self_join(Rs), eng.core_distance(Rs, 3),
                eng.annotate(centers, R), dict(degree=eng.degrees(Rs))]

    def same(x, y):
        return all(set(p) == set(q) and all(np.array_equal(p[f], q[f]) for f in p) for p, q in zip(x, y))

    before = snapshot()
    assert len(before[0]["q"]) > 0 and len(before[2]["i"]) > 0
    first = eng.self_knn(Rs, 10)
    top = eng.query_topk(centers, 10, R=R)
    middle = snapshot()
    assert same(before, middle)
    # ... and the top-k calls are themselves a function of their arguments alone
    assert kr.same_rows(eng.self_knn(Rs, 10), first) and kr.same_rows(eng.query_topk(centers, 10, R=R), top)
    assert kr.same_rows(eng.query_topk(centers, 3, R=R), {f: (top[f][:, :3] if top[f].ndim == 2 else top[f])
                                                            for f in ("id", "table", "dist", "count")})
    # a rebuilt, smaller index on the same handle
    eng.index_build(codes[:2000])
    got = eng.self_knn(Rs, 10)
    assert got["id"].shape == (2000, 10) and kr.same_rows(got, _edge_rows(eng.self_join(Rs), 2000, 10))
    eng.close()
