"""hs_topk_merge (host only, no GPU): the top-k rule of include/hsearch.h against tests/knn_ref.py on random tuple lists
-- repeats of a (q, id) under several tables, ties broken by id, padding tuples, -0.0, merging per-part rows against
the top-k of the union, idempotence, every invalid input with the outputs left unwritten -- the new exports, and the
argument errors of the two programs that take the new options."""
import os
import re
import subprocess

import numpy as np
import pytest

import hsearch_amd
from hsearch_amd import capi
from tests import knn_ref as kr
from tests.test_host_cli import _tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NEW = ["hs_query_topk", "hs_query_topk_dev", "hs_self_knn", "hs_self_knn_range", "hs_self_knn_dev",
        "hs_self_knn_range_dev", "hs_topk_merge"]
_TOPK = (1, 2, 5, 64)


def _random_hits(rng, nq, n_ids, m, values):
    """m distinct (q, id) pairs with distances drawn from `values` (heavy ties) and tables < 32"""
    pairs = rng.choice(nq * n_ids, size=m, replace=False)
    q, id = (pairs // n_ids).astype(np.uint32), (pairs % n_ids).astype(np.uint32)
    return q, id, rng.integers(0, 32, m).astype(np.uint32), rng.choice(values, m).astype(np.float64)


def test_library_exports_the_knn_symbols():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    declared = re.findall(r"HS_API\s+[\w\s\*]+?\b(hs_\w+)\s*\(", header)
    lib = hsearch_amd.load()
    for name in _NEW:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    assert "#define HS_TOPK_MAX 64u" in header and capi.TOPK_MAX == 64


@pytest.mark.parametrize("nq,n_ids,m,values", [(7, 40, 150, (1.0, 2.0, 2.5)), (50, 300, 4000, (0.0, 1.0, 1.5, 7.0)),
                                               (300, 20, 500, (3.0, 3.5)), (3, 500, 1200, (0.5, 1.0, 2.0, 4.0))])
def test_random_lists_with_heavy_ties(nq, n_ids, m, values):
    rng = np.random.default_rng(nq + m)
    q, id, table, dist = _random_hits(rng, nq, n_ids, m, values)
    for topk in _TOPK:
        want = kr.topk_rows(q, id, table, dist, nq, topk)
        got = capi.topk_merge(q, id, table, dist, nq, topk)
        assert kr.same_rows(got, want), topk
        assert int(got["count"].sum()) == m
        # ties are decided by id: inside a row, equal distances carry ascending ids
        d, i = got["dist"], got["id"].astype(np.int64)
        tied = (d[:, 1:] == d[:, :-1]) & np.isfinite(d[:, 1:])
        assert (i[:, 1:][tied] > i[:, :-1][tied]).all()
        if topk > 1 and len(values) < 4:
            assert tied.any()
        p = rng.permutation(m)                                  # any order of the input
        assert kr.same_rows(capi.topk_merge(q[p], id[p], table[p], dist[p], nq, topk), want), topk
    if nq == 3:
        assert (np.bincount(q, minlength=nq) > 64).all()        # (rows longer than the widest topk)


def test_repeats_of_a_pair_keep_the_smallest_table():
    rng = np.random.default_rng(5)
    nq, topk = 9, 4
    q, id, table, dist = _random_hits(rng, nq, 30, 120, (1.0, 2.0, 3.0))
    want = kr.topk_rows(q, id, np.minimum(table, 3), dist, nq, topk)
    # every tuple three times: once with its table cut at 3 and twice with larger ones
    q3, id3, d3 = np.tile(q, 3), np.tile(id, 3), np.tile(dist, 3)
    t3 = np.concatenate([table + 4, np.minimum(table, 3), table + 9]).astype(np.uint32)
    p = rng.permutation(len(q3))
    got = capi.topk_merge(q3[p], id3[p], t3[p], d3[p], nq, topk)
    assert kr.same_rows(got, want)
    assert np.array_equal(got["count"], np.bincount(q, minlength=nq))          # distinct ids, not tuples


def test_ties_are_broken_by_id_and_padding_is_skipped():
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    q, id = u32(0, 0, 0, 0, 1, 1), u32(9, 3, 7, capi.NO_ID, capi.NO_ID, 2)
    table, dist = u32(1, 2, 0, capi.NO_ID, 5, 4), np.array([1.0, 1.0, 0.5, np.inf, 0.25, 2.0])
    got = capi.topk_merge(q, id, table, dist, 3, 3)
    assert got["id"].tolist() == [[7, 3, 9], [2, capi.NO_ID, capi.NO_ID], [capi.NO_ID] * 3]
    assert got["table"].tolist() == [[0, 2, 1], [4, capi.NO_ID, capi.NO_ID], [capi.NO_ID] * 3]
    assert got["dist"].tolist() == [[0.5, 1.0, 1.0], [2.0, np.inf, np.inf], [np.inf] * 3]
    assert got["count"].tolist() == [3, 1, 0]
    # a padding tuple is skipped whatever else it carries: a q outside the rows, a NaN
    got2 = capi.topk_merge(u32(0, 77), u32(4, capi.NO_ID), u32(1, 0), np.array([1.0, np.nan]), 1, 2)
    assert got2["id"].tolist() == [[4, capi.NO_ID]] and got2["count"].tolist() == [1]


def test_no_table_array():
    """table == NULL: the rows are those of the same tuples, their tables all 0xffffffff; repeats still count once."""
    rng = np.random.default_rng(8)
    nq = 12
    q, id, table, dist = _random_hits(rng, nq, 50, 300, (1.0, 2.0, 3.0))
    for topk in (1, 5, 64):
        want = capi.topk_merge(q, id, table, dist, nq, topk)
        got = capi.topk_merge(np.tile(q, 2), np.tile(id, 2), None, np.tile(dist, 2), nq, topk)
        assert kr.same_rows(got, want, tables=False), topk
        assert np.array_equal(got["table"], np.full((nq, topk), capi.NO_ID, dtype=np.uint32)), topk


def test_negative_zero_is_read_as_zero():
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    got = capi.topk_merge(u32(0, 0, 0, 0), u32(5, 2, 5, 8), u32(3, 1, 2, 0), np.array([-0.0, 0.0, 0.0, 1.0]), 1, 3)
    assert got["id"].tolist() == [[2, 5, 8]] and got["table"].tolist() == [[1, 2, 0]]   # (5 given twice: one distance)
    assert not np.signbit(got["dist"]).any() and got["dist"].tolist() == [[0.0, 0.0, 1.0]]
    assert got["count"].tolist() == [3]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_merging_the_parts_rows_is_the_topk_of_the_union(seed):
    rng = np.random.default_rng(seed)
    nq, m = 40, 3000
    q, id, table, dist = _random_hits(rng, nq, 200, m, (0.0, 1.0, 1.5, 2.0, 4.0))
    for topk in (1, 5, 64):
        whole = capi.topk_merge(q, id, table, dist, nq, topk)
        part = rng.integers(0, 4, m)                               # a random split into four parts, one of them small
        part[rng.random(m) < 0.5] = 0
        rows = [capi.topk_merge(q[part == p], id[part == p], table[part == p], dist[part == p], nq, topk)
                for p in range(4)]
        cat = [np.concatenate(x) for x in zip(*(kr.flatten(r) for r in rows))]
        merged = capi.topk_merge(*cat, nq, topk)
        for f in ("id", "table"):
            assert np.array_equal(merged[f], whole[f]), (topk, f)
        assert np.array_equal(merged["dist"].view(np.uint64), whole["dist"].view(np.uint64)), topk
        # the count over rows that were cut is a lower bound, exact where no part's row was cut
        assert (merged["count"] <= whole["count"]).all()
        uncut = np.all([r["count"] <= topk for r in rows], axis=0)
        assert np.array_equal(merged["count"][uncut], whole["count"][uncut])
        # overlapping parts (a table partition reports a pair from several ranks): the smallest table wins
        again = capi.topk_merge(*[np.concatenate([c, c]) for c in cat], nq, topk)
        assert kr.same_rows(again, merged), topk
        # idempotence: a result fed back in is itself
        once = capi.topk_merge(*kr.flatten(whole), nq, topk)
        for f in ("id", "table"):
            assert np.array_equal(once[f], whole[f]), (topk, f)
        assert np.array_equal(once["dist"].view(np.uint64), whole["dist"].view(np.uint64))
        assert np.array_equal(once["count"], np.minimum(whole["count"], topk))


def _untouched_out(nq, topk):
    return dict(id=np.full((nq, topk), 77, dtype=np.uint32), table=np.full((nq, topk), 78, dtype=np.uint32),
                dist=np.full((nq, topk), 7.5), count=np.full(nq, 79, dtype=np.uint32))


def test_invalid_inputs_leave_the_outputs_unwritten():
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    nq = 3
    good = (u32(0, 1, 1, 2), u32(4, 5, 6, 4), u32(0, 1, 2, 3), np.array([1.0, 2.0, 0.5, 1.0]))
    bad = {"q >= nq": (u32(0, 3, 1, 2), *good[1:], 2),
           "NaN": (*good[:3], np.array([1.0, np.nan, 0.5, 1.0]), 2),
           "negative": (*good[:3], np.array([1.0, 2.0, -0.5, 1.0]), 2),
           "one pair, two distances": (u32(0, 1, 1, 1), u32(4, 5, 6, 5), good[2], np.array([1.0, 2.0, 0.5, 2.5]), 2),
           "one pair, two distances one ulp apart": (u32(0, 1, 1, 1), u32(4, 5, 6, 5), good[2],
                                                     np.array([1.0, 2.0, 0.5, np.nextafter(2.0, 3.0)]), 2),
           "topk = 0": (*good, 0),
           "topk = 65": (*good, 65)}
    for what, (q, id, table, dist, topk) in bad.items():
        rows = min(max(topk, 1), 64)
        out = _untouched_out(nq, rows)
        with pytest.raises(capi.HsError) as e:
            capi.topk_merge(q, id, table, dist, nq, topk, out=out)
        assert e.value.status == capi.HS_ERR_INVALID, what
        assert (out["id"] == 77).all() and (out["table"] == 78).all() and (out["dist"] == 7.5).all(), what
        assert (out["count"] == 79).all(), what
    got = capi.topk_merge(*good, nq, 2)
    assert got["id"].tolist() == [[4, capi.NO_ID], [6, 5], [4, capi.NO_ID]] and got["count"].tolist() == [1, 2, 1]
    # +inf is a distance like any other (a padded row's own entries are skipped by their id, not by it)
    got = capi.topk_merge(u32(0), u32(4), u32(1), np.array([np.inf]), 1, 1)
    assert got["id"].tolist() == [[4]] and got["count"].tolist() == [1]


def test_empty_cases():
    none = np.empty(0, dtype=np.uint32)
    for nq in (0, 1, 4):
        got = capi.topk_merge(none, none, none, np.empty(0), nq, 3)
        assert got["id"].shape == (nq, 3) and (got["id"] == capi.NO_ID).all() and (got["table"] == capi.NO_ID).all()
        assert np.isinf(got["dist"]).all() and (got["count"] == 0).all()
    with pytest.raises(capi.HsError):
        capi.topk_merge([0], [1], [0], [1.0], 0, 2)                           # any q is >= nq = 0


def test_argument_errors_of_the_programs(tmp_path):
    """--topk and -knn are refused from the arguments alone: before any file is read or a device opened."""
    out = str(tmp_path / "out.txt")
    search = [_tool("hs_motif_both_points"), "-d", str(tmp_path / "none.db"), "-c", str(tmp_path / "none.centers"),
              "-o", out, "-l", "25", "-K", "4", "-L", "3", "-W", "120", "-T", "50"]
    for extra, word in ((["--topk", "0"], "--topk"), (["--topk", "65"], "--topk"), (["--topk", "x"], "--topk"),
                        (["--topk", "3", "--gpus", "2"], "--gpus"),
                        (["--topk", "3", "--best-per-position", "1"], "--best-per-position")):
        r = subprocess.run(search + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--topk" in r.stderr and word in r.stderr, (extra, r.stderr)
        assert not os.path.exists(out), extra
    clust = [_tool("hs_hclust2"), "-k", str(tmp_path / "none.fa"), "-l", "25", "-K", "4", "-L", "3", "-W", "120",
             "-T", "50", "-o", out]
    for extra, word in ((["-linkage", "single", "-knn", "0"], "-knn"), (["-linkage", "single", "-knn", "65"], "-knn"),
                        (["-linkage", "dbscan", "-minpts", "3", "-knn", "abc"], "-knn"), (["-knn", "4"], "-linkage")):
        r = subprocess.run(clust + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "-knn" in r.stderr and word in r.stderr, (extra, r.stderr)
        assert not os.path.exists(out) and not os.path.exists(out + "hclust.knn.txt"), extra
