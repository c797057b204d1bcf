"""hs_dbscan_edges (host only, no GPU): the DBSCAN rule of include/hsearch.h applied to an edge list, against the plain
Python of tests/dbscan_ref.py -- on random graphs given in every form an edge list can take, on hand-built cases that
pin the border rule, and on invalid inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hsearch_amd
from hsearch_amd import capi
from tests import components_ref as cr
from tests import dbscan_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NEW = ("hs_degrees", "hs_degrees_dev", "hs_degrees_range", "hs_degrees_range_dev", "hs_dbscan", "hs_dbscan_dev",
        "hs_dbscan_edges")


def test_header_declares_and_library_exports():
    text = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in _NEW:
        assert re.search(r"HS_API\s+hs_status\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
    assert re.search(r"#define\s+HS_NOISE\s+0xffffffffu", text)
    assert capi.NOISE == dr.NOISE == 0xffffffff
    assert hsearch_amd.dbscan_edges is capi.dbscan_edges
    for name in ("degrees", "degrees_dev", "dbscan", "dbscan_dev"):
        assert callable(getattr(capi.Engine, name))


def _graph(seed, n, m):
    """m random pairs over n vertices, drawn so that dense spots and sparse ones both occur (one direction)."""
    rng = np.random.default_rng(seed)
    if n == 0 or m == 0:
        return np.empty(0, dtype=np.uint32), np.empty(0, dtype=np.uint32)
    ei = rng.integers(0, n, m)
    near = rng.random(m) < 0.95   # most pairs stay inside a window of ids: cliques-ish, with cores; the rest is far
    ej = np.where(near, np.minimum(n - 1, ei // 8 * 8 + rng.integers(0, 8, m)), rng.integers(0, n, m))
    return ei.astype(np.uint32), ej.astype(np.uint32)


def _forms(seed, ei, ej, n):
    """The same graph as one direction, both, shuffled, with repeats, with self pairs."""
    rng = np.random.default_rng(seed)
    m = len(ei)
    yield "one direction", ei, ej
    yield "the other direction", ej, ei
    bi, bj = np.concatenate([ei, ej]), np.concatenate([ej, ei])
    yield "both directions", bi, bj
    p = rng.permutation(2 * m)
    yield "shuffled", bi[p], bj[p]
    if m:
        r = rng.integers(0, m, m)
        flip = rng.random(m) < 0.5
        ri, rj = np.where(flip, ej[r], ei[r]), np.where(flip, ei[r], ej[r])
        yield "with repeats", np.concatenate([ei, ri]).astype(np.uint32), np.concatenate([ej, rj]).astype(np.uint32)
    if n:
        s = rng.integers(0, n, 5).astype(np.uint32)
        q = rng.permutation(m + 5)
        yield "with self pairs", np.concatenate([ei, s])[q], np.concatenate([ej, s])[q]


@pytest.mark.parametrize("n", [0, 1, 2, 600])
@pytest.mark.parametrize("density", [0, 1, 2, 3])
def test_edges_equal_reference_rule_in_every_form(n, density):
    m = {0: 0, 1: n // 2, 2: n + 1 if n else 0, 3: 3 * n}[density]
    ei, ej = _graph(10 * n + density, n, m)
    distinct = len({(min(x, y), max(x, y)) for x, y in zip(ei.tolist(), ej.tolist()) if x != y})
    for min_pts in (1, 2, 3, 5, n + 2):
        want = dr.dbscan_from_edges(n, ei, ej, min_pts)
        assert want["n_edges"] == 2 * distinct
        for what, fi, fj in _forms(n + min_pts, ei, ej, n):
            got = capi.dbscan_edges(fi, fj, n, min_pts, want_degree=True)
            dr.assert_same(got, want, (what, min_pts))
            dr.check_invariants(got, n, min_pts)
            plain = capi.dbscan_edges(fi, fj, n, min_pts)            # the degree array may be left out
            assert "degree" not in plain and np.array_equal(plain["label"], want["label"])
        if min_pts == 1:
            assert np.array_equal(want["label"], cr.labels_from_edges(n, ei, ej))
            assert want["n_clusters"] == cr.n_components(want["label"]) and want["n_core"] == n
        if min_pts == 2:   # the components with the singletons turned into noise
            comp = cr.labels_from_edges(n, ei, ej)
            alone = np.bincount(comp, minlength=n)[comp] == 1 if n else np.zeros(0, dtype=bool)
            assert np.array_equal(want["label"], np.where(alone, dr.NOISE, comp))
        if min_pts == n + 2:
            assert (want["label"] == dr.NOISE).all() and want["n_clusters"] == 0 and want["n_noise"] == n
    if n == 600 and density == 3:   # the input has all three kinds and several clusters
        want = dr.dbscan_from_edges(n, ei, ej, 5)
        assert want["n_clusters"] >= 2 and min(want["n_core"], want["n_border"], want["n_noise"]) >= 10


def _clique(ids):
    return [(x, y) for t, x in enumerate(ids) for y in ids[t + 1:]]


def test_border_takes_the_smallest_core_neighbour_not_the_smallest_label():
    a_ids, b_ids, x = [0, 9, 10, 11], [3, 4, 5, 6], 7
    pairs = _clique(a_ids) + _clique(b_ids) + [(x, 9), (3, x)]
    ei, ej = np.array(pairs, dtype=np.uint32).T
    got = capi.dbscan_edges(ei, ej, 13, 4, want_degree=True)
    want = dr.dbscan_from_edges(13, ei, ej, 4)
    dr.assert_same(got, want)
    assert (got["label"][a_ids] == 0).all() and (got["label"][b_ids] == 3).all()
    assert got["degree"][x] == 2 and got["label"][x] == 3        # neighbours 9 (cluster 0) and 3 (cluster 3): 3 < 9
    assert list(got["label"][[1, 2, 8, 12]]) == [dr.NOISE] * 4
    assert (got["n_clusters"], got["n_core"], got["n_border"], got["n_noise"], got["n_edges"]) == (2, 8, 1, 4, 28)
    # x one neighbour richer is core itself and fuses the two
    ei2, ej2 = np.append(ei, x).astype(np.uint32), np.append(ej, 4).astype(np.uint32)
    fused = capi.dbscan_edges(ei2, ej2, 13, 4)
    assert (fused["label"][a_ids + b_ids + [x]] == 0).all() and fused["n_clusters"] == 1 and fused["n_border"] == 0


def test_path_has_core_inside_and_border_ends():
    ids = [6, 2, 5, 1, 4]   # a - b - c - d - e
    ei, ej = np.array(ids[:-1], dtype=np.uint32), np.array(ids[1:], dtype=np.uint32)
    got = capi.dbscan_edges(ei, ej, 8, 3, want_degree=True)
    dr.assert_same(got, dr.dbscan_from_edges(8, ei, ej, 3))
    assert list(got["degree"]) == [0, 2, 2, 0, 1, 2, 1, 0]
    assert list(got["label"]) == [dr.NOISE, 1, 1, dr.NOISE, 1, 1, 1, dr.NOISE]
    assert (got["n_clusters"], got["n_core"], got["n_border"], got["n_noise"]) == (1, 3, 2, 3)
    tight = capi.dbscan_edges(ei, ej, 8, 4)   # nobody has three neighbours
    assert (tight["label"] == dr.NOISE).all() and tight["n_noise"] == 8


def test_errors_write_nothing():
    lib = capi.load()
    sentinel = 0xdeadbeef
    ei, ej = _graph(1, 50, 100)
    label, degree = np.full(50, sentinel, dtype=np.uint32), np.full(50, sentinel, dtype=np.uint32)
    c = capi._DbscanCounts(7, 7, 7, 7, 7)

    def call(pi, pj, m, n, min_pts, lab, deg, out=c):
        return lib.hs_dbscan_edges(pi, pj, m, n, min_pts, lab, deg, C.byref(out) if out is not None else None)

    bad = ei.copy()
    bad[99] = 50                                                          # the last pair names an id >= n
    for pi, pj in ((bad, ej), (ei, bad)):
        c.n_clusters = c.n_core = c.n_border = c.n_noise = c.n_edges = 7
        assert call(capi._vp(pi), capi._vp(pj), 100, 50, 2, capi._vp(label), capi._vp(degree)) == capi.HS_ERR_INVALID
        assert (label == sentinel).all() and (degree == sentinel).all()
        assert (c.n_clusters, c.n_core, c.n_border, c.n_noise, c.n_edges) == (0, 0, 0, 0, 0)
        with pytest.raises(capi.HsError) as e:
            capi.dbscan_edges(pi, pj, 50, 2)
        assert e.value.status == capi.HS_ERR_INVALID
    assert call(capi._vp(ei), capi._vp(ej), 100, 50, 0, capi._vp(label), capi._vp(degree)) == capi.HS_ERR_INVALID
    assert call(capi._vp(ei), capi._vp(ej), 100, 50, 2, None, capi._vp(degree)) == capi.HS_ERR_INVALID
    assert call(None, capi._vp(ej), 100, 50, 2, capi._vp(label), None) == capi.HS_ERR_INVALID
    assert call(capi._vp(ei), None, 100, 50, 2, capi._vp(label), None) == capi.HS_ERR_INVALID
    assert call(capi._vp(ei), capi._vp(ej), 100, 50, 2, capi._vp(label), None, out=None) == capi.HS_ERR_INVALID
    assert call(capi._vp(ei), capi._vp(ej), 100, 1 << 32, 2, capi._vp(label), None) == capi.HS_ERR_INVALID
    assert (label == sentinel).all() and (degree == sentinel).all()
    # nothing at all is fine: no vertices, no pairs, no arrays
    assert call(None, None, 0, 0, 1, None, None) == capi.HS_OK
    assert (c.n_clusters, c.n_core, c.n_border, c.n_noise, c.n_edges) == (0, 0, 0, 0, 0)
    assert call(capi._vp(ei), capi._vp(ej), 100, 50, 2, capi._vp(label), None) == capi.HS_OK   # and the degree optional
    assert (label != sentinel).all() and (degree == sentinel).all()
