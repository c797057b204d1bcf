"""The DBSCAN rule restated in plain Python (include/hsearch.h hs_dbscan / hs_dbscan_edges): sets of neighbours, the
union-find of tests/components_ref.py over the core vertices, the smallest core neighbour for a border vertex.  The
checker of the dbscan tests, never the thing under test."""
import numpy as np

from tests import components_ref as cr

NOISE = 0xffffffff


def neighbours(n, ei, ej):
    """Edges (ei[t], ej[t]) in any order, either or both directions, repeated, self pairs ignored -> the list of the
    n sets of neighbours: the graph, to be clustered at several min_pts."""
    nbr = [set() for _ in range(n)]
    for x, y in zip(np.asarray(ei).tolist(), np.asarray(ej).tolist()):
        if x != y:
            nbr[x].add(y)
            nbr[y].add(x)
    return nbr


def dbscan_from_neighbours(nbr, min_pts):
    """dict(label uint32 [n], degree uint32 [n], n_clusters, n_core, n_border, n_noise, n_edges)."""
    assert min_pts >= 1
    n = len(nbr)
    degree = np.array([len(s) for s in nbr], dtype=np.uint32).reshape(n)
    core = [len(s) + 1 >= min_pts for s in nbr]
    cx, cy = [], []
    for x in range(n):
        if core[x]:
            for y in nbr[x]:
                if x < y and core[y]:
                    cx.append(x)
                    cy.append(y)
    comp = cr.labels_from_edges(n, cx, cy)   # a non-core vertex stays alone in it and is not looked at
    label = np.full(n, NOISE, dtype=np.uint32)
    n_border = 0
    for x in range(n):
        if core[x]:
            label[x] = comp[x]
        else:
            near = [y for y in nbr[x] if core[y]]
            if near:
                label[x] = comp[min(near)]
                n_border += 1
    n_core = int(sum(core))
    return dict(label=label, degree=degree, n_clusters=int(sum(1 for x in range(n) if core[x] and comp[x] == x)),
                n_core=n_core, n_border=n_border, n_noise=n - n_core - n_border, n_edges=int(degree.sum()))


def dbscan_from_edges(n, ei, ej, min_pts):
    return dbscan_from_neighbours(neighbours(n, ei, ej), min_pts)


def assert_same(got, want, what=None, degree=True):
    """Exact equality of a dbscan result (Engine.dbscan / capi.dbscan_edges) with the reference's."""
    assert got["label"].dtype == np.uint32 and got["label"].shape == want["label"].shape, what
    assert np.array_equal(got["label"], want["label"]), what
    if degree:
        assert got["degree"].dtype == np.uint32 and np.array_equal(got["degree"], want["degree"]), what
    for f in ("n_clusters", "n_core", "n_border", "n_noise", "n_edges"):
        assert got[f] == want[f], (what, f, got[f], want[f])


def check_invariants(res, n, min_pts):
    label, degree = res["label"], res["degree"]
    assert res["n_core"] + res["n_border"] + res["n_noise"] == n
    assert int(degree.sum()) == res["n_edges"]
    core = degree.astype(np.int64) + 1 >= min_pts
    live = label != NOISE
    assert res["n_core"] == int(core.sum()) and res["n_noise"] == int((~live).sum())
    assert not core[~live].any()                              # a core vertex is never noise
    assert (label[live] < n).all()
    assert core[label[live]].all()                            # every label is a core vertex ...
    assert np.array_equal(label[label[live]], label[live])    # ... that labels itself
    assert (label[core] <= np.nonzero(core)[0]).all()
    assert res["n_clusters"] == int((label[core] == np.nonzero(core)[0]).sum())
