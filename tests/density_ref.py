"""The density-tree rule restated in plain Python / numpy (include/hsearch.h hs_core_distance / hs_density_tree /
hs_density_tree_edges / hs_density_tree_cut): core distances by sorting every vertex's neighbour distances, Kruskal
over the distinct unordered pairs in the order (w, lo, hi) with w = max(core[a], core[b], dist), and a plain cut.
Written from the definitions; the checker of the density tests, never the thing under test."""
import numpy as np

from tests.components_ref import _find, _labels

NOISE = 0xffffffff


def _distinct_pairs(ei, ej, dist):
    ei = np.asarray(ei, dtype=np.int64)
    ej = np.asarray(ej, dtype=np.int64)
    dist = np.asarray(dist, dtype=np.float64)
    keep = ei != ej
    lo, hi, d = np.minimum(ei, ej)[keep], np.maximum(ei, ej)[keep], dist[keep]
    order = np.lexsort((hi, lo))
    lo, hi, d = lo[order], hi[order], d[order]
    first = np.ones(len(lo), dtype=bool)
    first[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    assert np.array_equal(d.view(np.uint64)[~first], d.view(np.uint64)[np.flatnonzero(~first) - 1])
    return lo[first], hi[first], d[first]


def core_distances(n, lo, hi, d, min_pts):
    """float64 [n] from the DISTINCT unordered pairs: the (min_pts - 1)-th smallest neighbour distance with
    multiplicity, 0 for min_pts = 1, inf with fewer than min_pts - 1 neighbours."""
    assert min_pts >= 1
    if min_pts == 1:
        return np.zeros(n)
    nb = [[] for _ in range(n)]
    for x, y, w in zip(lo.tolist(), hi.tolist(), d.tolist()):
        nb[x].append(w)
        nb[y].append(w)
    return np.array([sorted(v)[min_pts - 2] if len(v) >= min_pts - 1 else np.inf for v in nb], dtype=np.float64)


def tree_from_edges(n, ei, ej, dist, min_pts):
    """Weighted pairs in any order, either or both directions, repeated, self pairs ignored -> dict(lo, hi uint32, w
    float64: the tree edges in ascending (w, lo, hi); core float64 [n]; label uint32 [n] (NOISE where core is inf);
    n_core, n_clusters, n_graph_edges = twice the distinct unordered pairs)."""
    lo, hi, d = _distinct_pairs(ei, ej, dist)
    core = core_distances(n, lo, hi, d, min_pts)
    w = np.maximum(d, np.maximum(core[lo], core[hi]))
    live = np.isfinite(w)
    n_graph = 2 * len(lo)
    lo, hi, w = lo[live], hi[live], w[live]
    order = np.lexsort((hi, lo, w))
    parent = list(range(n))
    t_lo, t_hi, t_w = [], [], []
    for x, y, v in zip(lo[order].tolist(), hi[order].tolist(), w[order].tolist()):
        rx, ry = _find(parent, x), _find(parent, y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
            t_lo.append(x)
            t_hi.append(y)
            t_w.append(v)
    label = _labels(parent)
    label[~np.isfinite(core)] = NOISE
    n_core = int(np.isfinite(core).sum())
    return dict(lo=np.array(t_lo, dtype=np.uint32), hi=np.array(t_hi, dtype=np.uint32),
                w=np.array(t_w, dtype=np.float64), core=core, label=label, n_core=n_core,
                n_clusters=n_core - len(t_lo), n_graph_edges=n_graph)


def cut(n, lo, hi, w, core, r):
    """uint32 [n]: NOISE where core > r or core is inf, else the smallest id per component of the tree edges with w <= r."""
    parent = list(range(n))
    for x, y, v in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist(), np.asarray(w).tolist()):
        if v <= r:
            rx, ry = _find(parent, x), _find(parent, y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    label = _labels(parent)
    core = np.asarray(core)
    label[~((core <= r) & np.isfinite(core))] = NOISE
    return label


def same_tree(got, want):
    """The three arrays bit-equal (weights compared as bits)."""
    return (got["lo"].dtype == np.uint32 and got["hi"].dtype == np.uint32 and got["w"].dtype == np.float64
            and np.array_equal(got["lo"], want["lo"]) and np.array_equal(got["hi"], want["hi"])
            and np.array_equal(got["w"].view(np.uint64), want["w"].view(np.uint64)))


def same_result(got, want):
    """Tree, core distances (as bits), labels and the counts the reference knows."""
    return (same_tree(got, want) and np.array_equal(got["core"].view(np.uint64), want["core"].view(np.uint64))
            and got["label"].dtype == np.uint32 and np.array_equal(got["label"], want["label"])
            and all(got[f] == want[f] for f in ("n_core", "n_clusters", "n_graph_edges"))
            and got["n_tree_edges"] == len(want["lo"]) == got["n_core"] - got["n_clusters"])
