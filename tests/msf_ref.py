"""The spanning-forest rule restated in plain Python / numpy (include/hsearch.h hs_msf / hs_msf_edges / hs_msf_cut):
Kruskal over the distinct unordered pairs in the order (dist, lo, hi) with a list-based union-find, and a plain cut.
The checker of the msf tests, never the thing under test."""
import numpy as np

from tests.components_ref import _find, _labels


def msf_from_edges(n, ei, ej, dist):
    """Weighted pairs in any order, either or both directions, repeated, self pairs ignored ->
    dict(lo uint32, hi uint32, dist float64: the tree edges in ascending (dist, lo, hi); label uint32 [n];
    n_graph_edges = twice the distinct unordered pairs)."""
    ei = np.asarray(ei, dtype=np.int64)
    ej = np.asarray(ej, dtype=np.int64)
    dist = np.asarray(dist, dtype=np.float64)
    keep = ei != ej
    lo, hi, d = np.minimum(ei, ej)[keep], np.maximum(ei, ej)[keep], dist[keep]
    # one occurrence per unordered pair (its occurrences carry the same bits: checked)
    order = np.lexsort((hi, lo))
    lo, hi, d = lo[order], hi[order], d[order]
    first = np.ones(len(lo), dtype=bool)
    first[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    assert np.array_equal(d.view(np.uint64)[~first], d.view(np.uint64)[np.flatnonzero(~first) - 1])
    lo, hi, d = lo[first], hi[first], d[first]
    order = np.lexsort((hi, lo, d))                      # (dist, lo, hi)
    parent = list(range(n))
    t_lo, t_hi, t_d = [], [], []
    for x, y, w in zip(lo[order].tolist(), hi[order].tolist(), d[order].tolist()):
        rx, ry = _find(parent, x), _find(parent, y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
            t_lo.append(x)
            t_hi.append(y)
            t_d.append(w)
    return dict(lo=np.array(t_lo, dtype=np.uint32), hi=np.array(t_hi, dtype=np.uint32),
                dist=np.array(t_d, dtype=np.float64), label=_labels(parent), n_graph_edges=2 * len(lo))


def cut(n, lo, hi, dist, r):
    """uint32 [n] labels (smallest id per component) of the forest of the tree edges with dist <= r."""
    parent = list(range(n))
    for x, y, w in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist(), np.asarray(dist).tolist()):
        if w <= r:
            rx, ry = _find(parent, x), _find(parent, y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    return _labels(parent)


def same_tree(got, want):
    """The three arrays bit-equal (distances compared as bits)."""
    return (got["lo"].dtype == np.uint32 and got["hi"].dtype == np.uint32 and got["dist"].dtype == np.float64
            and np.array_equal(got["lo"], want["lo"]) and np.array_equal(got["hi"], want["hi"])
            and np.array_equal(got["dist"].view(np.uint64), want["dist"].view(np.uint64)))
