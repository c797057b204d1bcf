"""The components rule restated in plain Python / numpy (include/hsearch.h hs_components / hs_components_merge):
a union-find over n vertices; label[i] = the smallest id of i's connected component.  The checker of the
components tests, never the thing under test."""
import numpy as np


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def _labels(parent):
    n = len(parent)
    label = np.empty(n, dtype=np.uint32)
    for i in range(n):          # the smaller root always stays: a root is its tree's smallest id
        label[i] = _find(parent, i)
    return label


def labels_from_edges(n, ei, ej):
    """Edges (ei[t], ej[t]) in any order, either or both directions -> uint32 [n] labels."""
    parent = list(range(n))
    for x, y in zip(np.asarray(ei).tolist(), np.asarray(ej).tolist()):
        rx, ry = _find(parent, x), _find(parent, y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return _labels(parent)


def merge_labels(stack):
    """[m][n] label arrays -> the labels of the union of the m forests (edges i -- stack[r][i])."""
    stack = np.asarray(stack)
    m, n = stack.shape
    ids = np.tile(np.arange(n), m)
    return labels_from_edges(n, ids, stack.reshape(-1))


def n_components(label):
    return int((np.asarray(label) == np.arange(len(label))).sum())


def random_forest(rng, n, p_edge=0.5):
    """Labels of a random sparse graph on n vertices (about p_edge * n edges): a valid hs_components output."""
    m = int(p_edge * n)
    return labels_from_edges(n, rng.integers(0, max(n, 1), m), rng.integers(0, max(n, 1), m))
