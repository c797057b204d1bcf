"""The annotation rule restated in numpy (include/hsearch.h hs_annotate / hs_merge_best): of a list of hits
(q, id, table, dist), per distinct id the hit that is smallest under (dist, table, q), rows in ascending id.  The
checker of the annotate tests, never the thing under test (a helper module, not collected)."""
import numpy as np

FIELDS = ("id", "q", "table", "dist")


def annotate(hits):
    """hits: dict with q, id, table, dist (any order).  Returns the dict of the kept rows."""
    hid = np.asarray(hits["id"], dtype=np.uint32)
    hq = np.asarray(hits["q"], dtype=np.uint32)
    ht = np.asarray(hits["table"], dtype=np.uint32)
    hd = np.asarray(hits["dist"], dtype=np.float64)
    order = np.lexsort((hq, ht, hd, hid))  # last key first: id, then dist, then table, then q
    first = np.ones(len(order), dtype=bool)
    first[1:] = hid[order][1:] != hid[order][:-1]
    keep = order[first]
    return dict(id=hid[keep], q=hq[keep], table=ht[keep], dist=hd[keep])


def concat(parts):
    return {f: np.concatenate([np.asarray(p[f]) for p in parts]) for f in FIELDS}


def assert_same(got, want, what=""):
    for f in FIELDS:
        assert np.array_equal(np.asarray(got[f]), np.asarray(want[f])), (what, f)
    # bitwise distances
    assert np.array_equal(np.asarray(got["dist"], dtype=np.float64).view(np.uint64),
                          np.asarray(want["dist"], dtype=np.float64).view(np.uint64)), (what, "dist bits")


def tie_levels(hits):
    """How often each level of the rule decides among the hits of one id: (ids decided by table at equal smallest
    distance, ids decided by q at equal smallest distance and table)."""
    hid, hq, ht, hd = (np.asarray(hits[f]) for f in ("id", "q", "table", "dist"))
    order = np.lexsort((hq, ht, hd, hid))
    i, q, t, d = hid[order], hq[order], ht[order], hd[order]
    same = (i[1:] == i[:-1]) & (d[1:] == d[:-1])
    first = np.ones(len(order), dtype=bool)
    first[1:] = i[1:] != i[:-1]
    second = np.zeros(len(order), dtype=bool)  # the runner-up of an id, right behind its winner
    second[1:] = first[:-1] & ~first[1:]
    by_table = int((second[1:] & same & (t[1:] != t[:-1])).sum())
    by_q = int((second[1:] & same & (t[1:] == t[:-1]) & (q[1:] != q[:-1])).sum())
    return by_table, by_q
