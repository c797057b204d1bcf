"""The top-k rule of include/hsearch.h (hs_query_topk, hs_self_knn, hs_topk_merge) in plain numpy: of a list of tuples
(q, id, table, dist) with each (q, id) once, per q the first topk under (dist bits, id).  Distances are >= +0 and no
NaN, so their bit patterns order like the doubles."""
import numpy as np

NO_ID = 0xffffffff


def topk_rows(q, id, table, dist, nq, topk):
    """dict(id, table, dist [nq][topk], count [nq]); unused entries NO_ID, NO_ID, +inf."""
    q = np.asarray(q, dtype=np.int64)
    id = np.asarray(id, dtype=np.uint32)
    table = np.asarray(table, dtype=np.uint32)
    bits = np.ascontiguousarray(dist, dtype=np.float64).view(np.uint64)
    order = np.lexsort((id, bits, q))
    qs = q[order]
    count = np.bincount(q, minlength=nq).astype(np.uint32)
    start = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64) if nq else np.zeros(0, dtype=np.int64)
    rank = np.arange(len(qs), dtype=np.int64) - start[qs]
    keep = rank < topk
    out_id = np.full((nq, topk), NO_ID, dtype=np.uint32)
    out_t = np.full((nq, topk), NO_ID, dtype=np.uint32)
    out_d = np.full((nq, topk), np.inf, dtype=np.float64)
    rows, cols, src = qs[keep], rank[keep], order[keep]
    out_id[rows, cols] = id[src]
    out_t[rows, cols] = table[src]
    out_d.view(np.uint64)[rows, cols] = bits[src]
    return dict(id=out_id, table=out_t, dist=out_d, count=count)


def same_rows(got, want, tables=True):
    """bit for bit: ids, tables, distance bits and counts"""
    return (got["id"].dtype == np.uint32 and got["dist"].dtype == np.float64 and got["count"].dtype == np.uint32
            and got["id"].shape == want["id"].shape and np.array_equal(got["id"], want["id"])
            and (not tables or np.array_equal(got["table"], want["table"]))
            and np.array_equal(got["dist"].view(np.uint64), want["dist"].view(np.uint64))
            and np.array_equal(got["count"], want["count"]))


def flatten(rows):
    """the rows of a result as tuples (q, id, table, dist), padding included: what topk_merge takes back"""
    nq, topk = rows["id"].shape
    q = np.repeat(np.arange(nq, dtype=np.uint32), topk)
    return q, rows["id"].ravel(), rows["table"].ravel(), rows["dist"].ravel()
