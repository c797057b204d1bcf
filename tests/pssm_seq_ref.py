"""The contract of hs_pssm_seq_scan in numpy (include/hsearch.h), over the hits of tests/pssm_ref.py's scan: the
sequence of a hit by a search in id_start, one row per distinct (profile, sequence), the best hit by a lexsort on
(-score, id)."""
import numpy as np

FIELDS = ("m", "seq", "count", "best_score", "best_id", "lo", "hi")


def rows_from_hits(m, id, score, nm, id_start):
    """dict(m, seq, count, best_score, best_id, lo, hi, n_hits, cnt, seq_cnt) of DISTINCT hits (m, id, score)."""
    m = np.asarray(m, dtype=np.int64)
    id = np.asarray(id, dtype=np.int64)
    score = np.asarray(score, dtype=np.float64)
    id_start = np.asarray(id_start, dtype=np.uint64).astype(np.int64)
    n_seq = len(id_start) - 1
    # the LAST sequence that starts at or below the id owns it
    s = np.searchsorted(id_start, id, side="right") - 1
    off = id - id_start[s]
    key = m * (n_seq + 1) + s
    # (key, -score, id): the first element of every key's run is its best hit
    order = np.lexsort((id, -score, key))
    key_o = key[order]
    first = np.ones(len(order), dtype=bool)
    first[1:] = key_o[1:] != key_o[:-1]
    best = order[first]
    uniq, inv = np.unique(key, return_inverse=True)
    assert np.array_equal(uniq, key[best])
    count = np.bincount(inv, minlength=len(uniq))
    lo = np.full(len(uniq), np.iinfo(np.int64).max)
    hi = np.full(len(uniq), -1)
    np.minimum.at(lo, inv, off)
    np.maximum.at(hi, inv, off)
    rm = m[best]
    return dict(m=rm.astype(np.uint32), seq=s[best].astype(np.uint32), count=count.astype(np.uint32),
                best_score=score[best], best_id=id[best].astype(np.uint32), lo=lo.astype(np.uint32),
                hi=hi.astype(np.uint32), n_hits=len(m), cnt=np.bincount(m, minlength=nm).astype(np.uint64),
                seq_cnt=np.bincount(rm, minlength=nm).astype(np.uint64))


def rows(hits, nm, id_start):
    """The rows of a scan's result (pssm_ref.scan or Engine.pssm_scan)."""
    return rows_from_hits(hits["m"], hits["id"], hits["score"], nm, id_start)


def same_rows(got, want, what=""):
    for f in FIELDS:
        assert len(got[f]) == len(want[f]), (what, f, len(got[f]), len(want[f]))
        a, b = np.asarray(got[f]), np.asarray(want[f])
        if f == "best_score":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (what, f)
    for f in ("n_hits", "cnt", "seq_cnt"):
        if f in got and f in want:
            assert np.array_equal(got[f], want[f]), (what, f)
