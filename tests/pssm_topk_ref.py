"""The contract of hs_pssm_topk in numpy (include/hsearch.h) on top of pssm_ref.scores: the rows, the counts, and
t_used for a given sample size through the s_j = floor(j * n / n_s) rule."""
import numpy as np

NO_ID = 0xffffffff
NO_FLOOR = -np.finfo(np.float64).max


def rows_from_scores(sc, topk, t_floor=None):
    """sc [nm][n] -> dict(id uint32 [nm][topk], score [nm][topk], count uint32 [nm]): per profile, of the k-mers with
    score >= floor, the best under (score descending, id ascending); padded with NO_ID / -inf."""
    sc = np.asarray(sc, dtype=np.float64)
    nm, n = sc.shape
    floor = np.full(nm, NO_FLOOR) if t_floor is None else np.asarray(t_floor, dtype=np.float64)
    tid = np.full((nm, topk), NO_ID, dtype=np.uint32)
    ts = np.full((nm, topk), -np.inf)
    tc = np.zeros(nm, dtype=np.uint32)
    ids = np.arange(n)
    for m in range(nm):
        keep = ids[sc[m] >= floor[m]]
        order = keep[np.lexsort((keep, -sc[m, keep]))][:topk]   # stable on (-score, id)
        tid[m, :len(order)] = order
        ts[m, :len(order)] = sc[m, order]
        tc[m] = len(order)
    return dict(id=tid, score=ts, count=tc)


def sample_ids(n, sample):
    n_s = min(n, sample)
    return np.array([j * n // n_s for j in range(n_s)], dtype=np.int64)   # python ints: exact


def t_used_from_scores(sc, topk, sample, t_floor=None):
    """[nm]: max(floor, the topk-th largest score over the sample), or the floor where the sample holds fewer than
    topk scores."""
    sc = np.asarray(sc, dtype=np.float64)
    nm, n = sc.shape
    floor = np.full(nm, NO_FLOOR) if t_floor is None else np.asarray(t_floor, dtype=np.float64).copy()
    if n == 0:
        return floor
    s = sample_ids(n, sample)
    if len(s) < topk:
        return floor
    tp = -np.sort(-sc[:, s], axis=1)[:, topk - 1]
    return np.maximum(floor, tp)


def rows(S, codes, topk, t_floor=None):
    try:
        import pssm_ref
    except ImportError:
        from tests import pssm_ref
    return rows_from_scores(pssm_ref.scores(S, codes), topk, t_floor)


def same_rows(got, want, what=""):
    assert np.array_equal(got["id"], want["id"]), what
    assert np.array_equal(got["score"].view(np.uint64), want["score"].view(np.uint64)), what
    assert np.array_equal(got["count"], want["count"]), what
