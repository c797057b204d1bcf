"""The rules of hs_cluster_weighted_profile and hs_cluster_pssm_cover (include/hsearch.h) in Python integers and numpy:
the rows of tests/summary_ref.py, the weights of tests/pssm_weights_ref.py with the members of a row as its sites, and
the left-to-right fp64 score of tests/pssm_ref.py.  Nothing of either rule is taken from the library."""
import numpy as np

import pssm_ref
import pssm_weights_ref
import summary_ref

NOISE = summary_ref.NOISE


def members(label, min_size):
    """(row labels, sizes, site_m, site_id): the (row, member) tuples in ascending (row, id)"""
    label = np.asarray(label, dtype=np.uint32)
    rl, rs = summary_ref.rows_of(label, min_size)
    sm, si = [], []
    for r, v in enumerate(rl.tolist()):
        ids = np.nonzero(label == v)[0]
        sm.append(np.full(len(ids), r, dtype=np.int64))
        si.append(ids.astype(np.int64))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int64)
    return rl, rs, cat(sm), cat(si)


def weighted_profile(codes, alphabet, label, min_size):
    """dict(label, size, counts, wcounts, wsum, distinct, weights)"""
    codes = np.asarray(codes, dtype=np.uint8)
    rl, rs, sm, si = members(label, min_size)
    res = pssm_weights_ref.weigh(codes, alphabet, sm, si, len(rl))
    assert np.array_equal(res["used"], rs.astype(np.uint64))
    k = codes.shape[1]
    return dict(label=rl, size=rs, counts=res["counts"].reshape(len(rl), k, alphabet),
                wcounts=res["wcounts"], wsum=res["wsum"], distinct=res["distinct"], weights=res["weights"])


def cover(codes, label, min_size, S):
    """dict(min_score, argmin): per row the smallest left-to-right score of its members and the smallest id attaining
    it (the ids of a row ascend: the first at the minimum)"""
    codes = np.asarray(codes, dtype=np.uint8)
    label = np.asarray(label, dtype=np.uint32)
    S = np.asarray(S, dtype=np.float64)
    rl, _ = summary_ref.rows_of(label, min_size)
    assert S.shape[0] == len(rl)
    ms = np.zeros(len(rl), dtype=np.float64)
    am = np.zeros(len(rl), dtype=np.uint32)
    for r, v in enumerate(rl.tolist()):
        ids = np.nonzero(label == v)[0]
        sc = pssm_ref.scores(S[r:r + 1], codes[ids])[0]
        ms[r] = sc.min()
        am[r] = ids[np.nonzero(sc == sc.min())[0][0]]
    return dict(min_score=ms, argmin=am)


def assert_same(got, want, what=""):
    for f in ("label", "size", "counts", "wcounts", "wsum", "distinct", "min_score", "argmin"):
        if f not in want or f not in got:
            continue
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, f, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, f)
        else:
            assert np.array_equal(g, w), (what, f)
    if "wcounts" in got and "wsum" in got and len(got["wsum"]):
        cols = np.asarray(got["wcounts"]).sum(axis=2, dtype=np.uint64)
        assert np.array_equal(cols, np.broadcast_to(np.asarray(got["wsum"])[:, None], cols.shape)), what
