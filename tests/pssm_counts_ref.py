"""The contract of hs_pssm_hit_counts and hs_pssm_refine in numpy (include/hsearch.h): a histogram over the hits of
tests/pssm_ref.py's scan, or over the best hits of tests/pssm_seq_ref.py's rows in the one-site-per-protein mode, and
the loop over them.  The loop takes its log-odds from capi.pssm_log_odds_exact (the host function the library applies),
so the whole trajectory is comparable bit for bit."""
import numpy as np

from hsearch_amd import capi

import pssm_ref
import pssm_seq_ref


def histogram(codes, alphabet, m, id, nm):
    """counts uint32 [nm][k][alphabet] and used uint64 [nm] of the DISTINCT sites (m, id)"""
    codes = np.asarray(codes)
    k = codes.shape[1]
    m = np.asarray(m, dtype=np.int64)
    id = np.asarray(id, dtype=np.int64)
    counts = np.zeros((nm, k, alphabet), dtype=np.int64)
    for p in range(k):
        np.add.at(counts, (m, p, codes[id, p].astype(np.int64)), 1)
    return counts.astype(np.uint32), np.bincount(m, minlength=nm).astype(np.uint64)


def from_hits(codes, alphabet, hits, nm, id_start=None):
    """dict(counts, cnt, used, n_hits) of a scan's hits (pssm_ref.scan or Engine.pssm_scan restricted to m < nm)"""
    m, i, sc = np.asarray(hits["m"]), np.asarray(hits["id"]), np.asarray(hits["score"])
    cnt = np.bincount(m.astype(np.int64), minlength=nm).astype(np.uint64)
    if id_start is None:
        counts, used = histogram(codes, alphabet, m, i, nm)
    else:
        rows = pssm_seq_ref.rows_from_hits(m, i, sc, nm, id_start)
        counts, used = histogram(codes, alphabet, rows["m"], rows["best_id"], nm)
        assert np.array_equal(used, rows["seq_cnt"])
    return dict(counts=counts, cnt=cnt, used=used, n_hits=len(m))


def hit_counts(codes, alphabet, S, t, id_start=None):
    S = np.asarray(S, dtype=np.float64)
    return from_hits(codes, alphabet, pssm_ref.scan(S, t, codes), S.shape[0], id_start)


def log_odds_numpy(counts, bg, pseudo):
    """the expression of hs_pssm_log_odds in numpy: every operation rounded to fp64 (log2 may differ by an ulp or two)"""
    c = np.asarray(counts).astype(np.float64)
    size = np.asarray(counts).astype(np.uint64).sum(axis=-1, keepdims=True).astype(np.float64)
    bg = np.asarray(bg, dtype=np.float64)
    return np.log2(((c + pseudo * bg) / (size + pseudo)) / bg)


def background(codes, alphabet):
    """the residue composition of the index: the counts of one profile that hits everything"""
    codes = np.asarray(codes)
    counts, _ = histogram(codes, alphabet, np.zeros(len(codes), np.int64), np.arange(len(codes)), 1)
    return capi.pssm_background(counts[0])


def refine(codes, alphabet, S0, t, n_iter, id_start=None, bg=None, pseudo=1.0):
    """dict(S, counts, used, iters, converged, history) -- history: the counts of every scan"""
    S = np.array(S0, dtype=np.float64)
    bg = background(codes, alphabet) if bg is None else np.asarray(bg, dtype=np.float64)
    prev, history = None, []
    iters, converged = 0, False
    for i in range(n_iter):
        got = hit_counts(codes, alphabet, S, t, id_start)
        history.append(got["counts"])
        iters += 1
        if i > 0 and np.array_equal(got["counts"], prev):
            converged = True
            break
        new = capi.pssm_log_odds_exact(got["counts"], bg, pseudo)
        keep = got["used"] == 0
        new[keep] = S[keep]
        S, prev = new, got["counts"]
    return dict(S=S, counts=got["counts"], used=got["used"], iters=iters, converged=converged, history=history)


def same_counts(got, want, what=""):
    for f in ("counts", "cnt", "used"):
        if f in got and f in want:
            a, b = np.asarray(got[f]), np.asarray(want[f])
            assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
            assert np.array_equal(a, b), (what, f)
    if "n_hits" in got and "n_hits" in want:
        assert got["n_hits"] == want["n_hits"], what
    assert np.array_equal(np.asarray(got["counts"]).sum(axis=2, dtype=np.uint64),
                          np.broadcast_to(np.asarray(got["used"])[:, None], np.asarray(got["counts"]).shape[:2])), what
