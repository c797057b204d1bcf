"""The contract of hs_pssm_weighted_counts and hs_pssm_refine_weighted in numpy and Python integers (include/hsearch.h):
position-based sequence weights over the sites of tests/pssm_counts_ref.py, the weighted log-odds one entry at a time in
Python floats (IEEE doubles, every operation rounded on its own, math.log2 the C library's), and the loop over them:
nothing of the weighted rule is taken from the library, and the whole trajectory is comparable bit for bit."""
import math

import numpy as np

from hsearch_amd import capi

import pssm_counts_ref
import pssm_ref
import pssm_seq_ref

ONE = 1 << 56


def u(r, c):
    """floor(2^56 / (r c)) in Python integers; 0 where the residue does not occur"""
    return ONE // (int(r) * int(c)) if r and c else 0


def sites(hits, nm, id_start=None):
    """(m, id) of the DISTINCT sites of a hit list: every hit, or the best hit of every (profile, sequence) row"""
    m, i, sc = np.asarray(hits["m"]), np.asarray(hits["id"]), np.asarray(hits["score"])
    if id_start is None:
        key = np.unique((m.astype(np.int64) << 32) | i.astype(np.int64))
        return (key >> 32).astype(np.int64), (key & 0xffffffff).astype(np.int64)
    rows = pssm_seq_ref.rows_from_hits(m, i, sc, nm, id_start)
    return np.asarray(rows["m"], dtype=np.int64), np.asarray(rows["best_id"], dtype=np.int64)


def weigh(codes, alphabet, site_m, site_id, nm):
    """dict(counts, wcounts, wsum, distinct, used, weights) of the sites; weights: W(i) as Python integers, in the
    order of the sites"""
    codes = np.asarray(codes)
    k = codes.shape[1]
    counts, used = pssm_counts_ref.histogram(codes, alphabet, site_m, site_id, nm)
    table = [[[0] * alphabet for _ in range(k)] for _ in range(nm)]
    distinct = np.zeros(nm, dtype=np.uint32)
    for m in range(nm):
        for p in range(k):
            r = int((counts[m, p] > 0).sum())
            distinct[m] += r
            table[m][p] = [u(r, c) for c in counts[m, p].tolist()]
    wc = [[[0] * alphabet for _ in range(k)] for _ in range(nm)]
    wsum = [0] * nm
    weights = []
    for m, i in zip(np.asarray(site_m).tolist(), np.asarray(site_id).tolist()):
        row = codes[i].tolist()
        w = sum(table[m][p][row[p]] for p in range(k))
        for p in range(k):
            wc[m][p][row[p]] += w
        wsum[m] += w
        weights.append(w)
    assert all(s <= k * ONE for s in wsum)
    return dict(counts=counts, wcounts=np.array(wc, dtype=np.uint64).reshape(nm, k, alphabet),
                wsum=np.array(wsum, dtype=np.uint64).reshape(nm), distinct=distinct, used=used, weights=weights)


def from_hits(codes, alphabet, hits, nm, id_start=None):
    """dict(counts, wcounts, wsum, distinct, cnt, used, n_hits, weights) of a scan's hits"""
    sm, si = sites(hits, nm, id_start)
    res = weigh(codes, alphabet, sm, si, nm)
    raw = pssm_counts_ref.from_hits(codes, alphabet, hits, nm, id_start)
    assert np.array_equal(raw["counts"], res["counts"]) and np.array_equal(raw["used"], res["used"])
    res.update(cnt=raw["cnt"], n_hits=raw["n_hits"])
    return res


def weighted_counts(codes, alphabet, S, t, id_start=None):
    S = np.asarray(S, dtype=np.float64)
    return from_hits(codes, alphabet, pssm_ref.scan(S, t, codes), S.shape[0], id_start)


def log_odds_numpy(wcounts, wsum, n_eff, bg, pseudo):
    """the expression of hs_pssm_log_odds_weighted in numpy: every operation rounded to fp64 (log2 may differ by an ulp
    or two)"""
    wc = np.asarray(wcounts).astype(np.float64)
    ws = np.asarray(wsum).astype(np.float64)[:, None, None]
    ne = np.asarray(n_eff, dtype=np.float64)[:, None, None]
    bg = np.asarray(bg, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(ws > 0, wc / np.where(ws > 0, ws, 1.0), 0.0)
    return np.log2(((f * ne + pseudo * bg) / (ne + pseudo)) / bg)


def log_odds_exact(wcounts, wsum, n_eff, bg, pseudo):
    """hs_pssm_log_odds_weighted's expression, entry by entry in Python floats: bit for bit what the library must give"""
    wc = np.asarray(wcounts)
    nm, k, A = wc.shape
    S = np.empty((nm, k, A), dtype=np.float64)
    bg = [float(b) for b in np.asarray(bg, dtype=np.float64)]
    pseudo = float(pseudo)
    for m in range(nm):
        ws, ne = int(wsum[m]), float(n_eff[m])
        den = ne + pseudo
        for p in range(k):
            row = wc[m, p].tolist()
            for a in range(A):
                f = float(row[a]) / float(ws) if ws else 0.0
                x = f * ne
                b = pseudo * bg[a]
                num = x + b
                freq = num / den
                ratio = freq / bg[a]
                S[m, p, a] = math.log2(ratio)
    return S


def n_eff(got, k, neff):
    if neff == "sites":
        return got["used"].astype(np.float64)
    assert neff == "columns"
    return got["distinct"].astype(np.float64) / np.float64(k)


def refine(codes, alphabet, S0, n_iter, t=None, rank=None, id_start=None, bg=None, pseudo=1.0, neff="sites",
           weighted=True):
    """dict(S, t, counts, wcounts, wsum, distinct, used, iters, converged, history) -- history: the (counts, wcounts) of
    every scan.  weighted=False: the loop of hs_pssm_refine / hs_pssm_refine_rank, for comparison."""
    assert (t is None) != (rank is None)
    codes = np.asarray(codes)
    k = codes.shape[1]
    S = np.array(S0, dtype=np.float64)
    nm = S.shape[0]
    bg = pssm_counts_ref.background(codes, alphabet) if bg is None else np.asarray(bg, dtype=np.float64)
    prev, history = None, []
    iters, converged = 0, False
    ti = None if t is None else np.asarray(t, dtype=np.float64)
    for i in range(n_iter):
        if rank is not None:
            sc = pssm_ref.scores(S, codes)
            r = np.broadcast_to(np.asarray(rank, dtype=np.int64), (nm,))
            ti = np.array([np.sort(sc[m])[len(codes) - int(r[m])] for m in range(nm)])
        got = weighted_counts(codes, alphabet, S, ti, id_start)
        history.append((got["counts"], got["wcounts"]))
        iters += 1
        if i > 0 and np.array_equal(got["counts"], prev[0]) and (not weighted or np.array_equal(got["wcounts"], prev[1])):
            converged = True
            break
        if weighted:
            new = log_odds_exact(got["wcounts"], got["wsum"], n_eff(got, k, neff), bg, pseudo)
        else:
            new = capi.pssm_log_odds_exact(got["counts"], bg, pseudo)
        keep = got["used"] == 0
        new[keep] = S[keep]
        S, prev = new, (got["counts"], got["wcounts"])
    return dict(S=S, t=ti, counts=got["counts"], wcounts=got["wcounts"], wsum=got["wsum"], distinct=got["distinct"],
                used=got["used"], iters=iters, converged=converged, history=history)


def same_weights(got, want, what=""):
    pssm_counts_ref.same_counts(got, want, what)
    for f in ("wcounts", "wsum", "distinct"):
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, f)
    wc = np.asarray(got["wcounts"])
    k = wc.shape[1]
    cols = wc.sum(axis=2, dtype=np.uint64)
    assert np.array_equal(cols, np.broadcast_to(np.asarray(got["wsum"])[:, None], cols.shape)), what
    assert all(int(s) <= k * ONE for s in np.asarray(got["wsum"]).tolist()), what
