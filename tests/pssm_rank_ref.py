"""The contract of hs_pssm_rank in numpy (include/hsearch.h), from a score matrix of tests/pssm_ref.scores: the rank-th
largest score per profile with its two counts, the sample rule of hsearch_amd/csrc/hs_pssm_rank.h in Python integers,
the ladder's diagnostics (t_scan, rounds), and the refinement loop with the threshold rule."""
import math

import numpy as np

ALL = -1.7976931348623157e308    # -DBL_MAX: the last rung of the ladder, every k-mer


def ranks(rank, nm):
    return np.broadcast_to(np.asarray(rank, dtype=np.int64), (nm,))


def from_scores(sc, rank):
    """sc [nm][n], rank a scalar or [nm] -> dict(t, cnt_ge, cnt_gt)."""
    sc = np.asarray(sc, dtype=np.float64)
    nm, n = sc.shape
    r = ranks(rank, nm)
    assert np.all((r >= 1) & (r <= n))
    srt = -np.sort(-sc, axis=1)                      # descending; no NaN, no -0.0 among contract scores
    t = srt[np.arange(nm), r - 1].copy()
    return dict(t=t, cnt_ge=(sc >= t[:, None]).sum(axis=1).astype(np.uint64),
                cnt_gt=(sc > t[:, None]).sum(axis=1).astype(np.uint64))


def isqrt_up(q):
    s = math.isqrt(q)
    return s if s * s == q else s + 1


def plan(rank, n, n_s, rnd):
    """The sample rank r_s of round rnd; n_s + 1 for "beyond the sample"."""
    rank, n, n_s = int(rank), int(n), int(n_s)
    assert 1 <= rank <= n and 1 <= n_s <= n
    if n_s == n:
        return rank
    q = -(-rank * n_s // n)
    r = q + (4 * isqrt_up(q) + 8) * 4 ** rnd
    return r if r <= n_s else n_s + 1


def sample_ids(n, n_s):
    return (np.arange(n_s, dtype=np.uint64) * np.uint64(n) // np.uint64(n_s)).astype(np.int64)


def ladder(sc, rank, sample):
    """dict(t_scan [nm], rounds [nm], n_s, retries): the round that resolves each profile under the sample rule."""
    sc = np.asarray(sc, dtype=np.float64)
    nm, n = sc.shape
    r = ranks(rank, nm)
    n_s = min(n, int(sample))
    srt = -np.sort(-sc[:, sample_ids(n, n_s)], axis=1)
    t_scan, rounds = np.empty(nm), np.zeros(nm, dtype=np.uint32)
    for m in range(nm):
        j = 0
        while True:
            r_s = plan(r[m], n, n_s, j)
            t = ALL if r_s > n_s else srt[m, r_s - 1]
            if int((sc[m] >= t).sum()) >= r[m]:
                break
            j += 1
        t_scan[m], rounds[m] = t, j
    return dict(t_scan=t_scan, rounds=rounds, n_s=n_s, retries=int(rounds.sum()))


def same(got, want, what=""):
    for f in ("t", "cnt_ge", "cnt_gt"):
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        if f == "t":
            g, w = g.view(np.uint64), np.ascontiguousarray(w).view(np.uint64)
        assert np.array_equal(g, w), (what, f, np.flatnonzero(g != w)[:8])


def refine(codes, alphabet, S0, rank, n_iter, id_start=None, bg=None, pseudo=1.0):
    """hs_pssm_refine_rank's loop over the reference rules of tests/pssm_counts_ref.py: dict(S, t, counts, used, iters,
    converged, history) -- t: the threshold of the last scan; history: the counts of every scan."""
    import pssm_counts_ref
    import pssm_ref
    from hsearch_amd import capi
    S = np.array(S0, dtype=np.float64)
    bg = pssm_counts_ref.background(codes, alphabet) if bg is None else np.asarray(bg, dtype=np.float64)
    prev, history = None, []
    iters, converged = 0, False
    for i in range(n_iter):
        t = from_scores(pssm_ref.scores(S, codes), rank)["t"]
        got = pssm_counts_ref.hit_counts(codes, alphabet, S, t, id_start)
        history.append(got["counts"])
        iters += 1
        if i > 0 and np.array_equal(got["counts"], prev):
            converged = True
            break
        new = capi.pssm_log_odds_exact(got["counts"], bg, pseudo)
        keep = got["used"] == 0
        new[keep] = S[keep]
        S, prev = new, got["counts"]
    return dict(S=S, t=t, counts=got["counts"], used=got["used"], iters=iters, converged=converged, history=history)
