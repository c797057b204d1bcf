"""Per-query radii restated from scalar searches (include/hsearch.h hs_query_radii): the result of a radii call is
the concatenation over the queries of the scalar call's result at each query's own radius.  A helper module for the
radii tests (not collected)."""
import numpy as np

# radius sets that straddle the regimes of a k-mer length: tight, the usual radius (twice: the common class), one
# on the 8-column side of the row choice for k = 25, and 0 (only identical k-mers)
RADIUS_SETS = {15: (12.0, 30.0, 30.0, 42.0, 0.0), 25: (20.0, 40.0, 40.0, 55.0, 0.0), 39: (30.0, 50.0, 50.0, 70.0, 0.0)}


def draw_radii(k, nq, seed=None):
    s = np.array(RADIUS_SETS[k])
    return s[np.random.default_rng(100 + k if seed is None else seed).integers(0, len(s), nq)]


def stitch(scalar_query, queries, radii, fields=("q", "id", "table", "dist", "cand")):
    """scalar_query(queries_subset, R) -> dict, run once per distinct radius over the queries that carry it, put
    back in query order.  Returns (result dict, {radius: number of hits})."""
    radii = np.asarray(radii, dtype=np.float64)
    nq = len(radii)
    per_q = [None] * nq
    cand = None
    hits_of = {}
    for r in sorted(set(radii.tolist())):
        sel = np.nonzero(radii == r)[0]
        res = scalar_query(queries[sel], float(r))
        hits_of[r] = len(res["q"])
        if "cand" in fields:
            if cand is None:
                cand = np.zeros((nq, res["cand"].shape[1]), dtype=np.uint64)
            cand[sel] = res["cand"]
        bounds = np.searchsorted(res["q"], np.arange(len(sel) + 1))
        for j, q in enumerate(sel):
            per_q[q] = {f: res[f][bounds[j]:bounds[j + 1]] for f in fields if f not in ("q", "cand")}
    out = {"q": np.concatenate([np.full(len(per_q[q]["id"]), q, dtype=np.uint32) for q in range(nq)])
           if nq else np.empty(0, dtype=np.uint32)}
    for f in fields:
        if f not in ("q", "cand"):
            out[f] = np.concatenate([per_q[q][f] for q in range(nq)]) if nq else np.empty(0)
    if "cand" in fields:
        out["cand"] = cand
    return out, hits_of
