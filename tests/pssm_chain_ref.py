"""The contract of hs_pssm_family_chain (include/hsearch.h) in fp64 over the hits of tests/pssm_ref.py's scan, written
independently of hsearch_amd/csrc/hs_pssm_chain.h: EVERY predecessor of every hit is listed (quadratic in a segment's
hits; numpy's element-wise fp64 operations, each rounded once), the list is sorted under the contract's order and its
head is taken when it is above +0.0.  Also the gapped planted construction of the end-to-end tests."""
import numpy as np

import pssm_family_ref as fam

FIELDS = ("group", "seq", "count", "gaps", "score", "first_m", "first_id", "last_m", "last_id", "shift")
TYPES = (np.uint32, np.uint32, np.uint32, np.uint32, np.float64, np.uint32, np.uint32, np.uint32, np.uint32, np.int32)
BITS = ("score",)


def chains_from_hits(m, id, score, nm, id_start, m_group, m_off, max_shift, gap_open=0.0, gap_ext=0.0, min_count=1,
                     t_group=None, n_groups=None, pred_m_ascending=False):
    """dict(FIELDS..., path [list of [(m, id), ...]], n_hits, cnt, grp_rows, all_segs) of DISTINCT hits (m, id, score).
    pred_m_ascending: ties between predecessors broken towards the SMALLER m -- NOT the contract; the tests use it to
    show that the tie order matters."""
    m = [int(x) for x in np.asarray(m).ravel()]
    id = [int(x) for x in np.asarray(id).ravel()]
    score = [float(x) + 0.0 for x in np.asarray(score, dtype=np.float64).ravel()]      # (-0.0 + 0.0 is +0.0)
    starts = [int(x) for x in np.asarray(id_start, dtype=np.uint64)]
    m_off = [int(x) for x in m_off]
    g_of = list(range(nm)) if m_group is None else [int(x) for x in m_group]
    if n_groups is None:
        n_groups = nm if m_group is None else (max(g_of) + 1 if nm else 0)
    gap_open, gap_ext = float(gap_open) + 0.0, float(gap_ext) + 0.0
    starts_a = np.asarray(starts, dtype=np.int64)
    segs = {}
    for i in sorted(range(len(m)), key=lambda i: (m[i], id[i])):                       # ascending (m, id)
        s = int(np.searchsorted(starts_a, id[i], side="right")) - 1                      # the LAST sequence at or below
        off = id[i] - starts[s]
        segs.setdefault((g_of[m[i]], s), []).append(dict(m=m[i], id=id[i], off=off, diag=off - m_off[m[i]],
                                                         score=score[i]))
    out = {f: [] for f in FIELDS}
    paths = []
    sign = 1 if pred_m_ascending else -1
    for key in sorted(segs):
        hits = segs[key]
        H = len(hits)
        M = np.array([h["m"] for h in hits], dtype=np.int64)
        ID = np.array([h["id"] for h in hits], dtype=np.int64)
        OFF = np.array([h["off"] for h in hits], dtype=np.int64)
        DIAG = np.array([h["diag"] for h in hits], dtype=np.int64)
        Cs, N = np.zeros(H, dtype=np.float64), np.zeros(H, dtype=np.int64)
        for i, h in enumerate(hits):
            d = np.abs(DIAG[i] - DIAG[:i])
            ok = np.nonzero((M[:i] < M[i]) & (OFF[:i] < OFF[i]) & (d <= max_shift))[0]       # EVERY predecessor
            best = None
            if len(ok):
                dj = d[ok]
                step = np.float64(gap_ext) * dj.astype(np.float64)       # one rounded product ...
                pen = np.float64(gap_open) + step                        # ... one rounded sum ...
                v = np.where(dj == 0, Cs[ok], Cs[ok] - pen)              # ... one rounded difference; C itself at d = 0
                j = np.lexsort((ID[ok], sign * M[ok], -N[ok], -v))[0]    # v, n descending; m descending; id ascending
                if v[j] > 0.0:
                    best = (float(v[j]), int(ok[j]), int(dj[j]))
            if best:
                v, j, dd = best
                h.update(C=v + h["score"], n=hits[j]["n"] + 1, first=hits[j]["first"], gaps=hits[j]["gaps"] + (dd != 0),
                         pred=j)
            else:
                h.update(C=0.0 + h["score"], n=1, first=i, gaps=0, pred=None)
            Cs[i], N[i] = h["C"], h["n"]
        ends = [i for i, h in enumerate(hits)
                if h["n"] >= min_count and (t_group is None or h["C"] >= float(t_group[key[0]]))]
        if not ends:
            continue
        e = min(ends, key=lambda i: (-hits[i]["C"], -hits[i]["n"], hits[i]["m"], hits[i]["id"]))
        h, f = hits[e], hits[hits[e]["first"]]
        vals = (key[0], key[1], h["n"], h["gaps"], h["C"], f["m"], f["id"], h["m"], h["id"], h["diag"] - f["diag"])
        for name, v in zip(FIELDS, vals):
            out[name].append(v)
        path, j = [], e
        while j is not None:
            path.append((hits[j]["m"], hits[j]["id"]))
            j = hits[j]["pred"]
        paths.append(path[::-1])
    res = {f: np.array(out[f], dtype=t) for f, t in zip(FIELDS, TYPES)}
    res.update(path=paths, n_hits=len(m), cnt=np.bincount(np.asarray(m, dtype=np.int64), minlength=nm).astype(np.uint64),
               grp_rows=np.bincount(res["group"], minlength=n_groups).astype(np.uint64), all_segs=len(segs))
    return res


def chains(hits, nm, id_start, m_group, m_off, max_shift, **kw):
    """The chains of a scan's result (pssm_ref.scan or Engine.pssm_scan)."""
    return chains_from_hits(hits["m"], hits["id"], hits["score"], nm, id_start, m_group, m_off, max_shift, **kw)


def same_chains(got, want, what=""):
    for f in FIELDS:
        assert len(got[f]) == len(want[f]), (what, f, len(got[f]), len(want[f]))
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.dtype == b.dtype, (what, f, a.dtype, b.dtype)
        if f in BITS:
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (what, f, a[:8], b[:8])
    for f in ("n_hits", "cnt", "grp_rows"):
        if f in got and f in want:
            assert np.array_equal(got[f], want[f]), (what, f)
    if "path_start" in got and "path" in want:
        assert got["path_start"].tolist() == np.concatenate([[0], np.cumsum([len(p) for p in want["path"]])]).tolist()
        flat = [x for p in want["path"] for x in p]
        assert list(zip(got["path_m"].tolist(), got["path_id"].tolist())) == flat, what


def sorted_offsets(m_group, nm, k, seed=5):
    """pssm_family_ref.offsets_in_groups with the offsets sorted inside every group (the chain's order rule)"""
    off = fam.offsets_in_groups(m_group, nm, k, seed).astype(np.int64)
    g = np.arange(nm) if m_group is None else np.asarray(m_group, dtype=np.int64)
    order = np.lexsort((off, g))
    return off[order].astype(np.uint32)


def rescore(path, score_of, m_off, id_start, gap_open, gap_ext):
    """the value of a chain's path [(m, id), ...] under the rule, from its hits' scores"""
    starts = np.asarray(id_start, dtype=np.uint64).astype(np.int64)
    total, prev = None, None
    for m, i in path:
        s = int(np.searchsorted(starts, i, side="right")) - 1
        diag = i - int(starts[s]) - int(m_off[m])
        if total is None:
            total = 0.0 + score_of[(m, i)]
        else:
            d = abs(diag - prev)
            v = total if d == 0 else total - (float(gap_open) + float(gap_ext) * float(d))
            total = v + score_of[(m, i)]
        prev = diag
    return total


PLANTED_GAPPED = (1, 6, 8, 9)            # the four lowest-numbered planted proteins of seed 20261
PLANTED_UNGAPPED = (19, 25, 31, 32, 33)


def planted_gapped(seed=20261, n_gap=4, ins=1):
    """pssm_family_ref.planted_motif with `ins` random residues inserted behind motif column 10 in the n_gap
    lowest-numbered planted proteins, as planted_case lays it out: dict(residues, seq_start, planted {protein: position},
    gapped (the proteins with the insertion), S, t, codes, id_start, k, A, shifts)."""
    from hsearch_amd import capi
    c = fam.planted_motif(seed=seed)
    k, A = c["k"], c["A"]
    rng = np.random.default_rng(seed + 1000 * ins)
    starts = c["seq_start"].astype(np.int64)
    prots = [c["residues"][a:b] for a, b in zip(starts[:-1], starts[1:])]
    gapped = sorted(c["planted"])[:n_gap]
    for p in gapped:
        at = c["planted"][p] + 11
        prots[p] = np.concatenate([prots[p][:at], rng.integers(0, A, size=ins).astype(np.uint8), prots[p][at:]])
    c["gapped"] = tuple(gapped)
    c["residues"] = np.concatenate(prots)
    c["seq_start"] = np.concatenate([[0], np.cumsum([len(p) for p in prots])]).astype(np.uint64)
    starts = c["seq_start"].astype(np.int64)
    pos = np.concatenate([np.arange(s, e - k + 1) for s, e in zip(starts[:-1], starts[1:])])
    c["codes"] = np.ascontiguousarray(c["residues"][pos[:, None] + np.arange(k)], dtype=np.uint8)
    c["id_start"] = capi.window_id_start(c["seq_start"], k)
    c["t"] = np.full(len(c["S"]), fam.PLANTED_T)
    c["ins"] = ins
    return c
