"""The contracts of hs_pssm_family_scan and hs_pssm_family_layout (include/hsearch.h) in numpy and Python floats, over
the hits of tests/pssm_ref.py's scan.  The row sum is an explicit loop over the row's hits in (m, id) order; the layout
is a dictionary-based union-find with positions, written independently of hsearch_amd/csrc/hs_pssm_family.h."""
import numpy as np

FIELDS = ("group", "seq", "diag", "count", "sum", "best_score", "best_m", "best_id", "lo", "hi")
BITS = ("sum", "best_score")


def rows_from_hits(m, id, score, nm, id_start, m_group=None, n_groups=None, m_off=None, min_count=1, t_group=None,
                   reverse_sum=False):
    """dict(FIELDS..., n_hits, cnt, grp_rows, all_rows) of DISTINCT hits (m, id, score).  reverse_sum: the sum taken
    in descending (m, id) order -- NOT the contract; the tests use it to show that the order matters."""
    m = np.asarray(m, dtype=np.int64)
    id = np.asarray(id, dtype=np.int64)
    score = np.asarray(score, dtype=np.float64)
    id_start = np.asarray(id_start, dtype=np.uint64).astype(np.int64)
    if n_groups is None:
        n_groups = nm if m_group is None else (int(np.max(m_group)) + 1 if nm else 0)
    g_of = np.arange(nm, dtype=np.int64) if m_group is None else np.asarray(m_group, dtype=np.int64)
    order = np.lexsort((id, m))
    m, id, score = m[order], id[order], score[order]
    s = np.searchsorted(id_start, id, side="right") - 1       # the LAST sequence that starts at or below the id
    off = id - id_start[s]
    diag = off - np.asarray(m_off, dtype=np.int64)[m] if m_off is not None else np.zeros(len(m), dtype=np.int64)
    g = g_of[m]
    rows = {}
    for i in range(len(m)):                                   # in ascending (m, id)
        rows.setdefault((int(g[i]), int(s[i]), int(diag[i])), []).append(i)
    out = {f: [] for f in FIELDS}
    all_rows = 0
    for key in sorted(rows):
        members = rows[key]
        all_rows += 1
        total = 0.0
        for i in (reversed(members) if reverse_sum else members):
            total = total + float(score[i])
        best = min(members, key=lambda i: (-score[i], m[i], id[i]))
        if len(members) < min_count or (t_group is not None and not total >= float(t_group[key[0]])):
            continue
        vals = (key[0], key[1], key[2] & 0xffffffff, len(members), total, score[best], m[best], id[best],
                min(off[i] for i in members), max(off[i] for i in members))
        for f, v in zip(FIELDS, vals):
            out[f].append(v)
    res = dict(group=np.array(out["group"], dtype=np.uint32), seq=np.array(out["seq"], dtype=np.uint32),
               diag=np.array(out["diag"], dtype=np.uint32).view(np.int32), count=np.array(out["count"], dtype=np.uint32),
               sum=np.array(out["sum"], dtype=np.float64), best_score=np.array(out["best_score"], dtype=np.float64),
               best_m=np.array(out["best_m"], dtype=np.uint32), best_id=np.array(out["best_id"], dtype=np.uint32),
               lo=np.array(out["lo"], dtype=np.uint32), hi=np.array(out["hi"], dtype=np.uint32))
    res.update(n_hits=len(m), cnt=np.bincount(m, minlength=nm).astype(np.uint64), all_rows=all_rows,
               grp_rows=np.bincount(res["group"], minlength=n_groups).astype(np.uint64))
    return res


def rows(hits, nm, id_start, **kw):
    """The rows of a scan's result (pssm_ref.scan or Engine.pssm_scan)."""
    return rows_from_hits(hits["m"], hits["id"], hits["score"], nm, id_start, **kw)


def same_rows(got, want, what=""):
    for f in FIELDS:
        assert len(got[f]) == len(want[f]), (what, f, len(got[f]), len(want[f]))
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.dtype == b.dtype, (what, f, a.dtype, b.dtype)
        if f in BITS:
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (what, f)
    for f in ("n_hits", "cnt", "grp_rows"):
        if f in got and f in want:
            assert np.array_equal(got[f], want[f]), (what, f)


def layout(hit_x, hit_y, hit_d, nm):
    """dict(group, off, order, n_groups, n_conflicts): the hits taken in order; pos[y] - pos[x] = d."""
    comp = {v: {v: 0} for v in range(nm)}        # the component of every profile: member -> position, shared
    conflicts = 0
    for x, y, d in zip(map(int, hit_x), map(int, hit_y), map(int, hit_d)):
        cx, cy = comp[x], comp[y]
        if cx is cy:
            conflicts += int(cy[y] - cx[x] != d)
            continue
        shift = cx[x] + d - cy[y]                # what brings y's component into x's frame
        for v, p in cy.items():
            cx[v] = p + shift
            comp[v] = cx
    group = np.zeros(nm, dtype=np.uint32)
    off = np.zeros(nm, dtype=np.uint32)
    seen = {}
    for v in range(nm):                          # numbered by the smallest member
        c = comp[v]
        if id(c) not in seen:
            seen[id(c)] = len(seen)
        group[v] = seen[id(c)]
        off[v] = c[v] - min(c.values())
    order = np.array(sorted(range(nm), key=lambda v: (group[v], off[v], v)), dtype=np.uint32)
    return dict(group=group, off=off, order=order, n_groups=len(seen), n_conflicts=conflicts)


def group_layouts(nm):
    """name -> m_group [nm] (None: singleton groups) for the layouts the tests run: singletons, one group of all,
    mixed sizes 1, 2, 3, 5 repeating"""
    mixed = np.repeat(np.arange(nm), np.resize([1, 2, 3, 5], nm))[:nm]
    return {"singletons": None, "one": np.zeros(nm, dtype=np.uint32), "mixed": mixed.astype(np.uint32)}


def offsets_in_groups(m_group, nm, k, seed=5):
    """m_off [nm]: offsets from 0 up to k + 6 (so that diagonals go negative), the first profile of every group at 0"""
    rng = np.random.default_rng(seed + nm)
    off = rng.integers(0, k + 7, size=nm).astype(np.uint32)
    g = np.arange(nm) if m_group is None else np.asarray(m_group)
    first = np.ones(nm, dtype=bool)
    first[1:] = g[1:] != g[:-1]
    off[first] = 0
    if nm > 1:
        off[-1] = k + 6
    return off


def order_sensitive_profiles(k, A, seed=41):
    """Three profiles for ONE group whose scores are of the order 2^40, 1 and 2^-12 with full mantissas: the sum of a
    row in another order rounds differently."""
    rng = np.random.default_rng(seed)
    base = rng.normal(0, 1, size=(3, k, A))
    return base * np.array([2.0 ** 40, 1.0, 2.0 ** -12])[:, None, None]


def planted_motif(seed=20261, k=25, A=20, n_prot=40, n_planted=9, motif_len=31, shifts=(0, 3, 6)):
    """Synthetic proteins, a motif of motif_len residues planted in a minority of them, and the profiles of its windows
    at `shifts`.  dict(residues, seq_start, planted {protein: position}, S [len(shifts)][k][A], t, shifts).  The
    profiles score +2 for the motif's residue and -1 otherwise, times 4 in the columns over the profile's own third of
    the motif and times 1/4 elsewhere: every profile listens to another part of the motif (what ordered blocks do), so a
    chance match of one says little about the others.  Column-wise Pearson correlation does not see the weights."""
    rng = np.random.default_rng(seed)
    motif = rng.integers(0, A, size=motif_len).astype(np.uint8)
    lens = rng.integers(60, 140, size=n_prot)
    prots = [rng.integers(0, A, size=int(l)).astype(np.uint8) for l in lens]
    planted = {}
    for p in rng.choice(n_prot, size=n_planted, replace=False):
        pos = int(rng.integers(0, lens[p] - motif_len + 1))
        copy = motif.copy()
        copy[rng.choice(motif_len, size=3, replace=False)] = rng.integers(0, A, size=3)   # a few substitutions
        prots[p][pos:pos + motif_len] = copy
        planted[int(p)] = pos
    S = np.full((len(shifts), k, A), -1.0)
    third = -(-motif_len // len(shifts))
    for i, sh in enumerate(shifts):
        S[i, np.arange(k), motif[sh:sh + k]] = 2.0
        own = (np.arange(k) + sh) // third == i           # the columns over the profile's own third of the motif
        S[i] *= np.where(own, 4.0, 0.25)[:, None]
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return dict(residues=np.concatenate(prots), seq_start=seq_start, planted=planted, S=S, motif=motif,
                shifts=np.array(shifts), k=k, A=A)


# the planted motif of the end-to-end tests: seed 20261, every profile at a threshold of -10
PLANTED_SEED, PLANTED_T = 20261, -10.0


def planted_case():
    """planted_motif at PLANTED_SEED with its windows index (codes, id_start) and thresholds t"""
    from hsearch_amd import capi
    c = planted_motif(seed=PLANTED_SEED)
    k = c["k"]
    starts = c["seq_start"].astype(np.int64)
    pos = np.concatenate([np.arange(s, e - k + 1) for s, e in zip(starts[:-1], starts[1:])])
    c["codes"] = np.ascontiguousarray(c["residues"][pos[:, None] + np.arange(k)], dtype=np.uint8)
    c["id_start"] = capi.window_id_start(c["seq_start"], k)
    c["t"] = np.full(len(c["S"]), PLANTED_T)
    return c
