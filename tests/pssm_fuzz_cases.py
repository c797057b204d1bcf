"""Random worlds for the profile calls (not collected): world(seed) is a pure function of the seed and returns everything
one case of tests/test_pssm_fuzz_cpu.py and tests/test_gpu_pssm_fuzz.py needs -- the shape, the proteins with their
windows, the profiles and thresholds, the family layout, the chain's arguments, the arguments of the other calls, and
the reference scan's hits (tests/pssm_ref.py), which the thresholds and the bounds are taken from.  numpy only.

The protein style and the window count are dealt by the seed (every pair of them within 16 consecutive seeds); all else
is drawn.  Two bounds keep the Python references quick: at most MAX_HITS hits in a world and at most MAX_SEGMENT in one
(family, sequence) segment (the chain reference is quadratic in a segment); a world above either lowers the hit
fraction of its profile with the most hits by one step, until it fits."""
import numpy as np

from hsearch_amd import capi, synth

try:
    import pssm_ref
except ImportError:
    from tests import pssm_ref

KS = (1, 2, 3, 9, 15, 24, 25, 26, 40, 64, 75)
ALPHABETS = (2, 4, 16, 17, 20, 21, 32)
NMS = (1, 2, 5, 16, 17, 24, 33)
WINDOWS = (1, 70, 600, 2500)
STYLES = ("one", "short", "mix", "islands")
FRACTIONS = ("all", 0.30, 0.05, 0.01, "single", "none")  # in the order the bounds step through; "none" only by them
SHIFTS = (0, 1, 3, 40, 65535)
PENALTIES = ((0.0, 0.0), (4.0, 1.0), (0.5, 2.0 ** -20), (1.0, 0.25))
BINS = (64, 100, 4096)
ROUTES = ("windows", "codes", "append", "remove", "load")
MAX_HITS, MAX_SEGMENT = 20000, 2000
ALL_GROUPS = -1e300                                     # a group threshold every row passes
SPLIT_ABOVE = 4                                         # the hooks library's batch limit in the worlds that use it


def coords(A):
    """tests/test_gpu_pssm_topk.py's _coords: the coordinate table of an alphabet of A residues"""
    if A == 20:
        return None
    rng = np.random.default_rng(77)
    base = synth.coords()
    if A < 20:
        return np.ascontiguousarray(base[:A])
    return np.ascontiguousarray(np.concatenate([base, rng.normal(0, 3, size=(A - 20, 8))]))


def _lengths(r, style, k, target):
    """protein lengths whose windows number at least `target` (and not many more)"""
    lens, wins = [], 0
    if style == "one":
        return [k + target - 1]
    while wins < target:
        if style == "short":        # mostly one window or none
            l = int(r.choice([k, k, k, k + 1, k + 2, int(r.integers(0, k + 3)), int(r.integers(0, k))]))
        elif style == "mix":
            l = int(r.choice([k - 1, k, k + 1, k + 63, k + 64, k + 300]))
        else:                       # islands: a few long proteins between runs of empty ones
            lens += [0] * int(r.integers(1, 40))
            l = k - 1 + int(r.integers(1, max(2, target // 2 + 2)))
        l = min(l, k - 1 + max(1, target - wins + 3))
        lens.append(l)
        wins += max(0, l - k + 1)
    if style == "islands":
        lens += [0] * int(r.integers(1, 40))
    return lens


def windows(residues, seq_start, k):
    """codes [n][k] of the windows of the proteins, in index_build_windows' order"""
    starts = np.asarray(seq_start, dtype=np.int64)
    pos = np.concatenate([np.arange(s, max(s, e - k + 1)) for s, e in zip(starts[:-1], starts[1:])]
                         + [np.empty(0, dtype=np.int64)]).astype(np.int64)
    return np.ascontiguousarray(np.asarray(residues)[pos[:, None] + np.arange(k)[None, :]], dtype=np.uint8).reshape(-1, k)


def _threshold(row_desc, frac):
    """an ATTAINED score of the descending row: a tie at it is a hit"""
    n = len(row_desc)
    if frac == "all":
        return float(row_desc[-1])
    if frac == "single":
        return float(row_desc[0])
    if frac == "none":              # (where the best score is attained too often for the bounds)
        return float(np.nextafter(row_desc[0], np.inf))
    return float(row_desc[max(1, int(np.ceil(frac * n))) - 1])


def segment_sizes(hit, m_group, id_start):
    """[groups][n_seq]: the hits of every (family, sequence) segment, of hit [nm][n]"""
    nm, n = hit.shape
    ids = np.asarray(id_start, dtype=np.int64)
    n_seq = len(ids) - 1
    seq = np.searchsorted(ids, np.arange(n), side="right") - 1
    g = np.arange(nm) if m_group is None else np.asarray(m_group, dtype=np.int64)
    per = np.zeros((int(g.max()) + 1, n_seq), dtype=np.int64)
    m, i = np.nonzero(hit)
    np.add.at(per, (g[m], seq[i]), 1)
    return per


def world(seed):
    r = np.random.default_rng(77000 + seed)
    style, target = STYLES[seed % 4], WINDOWS[(seed // 4) % 4]
    # two worlds in seven are TIED: five profiles or more, none alone in its group, nearly constant matrices, offsets
    # 0 .. 2 and a shift allowed -- equal chain values under several profiles, so that the order of every choice shows
    tied = seed % 7 in (2, 5)
    long_one = style == "one" and target == WINDOWS[-1]      # the largest shift over the longest segments
    # thousands of one-window proteins get 16 profiles or more and, where the batches are not split, a family of 16
    crowd = style == "short" and target == WINDOWS[-1]
    k, A = int(r.choice(KS)), int(r.choice(ALPHABETS))
    nm = int(r.choice(NMS[3:] if crowd else NMS[2:] if tied else NMS))
    hooks = seed % 5 == 3                                # the library's test build, which splits batches above 4

    # ---- proteins ------------------------------------------------------------------------------------------------
    lens = _lengths(r, style, k, target)
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    if r.random() < 0.3:                                 # a skewed composition: equal windows are common
        residues = r.choice(A, size=int(seq_start[-1]), p=r.dirichlet(np.full(A, 0.3))).astype(np.uint8)
    else:
        residues = r.integers(0, A, size=int(seq_start[-1])).astype(np.uint8)
    codes = windows(residues, seq_start, k)
    id_start = capi.window_id_start(seq_start, k)
    n = len(codes)
    assert n == int(id_start[-1]) >= 1

    # ---- profiles ------------------------------------------------------------------------------------------------
    S = r.normal(0, 2, size=(nm, k, A))
    dyadic = r.random(nm) < float(r.choice([0.2, 0.5, 1.0]))
    S[dyadic] = r.integers(-16, 17, size=S[dyadic].shape) / 4.0          # equal scores are common
    if r.random() < 0.4:
        S[dyadic] = r.integers(-1, 2, size=S[dyadic].shape) / 2.0        # very coarse: ties everywhere
    if tied:
        S = np.where(r.random(S.shape) < 0.5 / k, 0.25, 0.5)              # about half of the windows score k / 2
    if r.random() < 0.5:
        S[int(r.integers(nm)), :, int(r.integers(A))] = -1e30              # one forbidden residue

    # ---- families ------------------------------------------------------------------------------------------------
    sizes = []
    kind = r.choice(["one", "random"] if tied else ["singletons", "one", "random", "random"])
    if crowd:
        kind, sizes = "random", [16]
    while sum(sizes) < nm:
        sizes.append({"singletons": 1, "one": nm}.get(kind)
                     or int(r.choice([3, 4, 5, 16] if tied else [1, 2, 3, 4, 5, 16])))
        if hooks:
            sizes[-1] = min(sizes[-1], SPLIT_ABOVE)
    numbers = np.arange(len(sizes))
    sparse = r.random() < 0.4
    if sparse:                                           # unused group numbers
        numbers = np.cumsum(r.integers(1, 4, size=len(sizes))) - 1
    m_group = np.repeat(numbers, sizes)[:nm].astype(np.uint32)
    n_groups = int(m_group.max()) + 1 + (int(r.integers(0, 3)) if sparse else 0)
    m_off = r.integers(0, 3 if tied or r.random() < 0.3 else 2 * k, size=nm).astype(np.uint32)  # (0 .. 2: equal ones)
    if r.random() < 0.2:
        m_off[int(r.integers(nm))] = 10 ** 6             # larger than every protein: all its diagonals are negative
    chain_off = m_off[np.lexsort((m_off, m_group))].copy()               # sorted inside groups, for the chain
    dup = scaled = None
    if nm >= 2 and r.random() < 0.5:                     # one profile twice, side by side in one group at one offset
        dup = int(r.integers(nm - 1))
        S[dup + 1] = S[dup]
        m_group[dup + 1] = m_group[dup]
        m_off[dup + 1], chain_off[dup + 1] = m_off[dup], chain_off[dup]
    elif nm >= 3 and r.random() < 0.6:                   # three profiles of one group at 2^40, 1 and 2^-12
        scaled = int(r.integers(nm - 2))
        S[scaled:scaled + 3] = r.normal(0, 1, size=(3, k, A)) * np.array([2.0 ** 40, 1.0, 2.0 ** -12])[:, None, None]
        m_group[scaled + 1:scaled + 3] = m_group[scaled]
        m_off[scaled + 1:scaled + 3], chain_off[scaled + 1:scaled + 3] = m_off[scaled], chain_off[scaled]
    if hooks:                                            # (the two edits above can lengthen a group)
        while np.bincount(m_group).max() > SPLIT_ABOVE:
            g = int(np.bincount(m_group).argmax())
            m_group[np.flatnonzero(m_group == g)[SPLIT_ABOVE:]] = g + 1
            m_group[1:] = np.maximum.accumulate(m_group)[1:]
        n_groups = max(n_groups, int(m_group.max()) + 1)
        chain_off = chain_off[np.lexsort((chain_off, m_group))]

    # ---- thresholds: attained scores at the hit fractions, stepped down to the bounds ------------------------------
    sc = pssm_ref.scores(S, codes)
    desc = -np.sort(-sc, axis=1)
    main = int(r.integers(2 if tied else 5))
    step = np.where(r.random(nm) < 0.7, main, r.integers(0, 5, size=nm))
    dead = int(r.integers(nm)) if r.random() < 0.5 else None
    if seed % 16 == 6:
        dead = "all"                                     # a world without a hit

    def thresholds():
        t = np.array([_threshold(desc[m], FRACTIONS[step[m]]) for m in range(nm)])
        if dup is not None:
            t[dup + 1] = t[dup]
        if dead == "all":
            t = np.nextafter(desc[:, 0], np.inf)
        elif dead is not None:
            t[dead] = np.nextafter(desc[dead, 0], np.inf)                # the next double above the best score
        return t

    while True:
        t = thresholds()
        hit = sc >= t[:, None]
        per_m = hit.sum(axis=1)
        if per_m.sum() <= MAX_HITS and segment_sizes(hit, m_group, id_start).max() <= MAX_SEGMENT:
            break
        worst = int(np.argmax(np.where(step < len(FRACTIONS) - 1, per_m, -1)))
        assert step[worst] < len(FRACTIONS) - 1
        step[worst] += 1
        if dup is not None and worst in (dup, dup + 1):
            step[dup] = step[dup + 1] = step[worst]
    hits = pssm_ref.scan(S, t, codes)

    # ---- the family's filters, the chain, the other calls ---------------------------------------------------------
    median = float(np.sort(hits["score"])[len(hits["score"]) // 2]) if len(hits["score"]) else 0.0
    t_kind = r.choice(["none", "median", "mixed"])
    t_group = None
    if t_kind != "none":
        t_group = np.full(n_groups, median)
        if t_kind == "mixed":
            t_group[r.random(n_groups) < 0.5] = ALL_GROUPS
    gap_open, gap_ext = PENALTIES[int(r.integers(len(PENALTIES)))]
    topk = min(int(r.choice([1, 7, n, n + 5])), capi.TOPK_MAX)
    rank = r.integers(1, n + 1, size=nm).astype(np.uint64)
    rank[int(r.integers(nm))] = int(r.choice([1, n]))
    bg = r.dirichlet(np.full(A, 2.0)) * (1.0 - 2.0 ** -30)              # (a total mass below 1, as the null tests take it)
    top = float(np.max(S.max(axis=2).sum(axis=1)))
    h = max(1, nm // 2)
    d0 = (S[:, None, :, :] * S[None, :, :, :]).sum(axis=(2, 3))          # about the d = 0 similarities
    return dict(
        seed=seed, style=style, tied=tied, k=k, A=A, nm=nm, n=n, coords=coords(A), hooks=hooks,
        residues=residues, seq_start=seq_start, codes=codes, id_start=id_start, n_seq=len(id_start) - 1,
        S=S, t=t, sc=sc, hits=hits, dup=dup, scaled=scaled, dead=dead,
        m_group=m_group, n_groups=n_groups, m_off=m_off, chain_off=chain_off,
        min_count=int(r.choice([1, 2, 3])), t_group=t_group,
        max_shift=SHIFTS[-1] if long_one else int(r.choice(SHIFTS[1:] if tied else SHIFTS)),
        gap_open=gap_open, gap_ext=gap_ext,
        topk=topk, rank=rank, bg=bg, bins=int(r.choice(BINS)),
        t_lo=None if r.random() < 0.5 else float(top - r.choice([3.0, 20.0, 200.0])),
        p=float(r.choice([1.0, 0.5, 1e-2, 1e-5])),
        min_overlap=int(r.choice([1, k // 2 + 1, k])), cmp_t=float(np.quantile(d0, 0.6)), cmp_split=h,
        # how the GPU test runs the world: by the seed's residues, so that a failure's name reproduces it
        # (seed 27: query_batch = 1 with pssm_filter = 0 on an appended index)
        pssm_filter=0 if seed % 4 == 3 else 1, query_batch=(1, 3, 16)[seed % 3],
        route=ROUTES[seed % 5] if n >= 2 else ROUTES[seed % 2], dev=seed % 4 == 2)


def references(w):
    """What every call must return for the world w, from the reference rules of tests/*_ref.py alone: dict(seq, fam,
    fam_plain, chain, topk, topk_hits, rank, counts, counts_seq, weights, weights_seq, cmp_self, cmp_xy, pv_m,
    pv_score, p_hi, p_lo, thr, reached, seconds -- the references' CPU time)."""
    import time
    try:
        import pssm_chain_ref, pssm_compare_ref, pssm_counts_ref, pssm_family_ref, pssm_null_ref, pssm_rank_ref
        import pssm_seq_ref, pssm_topk_ref, pssm_weights_ref
    except ImportError:
        from tests import (pssm_chain_ref, pssm_compare_ref, pssm_counts_ref, pssm_family_ref, pssm_null_ref,
                           pssm_rank_ref, pssm_seq_ref, pssm_topk_ref, pssm_weights_ref)
    t0 = time.process_time()
    h, nm, ids, k, A = w["hits"], w["nm"], w["id_start"], w["k"], w["A"]
    out = dict(seq=pssm_seq_ref.rows(h, nm, ids), fam_plain=pssm_family_ref.rows(h, nm, ids))
    out["fam"] = pssm_family_ref.rows(h, nm, ids, **family_args(w))
    out["chain"] = pssm_chain_ref.chains(h, nm, ids, *chain_args(w)[0], **chain_args(w)[1])
    out["topk"] = pssm_topk_ref.rows_from_scores(w["sc"], w["topk"])
    out["topk_hits"] = pssm_topk_ref.rows_from_scores(w["sc"], w["topk"], t_floor=w["t"])
    out["rank"] = pssm_rank_ref.from_scores(w["sc"], w["rank"])
    out["counts"] = pssm_counts_ref.from_hits(w["codes"], A, h, nm)
    out["counts_seq"] = pssm_counts_ref.from_hits(w["codes"], A, h, nm, ids)
    out["weights"] = pssm_weights_ref.from_hits(w["codes"], A, h, nm)
    out["weights_seq"] = pssm_weights_ref.from_hits(w["codes"], A, h, nm, ids)
    X, Y = compare_args(w)
    out["cmp_self"] = pssm_compare_ref.compare(w["S"], w["cmp_t"], None, w["min_overlap"])
    out["cmp_xy"] = pssm_compare_ref.compare(X, w["cmp_t"], Y, w["min_overlap"])
    # p-values: of the world's hits and, per profile, of a score above the grid and one below it
    prs = pssm_null_ref.tables(w["S"], w["bg"], w["t_lo"], w["bins"])
    top = w["S"].max(axis=2).sum(axis=1)
    out["pv_m"] = np.concatenate([h["m"], np.arange(nm), np.arange(nm)]).astype(np.uint32)
    out["pv_score"] = np.concatenate([h["score"], top + np.abs(top) + 1.0, np.full(nm, -1e300)])
    out["p_hi"], out["p_lo"] = pssm_null_ref.pvalues(prs, k, A, w["bins"], out["pv_m"], out["pv_score"])
    out["thr"] = pssm_null_ref.thresholds(prs, k, A, w["bins"], w["t_lo"], w["p"])
    out["seconds"] = time.process_time() - t0
    out["reached"] = reached(w, out)
    return out


def family_args(w):
    return dict(m_group=w["m_group"], n_groups=w["n_groups"], m_off=w["m_off"], min_count=w["min_count"],
                t_group=w["t_group"])


def chain_args(w):
    return ((w["m_group"], w["chain_off"], w["max_shift"]),
            dict(gap_open=w["gap_open"], gap_ext=w["gap_ext"], min_count=w["min_count"], t_group=w["t_group"],
                 n_groups=w["n_groups"]))


def compare_args(w):
    """X and Y of the X-against-Y comparison: the two halves of the profiles (one profile: against itself)"""
    h = w["cmp_split"]
    return w["S"][:h], (w["S"][h:] if w["nm"] > 1 else w["S"])


def reached(w, want):
    """The edges the world reaches, on the reference alone: name -> bool"""
    h, ids = w["hits"], w["id_start"].astype(np.int64)
    m, i = h["m"].astype(np.int64), h["id"].astype(np.int64)
    seq = np.searchsorted(ids, i, side="right") - 1
    g = w["m_group"].astype(np.int64)[m]
    segs = np.unique(g * (len(ids) + 1) + seq, return_counts=True)[1]
    # a reported family row whose best score two different profiles attain
    fam, tie = want["fam"], False
    if len(fam["group"]) and len(m):
        diag = (i - ids[seq]) - w["m_off"].astype(np.int64)[m]
        best = {(int(a), int(b), int(c)): (float(s), int(bm)) for a, b, c, s, bm in
                zip(fam["group"], fam["seq"], fam["diag"], fam["best_score"], fam["best_m"])}
        for a, b, c, s, mm in zip(g.tolist(), seq.tolist(), diag.tolist(), h["score"].tolist(), m.tolist()):
            row = best.get((a, b, c))
            if row is not None and row[0] == s and row[1] != mm:
                tie = True
                break
    stride = (w["A"] + 15) // 16 * 16
    return dict(segment_over_256=bool(len(segs) and segs.max() > 256),
                run_over_64=bool(len(want["seq"]["count"]) and want["seq"]["count"].max() > 64),
                sequences_over_256=w["n_seq"] > 256, one_sequence=w["n_seq"] == 1,
                empty_sequences=bool((np.diff(w["seq_start"].astype(np.int64)) == 0).any()),
                chain_of_4=bool(len(want["chain"]["count"]) and want["chain"]["count"].max() >= 4),
                chain_with_gap=bool(len(want["chain"]["gaps"]) and want["chain"]["gaps"].max() > 0),
                row_of_2=bool(len(fam["count"]) and fam["count"].max() >= 2), best_tie=tie,
                compare_unfiltered=w["k"] * stride > 1024, n_is_1=w["n"] == 1, no_hit=len(m) == 0)


# the floors tests/test_pssm_fuzz_cpu.py holds the default case set to: worlds that must reach each edge
FLOORS = dict(segment_over_256=4, run_over_64=4, sequences_over_256=4, one_sequence=4, empty_sequences=4, chain_of_4=4,
              chain_with_gap=4, row_of_2=4, best_tie=4, compare_unfiltered=4, n_is_1=1, no_hit=1)
DEFAULT_CASES = 32
