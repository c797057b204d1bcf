"""The rule of hs_seq_match (include/hsearch.h) in plain numpy: a hit list reduced per (query group, database
sequence, diagonal).  Takes a hit list -- a dict with q, id, dist as the engine's query calls return it -- and the four
arrays q_group, n_groups, q_off, id_start; a (q, id) given several times counts once; -0.0 is read as +0.0."""
import numpy as np

FIELDS = ("group", "seq", "diag", "count", "best_dist", "best_q", "best_id", "lo", "hi")
_TYPES = dict(group=np.uint32, seq=np.uint32, diag=np.int32, count=np.uint32, best_dist=np.float64, best_q=np.uint32,
              best_id=np.uint32, lo=np.uint32, hi=np.uint32)


def empty():
    return {f: np.empty(0, dtype=_TYPES[f]) for f in FIELDS}


def seq_match(hits, id_start, q_group=None, q_off=None):
    q = np.asarray(hits["q"], dtype=np.int64)
    id = np.asarray(hits["id"], dtype=np.int64)
    dist = np.asarray(hits["dist"], dtype=np.float64) + 0.0
    id_start = np.asarray(id_start, dtype=np.int64)
    # one entry per (q, id)
    _, first = np.unique(q << 32 | id, return_index=True)
    q, id, dist = q[first], id[first], dist[first]
    if len(q) == 0:
        return empty()
    g = q if q_group is None else np.asarray(q_group, dtype=np.int64)[q]
    s = np.searchsorted(id_start, id, side="right") - 1  # the LAST sequence starting at or below id owns it
    off = id - id_start[s]
    diag = np.zeros(len(q), dtype=np.int64) if q_off is None else off - np.asarray(q_off, dtype=np.int64)[q]
    bits = dist.view(np.uint64)  # (distances are >= +0: the bits order like the doubles)
    order = np.lexsort((id, q, bits, diag, s, g))
    g, s, diag, q, id, dist, off = (x[order] for x in (g, s, diag, q, id, dist, off))
    head = np.ones(len(q), dtype=bool)
    head[1:] = (g[1:] != g[:-1]) | (s[1:] != s[:-1]) | (diag[1:] != diag[:-1])
    at = np.flatnonzero(head)
    return dict(group=g[at].astype(np.uint32), seq=s[at].astype(np.uint32), diag=diag[at].astype(np.int32),
                count=np.diff(np.append(at, len(q))).astype(np.uint32), best_dist=dist[at],
                best_q=q[at].astype(np.uint32), best_id=id[at].astype(np.uint32),
                lo=np.minimum.reduceat(off, at).astype(np.uint32), hi=np.maximum.reduceat(off, at).astype(np.uint32))


def assert_same(got, want, what=""):
    for f in FIELDS:
        assert got[f].dtype == _TYPES[f] and len(got[f]) == len(want[f]), (what, f, len(got[f]), len(want[f]))
    for f in FIELDS:
        a, b = got[f], want[f]
        if f == "best_dist":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, (what, f, int(bad[0]), {g: (got[g][bad[0]], want[g][bad[0]]) for g in FIELDS})


# ---- the proteins the GPU tests search: a database around k, queries assembled from its fragments -------------------
K_MER, LSH = 15, dict(K=8, L=4, W=120.0)
R = 12.0  # a k-mer itself (distance +0) and about a quarter of its single substitutions (3 .. 26 apart) are hits


def _cat(parts):
    lens = [len(p) for p in parts]
    res = np.concatenate(parts).astype(np.uint8) if sum(lens) else np.empty(0, dtype=np.uint8)
    return res, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def make_proteins(k=K_MER, seed=5):
    """dict(db, db_start, qry, qry_start): about 60 database proteins of 0 .. 300 residues (some shorter than k, some
    exactly k; about 4 000 windows) and 8 query proteins made of their fragments:
      0     an exact copy of k + 150 residues: one diagonal row of 151 hits at distance +0 (ties down to (q, id))
      1     the first 40 residues of a protein placed late (a negative diagonal, the first window), the last 40 of
            another placed early (a positive diagonal, the last window), a protein of exactly k residues whole
      2..6  each 25 fragments of exactly k residues (single seeds) and two fragments of 60 with substitutions
      7     shorter than k: a group without queries
    """
    rng = np.random.default_rng(seed)
    lens = [0, 3, k - 1, k, k, k + 1, 300, 280] + rng.integers(0, 160, 50).tolist() + [k - 2, 0]
    db = [rng.integers(0, 20, n).astype(np.uint8) for n in lens]
    rnd = lambda n: rng.integers(0, 20, n).astype(np.uint8)
    qry = [np.concatenate([rnd(20), db[6][100:100 + k + 150], rnd(10)]),
           np.concatenate([rnd(5), db[7][-40:], rnd(15), db[6][:40], rnd(7), db[3], rnd(4)])]
    donors = [s for s, n in enumerate(lens) if n >= k + 4]
    for _ in range(5):
        parts = []
        for _ in range(25):
            s = donors[rng.integers(len(donors))]
            at = rng.integers(0, lens[s] - k + 1)
            parts += [db[s][at:at + k], rnd(3)]
        for _ in range(2):
            s = donors[rng.integers(len(donors))]
            n = min(60, lens[s])
            at = rng.integers(0, lens[s] - n + 1)
            frag = db[s][at:at + n].copy()
            pos = np.arange(rng.integers(0, 12), n, 12)
            frag[pos] = (frag[pos] + rng.integers(1, 20, len(pos))) % 20  # (another residue, always)
            parts += [frag, rnd(6)]
        qry.append(np.concatenate(parts))
    qry.append(rnd(k - 1))
    d, ds = _cat(db)
    q, qs = _cat(qry)
    return dict(db=d, db_start=ds, qry=q, qry_start=qs)
