"""Multi-probe LSH restated in numpy (include/hsearch.h hs_set_multiprobe, rules 1-5): the probe sequence of a
point in a table, and a CPU multi-probe search.  A helper module for the multi-probe tests (not collected)."""
import heapq

import numpy as np


def fractions(oracle, a, b, W, pts):
    """Rule 1 for every table: (h[n][L][K] int64, x[n][L][K] fp64), elementwise fp64 from the oracle's dots."""
    hs, xs = [], []
    for l in range(a.shape[0]):
        _, dots = oracle.hash_table(a[l], b[l], W, pts, want_dots=True)
        v = (dots + b[l][None, :]) / W
        h = np.floor(v)
        hs.append(h.astype(np.int64))
        xs.append(v - h)
    return np.stack(hs, axis=1), np.stack(xs, axis=1)


def sorted_distances(x):
    """Rule 2: the 2K boundary distances of one (point, table) ascending by (z, j, delta): [(z, j, delta)]."""
    z = []
    for j, xj in enumerate(x):
        z.append((float(xj), j, -1))
        z.append((float(1.0 - xj), j, +1))
    z.sort()
    return z


def score(z, mask):
    """Rule 3: sum of z_i * z_i over the set in ascending i, each product and sum rounded (fp64)."""
    s = 0.0
    i = 0
    while mask >> i:
        if (mask >> i) & 1:
            s = s + z[i][0] * z[i][0]
        i += 1
    return s


def is_valid(z, mask):
    seen = set()
    for i in range(len(z)):
        if (mask >> i) & 1:
            if z[i][1] in seen:
                return False
            seen.add(z[i][1])
    return True


def perturbation_sets(z, T):
    """Rule 4: the emitted masks (at most T) of the (score, mask) min-heap."""
    M = len(z)
    heap = [(score(z, 1), 1)]
    out, pops = [], 0
    while len(out) < T and pops < 4 * (T + 1) and heap:
        _, m = heapq.heappop(heap)
        pops += 1
        top = m.bit_length() - 1
        if top + 1 < M:
            shifted = (m & ~(1 << top)) | (1 << (top + 1))
            expanded = m | (1 << (top + 1))
            heapq.heappush(heap, (score(z, shifted), shifted))
            heapq.heappush(heap, (score(z, expanded), expanded))
        if is_valid(z, m):
            out.append(m)
    return out


def all_valid_sets(z):
    """Every valid non-empty set, by (score, mask): what the heap must emit in order (given enough pops)."""
    M = len(z)
    sets = [(score(z, m), m) for m in range(1, 1 << M) if is_valid(z, m)]
    sets.sort()
    return [m for _, m in sets]


def probe_buckets(oracle, a, b, W, pts, T):
    """Rule 5: (buckets[n][L][1+T][K] int32, valid[n][L][1+T] uint8); empty slots repeat the home bucket."""
    h, x = fractions(oracle, a, b, W, pts)
    n, L, K = h.shape
    P = T + 1
    buckets = np.repeat(h[:, :, None, :], P, axis=2)
    valid = np.zeros((n, L, P), dtype=np.uint8)
    valid[:, :, 0] = 1
    for q in range(n):
        for l in range(L):
            z = sorted_distances(x[q, l])
            for t, m in enumerate(perturbation_sets(z, T), start=1):
                for i, (_, j, delta) in enumerate(z):
                    if (m >> i) & 1:
                        buckets[q, l, t, j] += delta
                valid[q, l, t] = 1
    return buckets.astype(np.int32), valid


def search(oracle, a, b, W, db_pts, centers, R, T):
    """A CPU multi-probe search: dict(q, id, table, dist, cand) in the order (query, table, id)."""
    db_ints = oracle.hash_all(a, b, W, db_pts)  # [n][L][K]
    L = a.shape[0]
    tables = []
    for l in range(L):
        d = {}
        for i, key in enumerate(map(tuple, db_ints[:, l, :])):
            d.setdefault(key, []).append(i)
        tables.append(d)
    buckets, valid = probe_buckets(oracle, a, b, W, centers, T)
    d2 = oracle.pairwise_square(db_pts, centers)  # [nq][n]
    r2 = R * R
    nq = centers.shape[0]
    cand = np.zeros((nq, L), dtype=np.uint64)
    hq, hid, ht, hd = [], [], [], []
    for q in range(nq):
        first = {}
        for l in range(L):
            for t in range(T + 1):
                if not valid[q, l, t]:
                    continue
                members = tables[l].get(tuple(int(v) for v in buckets[q, l, t]), [])
                cand[q, l] += len(members)
                for i in members:
                    if i not in first:
                        first[i] = l
        rows = sorted((l, i) for i, l in first.items() if d2[q, i] <= r2)
        for l, i in rows:
            hq.append(q)
            hid.append(i)
            ht.append(l)
            hd.append(np.sqrt(d2[q, i]))
    return dict(q=np.array(hq, dtype=np.uint32), id=np.array(hid, dtype=np.uint32),
                table=np.array(ht, dtype=np.uint32), dist=np.array(hd, dtype=np.float64), cand=cand)
