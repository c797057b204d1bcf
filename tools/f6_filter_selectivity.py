#!/usr/bin/env python3
"""How selective is the FP6 (e2m3) join filter?  numpy only, no GPU, no library.

A reduced form of bench.py's workload: 300 000 synthetic 25-mers, 600 queries derived from them, K = 16,
W = 212, R = 40, hash tables 0 and 1.  For every in-bucket (member, query) pair it evaluates

  true hit          d^2 <= R^2 over all 8 columns, fp64
  exact 4 columns   d4^2 <= R^2
  int8 bound        hs_join8.hip's header: x^ = rint(127 x / max|x|), rho and gamma with worst-case rounding terms
  FP6 / FP4 bound   hs_join6_tables.h: e2m3 (e2m1) rows, a per-residue-pair exact error e[a] + e[b] >= E[a][b],
                    thresholds rounded down to 2^-6 and lowered by one more

and writes the shares to profiles/f6_filter_selectivity.json.  The tables are re-derived here in numpy, not taken
from the library: tests/test_join6_tables_cpu.py checks the library's against the same definitions."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hsearch_amd import synth  # noqa: E402

E2M3 = np.array([(m if e == 0 else (8 + m) << (e - 1)) / 8.0 for e in range(4) for m in range(8)])
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def grid_tables(table, grid):
    """(s, X^ [A][4], e [A], r [A]) of a coordinate table for a floating-point grid of magnitudes."""
    x = np.asarray(table, dtype=np.float64)[:, :4]
    s = grid.max() / np.abs(x).max()
    v = s * x
    X = np.sign(v) * grid[np.abs(np.abs(v)[:, :, None] - grid[None, None, :]).argmin(axis=2)]
    E = s * s * (x @ x.T) - X @ X.T
    e = 0.5 * E.max(axis=1)
    A = len(x)
    for _ in range(200):
        moved = False
        for a in range(A):
            others = np.delete(E[a] - e, a)
            need = max(others.max() if A > 1 else -np.inf, 0.5 * E[a, a])
            if need < e[a]:
                e[a] = need
                moved = True
        if not moved:
            break
    r = 0.5 * s * s * (x * x).sum(axis=1) - e
    return s, X, e, r


def pass_grid(table, x, c, r2, grid=E2M3):
    """The per-residue exact bound on a grid: F >= 0 per (member x, query c) pair of code rows."""
    s, X, _, r = grid_tables(table, grid)
    S = X @ X.T
    rho = np.floor(r[x].sum(axis=1) * 64.0) / 64.0 - 1.0 / 64.0
    gamma = np.floor((r[c].sum(axis=1) - 0.5 * s * s * r2) * 64.0) / 64.0 - 1.0 / 64.0
    return S[x, c].sum(axis=1) - rho - gamma >= 0.0


def pass_f6(table, x, c, r2):
    return pass_grid(table, x, c, r2, E2M3)


def pass_int8(table, x, c, r2):
    """hs_join8.hip: acc = x^.c^ - rho - gamma >= 0 (queries that are k-mers: no saturation)."""
    t = np.asarray(table, dtype=np.float64)[:, :4]
    s = 127.0 / np.abs(t).max()
    q = np.rint(s * t)
    k = x.shape[1]
    n2 = (t * t).sum(axis=1)
    l1 = np.abs(q).sum(axis=1)
    rho = np.floor(0.5 * s * s * n2[x].sum(axis=1) - 0.5 * l1[x].sum(axis=1) - 0.25 * 4 * k - 2.0)
    gamma = np.floor(0.5 * s * s * (n2[c].sum(axis=1) - r2) - 0.5 * l1[c].sum(axis=1) - 2.0)
    return (q @ q.T)[x, c].sum(axis=1) - rho - gamma >= 0.0


def in_bucket_pairs(codes, qcodes, a, b, W):
    """(member index, query index) of all pairs that share a bucket in one of the tables a[l], b[l]."""
    t = synth.coords()
    pts, cpts = t[codes].reshape(len(codes), -1), t[qcodes].reshape(len(qcodes), -1)
    xi, ci = [], []
    for l in range(a.shape[0]):
        hb = np.floor((pts @ a[l].T + b[l]) / W).astype(np.int64)
        hq = np.floor((cpts @ a[l].T + b[l]) / W).astype(np.int64)
        _, inv = np.unique(np.concatenate([hb, hq]), axis=0, return_inverse=True)
        inv = inv.ravel()
        db_b, q_b = inv[:len(codes)], inv[len(codes):]
        order = np.argsort(db_b, kind="stable")
        lo, hi = np.searchsorted(db_b[order], q_b, "left"), np.searchsorted(db_b[order], q_b, "right")
        for q in range(len(qcodes)):
            xi.append(order[lo[q]:hi[q]])
            ci.append(np.full(hi[q] - lo[q], q, dtype=np.int64))
    return np.concatenate(xi), np.concatenate(ci)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--db-size", type=int, default=300_000)
    ap.add_argument("--queries", type=int, default=600)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--W", type=float, default=212.0)
    ap.add_argument("--R", type=float, default=40.0)
    ap.add_argument("--tables", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f6_filter_selectivity.json"))
    args = ap.parse_args()
    t = synth.coords()
    codes = synth.make_db(args.db_size, args.k)
    qcodes, _ = synth.make_query_codes(codes, args.queries)
    a, b = synth.make_planes(args.k, args.K, 8, args.W)
    xi, ci = in_bucket_pairs(codes, qcodes, a[:args.tables], b[:args.tables], args.W)
    r2 = args.R * args.R
    res = {"pairs": int(len(xi))}
    flags = {}
    step = 1 << 20
    names = ("true_hits", "exact_4_columns", "int8_bound", "fp6_e2m3_bound", "fp4_e2m1_bound")
    for n in names:
        flags[n] = np.zeros(len(xi), dtype=bool)
    for i in range(0, len(xi), step):
        x, c = codes[xi[i:i + step]], qcodes[ci[i:i + step]]
        d = t[x] - t[c]
        flags["true_hits"][i:i + step] = (d * d).sum(axis=(1, 2)) <= r2
        flags["exact_4_columns"][i:i + step] = (d[:, :, :4] ** 2).sum(axis=(1, 2)) <= r2
        flags["int8_bound"][i:i + step] = pass_int8(t, x, c, r2)
        flags["fp6_e2m3_bound"][i:i + step] = pass_grid(t, x, c, r2, E2M3)
        flags["fp4_e2m1_bound"][i:i + step] = pass_grid(t, x, c, r2, E2M1)
    hit = flags["true_hits"]
    res["pass_share"] = {n: float(flags[n].mean()) for n in names}
    res["non_hit_survivor_share"] = {n: float((flags[n] & ~hit).mean()) for n in names[1:]}
    res["hits_dropped"] = {n: int((hit & ~flags[n]).sum()) for n in names[1:]}
    s, _, e, _ = grid_tables(t, E2M3)
    res["fp6_scale"] = float(s)
    res["fp6_e_max"] = float(e.max())
    res["config"] = {k: v for k, v in vars(args).items() if k != "out"}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
