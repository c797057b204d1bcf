"""The join filters' rules restated in numpy, and inputs built to ATTAIN their error bounds: shared by
tests/test_join_bound_cpu.py (the premises, no GPU) and tests/test_gpu_join_bound.py (the device held to them).

The rules (header comments of hs_join8.hip and hs_join.hip).
  int8 rows   x^ = rint(s x), c^ = rint(s c) saturated to +-127, s = 127 / max |entry| of the row form's columns;
              rho = floor(s^2 |x1|^2 / 2 - L1(x^)/2 - dims/4 - 2)           (hs_gather_rec8_kernel)
              gamma = floor(s^2 (|c1|^2 - R^2) / 2 - L1(c^)/2 - pen - 2)    (hs_qprep8_kernel, hs_qprep8_codes_kernel)
              pen = sum 127.5 max(0, |s c_i - c^_i| - 1/2);  a pair passes iff acc = x^.c^ - rho - gamma >= 0.
              narrow rows: columns 0..3, dims = 4k;  wide rows: all 8 columns on one scale, dims = 8k.
              The slack the bound grants a pair is L1(x^)/2 + L1(c^)/2 + dims/4 + pen + 4; a pair's attained share
              of it is 1 - acc / slack.
  refine8     lhs = |x|^2 + (|c|^2 - R^2), rhs = 2 (uA + uB), u = (x^.c^ + L1(x^)/2 + e + 4k/4) / s^2 per column half
              with e = the float, rounded up, of L1(c^)/2 + pen + 2; passes unless lhs > rhs + tol,
              tol = 1e-5 (|x|^2 + ||c|^2 - R^2| + 1).
  fp16 join   G = |x1|^2 + |c1|^2 - 2 x1^.c1^ - R^2 - 1.5 - e_c |x1^|, e_c = 1.01 2^-9 |c1|; passes iff G < 0.
  FP6 join    F of a pair from the library's own host exports (capi.join6_tables / join6_thresholds): f6_figure.
Every float32 the device keeps is kept here: scale[0..5], the tables' squared norms, refine8's sum of them, the two
rounded-up floats of a query's second row.  Products and sums that the device rounds in an order of its own (a wave's
tree of partial sums) are exact for the tables below -- their entries are 21-bit dyadic numbers -- so the order does
not matter; for other tables the model may differ from the device in the last place of a floor.

The construction (int8).  Alphabet 21.  Every entry of the table is sign_j (m + 1/2 - DELTA) / 8 with an integer m and
one sign per column j; residue 0, the pin, holds exactly 127/8 in columns 0 and 4, so the narrow scale, the scale of
columns 4..7 and the wide scale are all exactly 8.  Residues 1..20 are five families of four that share columns 4..7.
Then x^ = sign m and every quantisation error is e = sign (1/2 - DELTA).  A query c = x + t/8 with an integer vector t
that keeps every sign has c^ = x^ + t and the same errors, so x^.n, e.c^ and e.n all take their maximum at once:
    x^.c^ = s^2 x.c - (1/2 - DELTA)(L1(x^) + L1(c^)) - (1/2 - DELTA)^2 dims,
and where t lies inside the filter's columns |x1 - c1|^2 = d2 = R^2 makes the geometric step tight too.  What is left
of the slack is the +2 +2 rounding allowance, two floors and DELTA (L1(x^) + L1(c^) + dims).

Measured on these cases (tests/test_join_bound_cpu.py prints them; it asserts the bounds in brackets):
    int8 narrow rows, points, k = 15 / 25 / 39 / 41 / 50      acc 5..6    share >= 0.99518 (k = 15; 0.9975 from k = 25)
    int8 wide rows, points, k = 15 / 23                       acc 5..6    share >= 0.99781
    int8 narrow rows, codes, k = 21 / 25 / 39 / 50            acc 5..6    share >= 0.99681   (large radii: n_big)
    int8 wide rows, codes, k = 15 / 23                        acc 5..6    share >= 0.99778
        [asserted for all four: 0 <= acc <= 8, share >= 0.995, rho and -gamma inside their digits]
    int8 saturated, k = 25, 1 or 2 pinned coordinates         acc 72..140 share >= 0.96862
        This construction cannot reach 0.995.  A pinned coordinate has x^ = 127 and e = 0: of the 127.5 u + 63.5 units
        the bound grants it (u = 6 or 9: how far the query coordinate lies outside, in units of 1/s) only x^.n = 127 u
        can be used, so 63.5 + u/2 stay unused per pinned coordinate: 66.5 with one, 134.5 with two.
        [asserted: 0 <= acc <= 8 + that, and the share that follows from it, which is >= 0.95 at these slacks]
    all8 shifts under 4-column rows are tight for the join at R = 0 only (part of the distance lies in columns 4..7).
    refine8, narrow and all8 points, k = 25 / 39 / 50         (rhs + tol - lhs) s^2 / 2 = 5.83 .. 8.71 units, of which
        the tolerance term is 1.25 .. 3.38 and each half's + 2 another 4              [asserted: 0 .. 17.5 = twice that]
    fp16, k = 25                                              G = -1.76 .. -1.59 at R = 0, -2.01 .. -1.86 at R = 16.1,
        -3.78 .. -3.66 at R = 45.8; with e_c halved G = +1.03 .. +7.08                [asserted: -fp16_cap(R) <= G < 0]
    FP6, codes, k = 21 / 25 (test_gpu_join_bound.py prints it)  F = 78 .. 452 units of 2^-6: not tight, by design
"""
import functools
import math

import numpy as np

from hsearch_amd import capi, synth
from tests import onradius_ref

S = 8.0
PIN = 127.0 / S
DELTA = 2.0 ** -14
ALPHABET = 21
FAMILIES = 5                        # residues 1 + 4 f .. 4 + 4 f share columns 4..7
SIGN = np.array([1.0, -1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0])
DIG, RDIG = 13, 11                  # base-127 digits of -gamma and of rho
N_ATT, N_NOISE = 288, 2600          # attained members (= queries) per radius; random bucket mates
K_PLANES, L_PLANES = 2, 3

# the weakenings test_join_bound_cpu.py applies one at a time
DROPS = ("l1x", "l1c", "dims", "dims4k", "recpos", "pen")


def ks_of(k, wide=False):
    """k-steps of 32 bytes in a row (hs_join8.hip)"""
    if wide:
        return 6 if k <= 20 else 8
    return 4 if k <= 25 else 6 if k <= 41 else 8


def _f32(x):
    return np.asarray(np.asarray(x, dtype=np.float32), dtype=np.float64)


def _f32_up(x):
    """__double2float_ru"""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    f = np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)
    return f.astype(np.float64)


def _q127(v):
    return np.clip(np.rint(v), -127, 127).astype(np.int64)


def _fits(v, nd):
    """does v fit nd base-127 digits and a remainder (digits127)"""
    return np.abs(np.floor_divide(v, 127)) <= 127 * nd


# ------------------------------------------------------------------------------------------------ the rules
def tables(table):
    """hs_jtables8_kernel: the quantised rows, the float-rounded scales and squared norms"""
    t = np.asarray(table, dtype=np.float64)
    n4 = np.zeros(len(t))
    for j in range(4):
        n4 = n4 + t[:, j] * t[:, j]
    n8, nB = n4.copy(), np.zeros(len(t))
    for j in range(4, 8):
        n8 = n8 + t[:, j] * t[:, j]
        nB = nB + t[:, j] * t[:, j]
    mm, mm2 = np.abs(t[:, :4]).max(), np.abs(t[:, 4:]).max()
    s = 127.0 / mm
    s2 = float(_f32(127.0 / mm2))
    sw = 127.0 / max(mm, mm2)
    return dict(s=float(_f32(s)), half=float(_f32(0.5 * s * s)), q4=_q127(s * t[:, :4]), n4=n4, n4f=_f32(n4),
                s2=s2, qB=_q127(s2 * t[:, 4:]), nB=nB, n8f=_f32(n8),
                sw=float(_f32(sw)), halfw=float(_f32(0.5 * sw * sw)), qw=_q127(sw * t))


def members(T, codes, wide, drop=None):
    """hs_gather_rec8_kernel: x^ [n][dims], L1(x^), rho, and whether rho fits its digits"""
    n, k = codes.shape
    q = (T["qw"] if wide else T["q4"])[codes]
    l1p = np.abs(q).sum(axis=2)
    plast = 8 * ks_of(k) - 8
    if drop == "recpos" and not wide and plast < k:
        l1p[:, plast] = 0
    l1 = l1p.sum(axis=1)
    nx = (T["n8f"] if wide else T["n4f"])[codes].sum(axis=1)         # floats summed in double: exact
    dims = (8 if wide else 4) * k
    used = 4 * k if (drop == "dims4k" and wide) else dims
    rho = T["halfw" if wide else "half"] * nx - (0.0 if drop == "l1x" else 0.5 * l1)
    rho = np.floor(rho - (0.0 if drop == "dims" else 0.25 * used) - 2.0).astype(np.int64)
    return dict(xq=q.reshape(n, -1), l1=l1, rho=rho, fits=_fits(rho, RDIG), dims=dims)


def _gamma(sA, nc, r2, l1, pen, drop):
    g = 0.5 * sA * sA * (nc - r2) - (0.0 if drop == "l1c" else 0.5 * l1) - (0.0 if drop == "pen" else pen) - 2.0
    g = np.floor(g).astype(np.int64)
    return g, _fits(-g, DIG)


def queries_points(T, pts, k, R, wide, drop=None):
    """hs_qprep8_kernel: c^ [n][dims], L1(c^), the saturation penalty, gamma, and whether -gamma fits"""
    c = np.asarray(pts, dtype=np.float64).reshape(len(pts), k, 8)
    v = c if wide else c[:, :, :4]
    sA = T["sw"] if wide else T["s"]
    sv = sA * v
    qv = _q127(sv)
    pen = (127.5 * np.maximum(0.0, np.abs(sv - qv) - 0.5)).sum(axis=(1, 2))
    nc = (v * v).sum(axis=(1, 2))
    l1 = np.abs(qv).sum(axis=(1, 2))
    g, fits = _gamma(sA, nc, R * R, l1, pen, drop)
    safe = (np.abs(sv).max(axis=(1, 2)) < 1.0e6) & (pen < 30000.0) & (np.abs(g) < 1.0e9)
    return dict(cq=qv.reshape(len(pts), -1), l1=l1, pen=pen, gamma=g, fits=fits, safe=safe, nc=nc)


def queries_codes(T, codes, R, wide, drop=None):
    """hs_qprep8_codes_kernel: the table's own quantised rows, norms from the table's doubles, no penalty"""
    n, k = codes.shape
    q = (T["qw"] if wide else T["q4"])[codes]
    nc = ((T["n4"] + T["nB"]) if wide else T["n4"])[codes].sum(axis=1)
    l1 = np.abs(q).sum(axis=(1, 2))
    g, fits = _gamma(T["sw"] if wide else T["s"], nc, R * R, l1, np.zeros(n), drop)
    return dict(cq=q.reshape(n, -1), l1=l1, pen=np.zeros(n), gamma=g, fits=fits, safe=np.ones(n, dtype=bool), nc=nc)


def acc_of(mem, qry, pair_m=None):
    """(acc, granted slack) of the pairs (member pair_m[i], query i)"""
    m = np.arange(len(qry["gamma"])) if pair_m is None else pair_m
    dot = (mem["xq"][m] * qry["cq"]).sum(axis=1)
    acc = dot - mem["rho"][m] - qry["gamma"]
    slack = 0.5 * mem["l1"][m] + 0.5 * qry["l1"] + 0.25 * mem["dims"] + qry["pen"] + 4.0
    return acc, slack


def refine8(T, mcodes, pts, R):
    """hs_refine8_kernel for the pairs (mcodes[i], pts[i]): lhs, rhs and the tolerance term; the pair passes unless
    lhs > rhs + tol.  units = s^2 / 2 turns rhs + tol - lhs into the int8 filters' units."""
    n, k = mcodes.shape
    c = np.asarray(pts, dtype=np.float64).reshape(n, k, 8)
    u, nc = [], 0.0
    for half, s, qx in ((slice(0, 4), T["s"], T["q4"]), (slice(4, 8), T["s2"], T["qB"])):
        v = c[:, :, half]
        sv = s * v
        qv = _q127(sv)
        pen = (127.5 * np.maximum(0.0, np.abs(sv - qv) - 0.5)).sum(axis=(1, 2))
        e = _f32_up(0.5 * np.abs(qv).sum(axis=(1, 2)) + pen + 2.0)
        x = qx[mcodes]
        dot = (x * qv).sum(axis=(1, 2))
        u.append((dot + 0.5 * np.abs(x).sum(axis=(1, 2)) + e + 0.25 * (4 * k)) * (1.0 / (s * s)))
        nc = nc + (v * v).sum(axis=(1, 2))
    nx = np.zeros(n, dtype=np.float32)
    for p in range(k):                                  # fp32, position by position
        nx = nx + T["n8f"][mcodes[:, p]].astype(np.float32)
    nx = nx.astype(np.float64)
    cq = nc - R * R
    return dict(lhs=nx + cq, rhs=2.0 * (u[0] + u[1]), tol=1e-5 * (nx + np.abs(cq) + 1.0), units=0.5 * T["s"] ** 2)


def fp16_G(table, mcodes, pts, R, ec_factor=1.0):
    """hs_jtables_kernel, hs_qprep_kernel and hs_join_kernel (k <= 25) for the pairs (mcodes[i], pts[i]): G, summed
    here in double where the MFMA accumulates in fp32"""
    t = np.asarray(table, dtype=np.float64)
    n, k = mcodes.shape
    tab16 = t[:, :4].astype(np.float32).astype(np.float16).astype(np.float64)
    norm = np.zeros(len(t))
    for j in range(4):
        norm = norm + t[:, j] * t[:, j]
    norm = norm.astype(np.float32)
    nx = np.zeros(n, dtype=np.float32)
    for p in range(k):
        nx = nx + norm[mcodes[:, p]]
    nhi = nx.astype(np.float16)
    nlo = (nx - nhi.astype(np.float32)).astype(np.float16)
    xn = (np.sqrt(nx) * np.float32(1.002)).astype(np.float16)
    c = np.asarray(pts, dtype=np.float64).reshape(n, k, 8)[:, :, :4]
    nc = (c * c).sum(axis=(1, 2))
    c16 = c.astype(np.float32).astype(np.float16).astype(np.float64)
    v = (nc - R * R - 1.5).astype(np.float32)
    vhi = v.astype(np.float16)
    vlo = (v - vhi.astype(np.float32)).astype(np.float16)
    ec = (np.sqrt(nc) * (1.01 / 512.0) * ec_factor).astype(np.float32).astype(np.float16)
    dot = (tab16[mcodes] * c16).sum(axis=(1, 2))
    f = lambda h: h.astype(np.float64)
    return f(nhi) + f(nlo) + f(vhi) + f(vlo) - 2.0 * dot - f(ec) * f(xn)


def _e2m3_eighths(code):
    code = np.asarray(code, dtype=np.int64)
    m, e = code & 7, (code >> 3) & 3
    v = np.where(e > 0, (8 + m) << np.maximum(e - 1, 0), m)
    return np.where(code & 32, -v, v)


def f6_figure(table, mcodes, qcodes, R):
    """F of the pairs (mcodes[i], qcodes[i]) in units of 2^-6, from what the library's host exports hand out (the
    kernel keeps a pair whose F is not negative)"""
    X8 = _e2m3_eighths(capi.join6_tables(table)["codes"])
    S64 = (X8 @ X8.T).astype(np.int64)
    mem = capi.join6_thresholds(table, mcodes, 0.0)
    qry = capi.join6_thresholds(table, qcodes, R * R)
    return S64[mcodes, qcodes].sum(axis=1) - (mem["rho64"] - mem["rho0_64"]) + qry["c64"]


# ------------------------------------------------------------------------------------------- the constructions
def _m_range(k):
    """magnitudes that keep rho and -gamma inside their digits at every radius of the cases"""
    return (8, 40) if k <= 41 else (8, 35)


@functools.lru_cache(maxsize=None)
def int8_table(k):
    rng = np.random.default_rng([88, k])
    lo, hi = _m_range(k)
    m = rng.integers(lo, hi + 1, size=(ALPHABET, 8)).astype(np.float64)
    fam = rng.integers(lo, hi + 1, size=(FAMILIES, 4)).astype(np.float64)
    m[1:, 4:] = np.repeat(fam, 4, axis=0)
    t = SIGN * (m + 0.5 - DELTA) / S
    t[0, 0], t[0, 4] = SIGN[0] * PIN, SIGN[4] * PIN
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def fp16_table():
    """entries +-2^e (1 + 2^-11 - 2^-20): each rounds DOWN to 2^e in fp16, with the largest relative error"""
    rng = np.random.default_rng(1616)
    e = rng.integers(1, 5, size=(ALPHABET, 8))
    fam = rng.integers(1, 5, size=(FAMILIES, 4))
    e[1:, 4:] = np.repeat(fam, 4, axis=0)
    for f in range(FAMILIES):            # no two residues of a family alike in columns 0..3
        rows = e[1 + 4 * f:5 + 4 * f, :4]
        while len(np.unique(rows, axis=0)) < 4:
            rows[:] = rng.integers(1, 5, size=(4, 4))
    t = SIGN * np.ldexp(1.0 + 2.0 ** -11 - 2.0 ** -20, e)
    t.setflags(write=False)
    return t


def embed(table, codes):
    return np.ascontiguousarray(table[codes].reshape(len(codes), -1))


def _members(rng, n, k):
    """k-mers without the pin residue"""
    return rng.integers(1, ALPHABET, size=(n, k), dtype=np.uint8)


def _noise(rng, n, k):
    return rng.integers(0, ALPHABET, size=(n, k), dtype=np.uint8)


def _multiset(rng, D, R):
    """D integers with sum of squares ~ 64 R^2: the shifts' magnitudes (towards larger |c^|), a third of the small
    ones negative (towards smaller |c^|: never below 8 - 7 = 1)"""
    tot = 64.0 * R * R
    nnz = int(min(D, max(1, tot // 9)))
    vals = np.zeros(D, dtype=np.int64)
    vals[:nnz] = np.maximum(1, np.rint(math.sqrt(tot / nnz) * rng.uniform(0.6, 1.4, size=nnz)))
    flip = (vals > 0) & (vals <= 7) & (rng.random(D) < 1.0 / 3.0)
    return np.where(flip, -vals, vals)


def _planes(k, W):
    return synth.make_planes(k, K_PLANES, L_PLANES, W)


def _shuffled(rng, parts):
    """the DB of the parts in one random order, and where every row of every part went"""
    db = np.concatenate(parts)
    perm = rng.permutation(len(db))
    where = np.empty(len(db), dtype=np.int64)
    where[perm] = np.arange(len(db))
    out, at = [], 0
    for p in parts:
        out.append(where[at:at + len(p)])
        at += len(p)
    return np.ascontiguousarray(db[perm]), out


# target radii of the points cases: none, small, and about 0.85 of the typical distance of two random k-mers of the
# table (beyond it the random bucket mates become hits by the hundred thousand)
R_BIG = {15: 15.0, 23: 19.0, 25: 20.0, 39: 25.0, 41: 25.0, 50: 27.0}
R_SMALL = 3.0


@functools.lru_cache(maxsize=None)
def points_case(k, shifts, saturated=False):
    """dict(k, table, a, b, W, K, L, db_codes, db, radii: [dict(R, d2, pts [n][8k], pair_id [n], members [n][k])]).
    Query i of a radius is DB k-mer pair_id[i] plus t/8; shifts "narrow": t in columns 0..3, "all8": in all."""
    rng = np.random.default_rng([25, k, int(shifts == "all8"), int(saturated)])
    table = int8_table(k)
    cols = np.arange(4) if shifts == "narrow" else np.arange(8)
    targets = (R_SMALL,) if saturated else (0.0, R_SMALL, R_BIG[k])
    groups = [_members(rng, N_ATT, k) for _ in targets]
    pushes = np.array([6, 9])
    if saturated:
        # one or two positions hold the pin residue: x^ = 127 in column 0 there
        for i, x in enumerate(groups[0]):
            x[rng.choice(k, size=1 + i % 2, replace=False)] = 0
    db_codes, ids = _shuffled(rng, groups + [_noise(rng, N_NOISE, k)])
    radii = []
    for g, target in enumerate(targets):
        x = groups[g]
        D = k * len(cols)
        base = _multiset(rng, D - (2 if saturated else 0), target) if target > 0 else np.zeros(D, dtype=np.int64)
        t = np.zeros((len(x), k, 8))
        for i in range(len(x)):
            if saturated:
                # the pushes sit on the pinned coordinates; with one pinned position the other push is an ordinary shift
                pins = np.flatnonzero(x[i] == 0)
                free = np.ones((k, len(cols)), dtype=bool)
                free[pins, 0] = False
                row = np.zeros((k, len(cols)), dtype=np.int64)
                row[pins, 0] = pushes[:len(pins)]
                rest = np.concatenate([base, pushes[len(pins):]])
                row[free] = rng.permutation(np.concatenate([rest, np.zeros(free.sum() - len(rest), dtype=np.int64)]))
                t[i][:, cols] = row
            else:
                t[i][:, cols] = rng.permutation(base).reshape(k, len(cols))
        pts = embed(table, x) + (SIGN * t / S).reshape(len(x), -1)
        d2 = float((t[0] * t[0]).sum() / (S * S))                   # exact: every term is an integer / 64
        radii.append(dict(R=onradius_ref.covering_radius(d2), d2=d2, pts=np.ascontiguousarray(pts), pair_id=ids[g],
                          members=x))
    W = 8.0 * max(r["R"] for r in radii)
    a, b = _planes(k, W)
    return dict(k=k, table=table, a=a, b=b, W=W, K=K_PLANES, L=L_PLANES, db_codes=db_codes, db=embed(table, db_codes),
                radii=radii, shifts=shifts, saturated=saturated, source="points",
                name="points-k%d-%s%s" % (k, shifts, "-saturated" if saturated else ""))


def _script(rng, table, n_sub, far):
    """n_sub ordered substitutions (src, dst) inside families; far: the pairs of a family furthest apart"""
    src, dst = np.empty(n_sub, dtype=np.uint8), np.empty(n_sub, dtype=np.uint8)
    for i in range(n_sub):
        f = 1 + 4 * rng.integers(0, FAMILIES)
        pairs = [(x, y) for x in range(f, f + 4) for y in range(f, f + 4) if x != y]
        if far:
            pairs.sort(key=lambda p: -float(((table[p[0]] - table[p[1]]) ** 2).sum()))
            pairs = pairs[:4]
        src[i], dst[i] = pairs[rng.integers(0, len(pairs))]
    return src, dst


def _d2_sequential(x, c):
    acc = np.zeros(len(x))
    for i in range(x.shape[1]):
        acc = acc + (x[:, i] - c[:, i]) * (x[:, i] - c[:, i])
    return acc


def _codes_case(name, k, table, seed, n_small, n_big):
    rng = np.random.default_rng([77, k, seed])
    groups, queries = [], []
    for n_sub, far in ((0, False), (n_small, False), (n_big, True)):
        x = _members(rng, N_ATT, k)
        c = x.copy()
        if n_sub:
            src, dst = _script(rng, table, n_sub, far)
            for i in range(len(x)):
                pos = np.sort(rng.choice(k, size=n_sub, replace=False))     # the script in order, as in onradius_ref
                x[i, pos] = src
                c[i] = x[i]
                c[i, pos] = dst
        groups.append(x)
        queries.append(c)
    # the queries of the radii > 0 are DB k-mers too: the same pairs serve the self-join
    db_codes, ids = _shuffled(rng, groups + queries[1:] + [_noise(rng, N_NOISE, k)])
    assert len(np.unique(db_codes, axis=0)) == len(db_codes)
    radii = []
    for g in range(3):
        d2 = _d2_sequential(embed(table, groups[g][:1]), embed(table, queries[g][:1]))[0]
        radii.append(dict(R=onradius_ref.covering_radius(float(d2)), d2=float(d2), codes=queries[g],
                          pts=embed(table, queries[g]), pair_id=ids[g], members=groups[g],
                          self_id=ids[2 + g] if g else ids[0]))
    W = 8.0 * max(r["R"] for r in radii)
    a, b = _planes(k, W)
    return dict(k=k, table=table, a=a, b=b, W=W, K=K_PLANES, L=L_PLANES, db_codes=db_codes, db=embed(table, db_codes),
                radii=radii, shifts="narrow", saturated=False, source="codes", name=name)


def n_big(k):
    """Substitutions of the codes cases' large radius: about half the positions up to k = 25, two thirds beyond.
    Each one, between the residues of a family furthest apart, adds about 16 to d2, so the radius is 12..16 up to
    k = 25 and reaches the searches' usual 20..40 only for the long k-mers.  More does not work for the short ones:
    the members of a radius all carry the script's source residues, so with most positions planted they are near
    copies of each other, and pairs other than the attained ones then lie exactly on the radius (k = 15: none with
    8 substitutions, 4..41 with 10 or 12) -- the run one double below could no longer count the attained pairs."""
    return k // 2 + 1 if k <= 25 else (2 * k) // 3


@functools.lru_cache(maxsize=None)
def codes_case(k):
    """Queries that are k-mers: members with substitutions inside families (columns 0..3 only), one ordered script
    per radius so that all its pairs share one d2.  radii[g] as in points_case, plus codes [n][k] and self_id [n]
    (the query's own DB id; radius 0: the member's)."""
    return _codes_case("codes-k%d" % k, k, int8_table(k), 0, 2, n_big(k))


@functools.lru_cache(maxsize=None)
def fp16_case():
    """k = 25 over fp16_table(): a member itself (R = 0, entered as a point) and members with 2 and 6 residues
    exchanged inside families"""
    return _codes_case("fp16-k25", 25, fp16_table(), 16, 2, 6)


# ------------------------------------------------------------------------------------------------- the cases
# (k, shifts, row form the case is meant for): the form decides which model the CPU premises hold the pairs to
POINTS = [(25, "narrow", "narrow"), (25, "all8", "narrow"), (39, "narrow", "narrow"), (39, "all8", "narrow"),
          (41, "narrow", "narrow"), (50, "narrow", "narrow"), (50, "all8", "narrow"),
          (15, "all8", "wide"), (23, "all8", "wide"), (15, "narrow", "narrow")]
CODES = [(25, "narrow"), (39, "narrow"), (50, "narrow"), (21, "narrow"), (15, "wide"), (23, "wide")]


def tight_radii(case, form):
    """the radii (indices) at which the case's pairs are tight for the int8 filter of row form `form`: all of them,
    but for all8 shifts under 4-column rows -- part of their distance lies in columns 4..7, so beyond R = 0 they
    are tight for hs_refine8_kernel and the wide rows only"""
    return [0] if (case["shifts"] == "all8" and form == "narrow") else list(range(len(case["radii"])))


def int8_figures(case, form, drop=None):
    """per radius: (acc, slack, rho fits, -gamma fits, safe) of the attained pairs under the row form `form`"""
    T = tables(case["table"])
    wide = form == "wide"
    out = []
    for r in case["radii"]:
        mem = members(T, r["members"], wide, drop)
        if case["source"] == "codes":
            qry = queries_codes(T, r["codes"], r["R"], wide, drop)
        else:
            qry = queries_points(T, r["pts"], case["k"], r["R"], wide, drop)
        acc, slack = acc_of(mem, qry)
        out.append(dict(acc=acc, slack=slack, rho_fits=mem["fits"], gamma_fits=qry["fits"], safe=qry["safe"],
                        pen=qry["pen"]))
    return out
