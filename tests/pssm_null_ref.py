"""The rule of hs_pssm_pvalue / hs_pssm_pvalue_threshold in numpy and Python floats (IEEE doubles, one rounding per
operation, no FMA), stated from the contract in include/hsearch.h: two-sided entries, deficits on a grid of B bins,
the two integer distributions convolved position by position with residues ascending, the blocked cumulative sum,
the lookups and the threshold's bisection.  The constants are the rule's: 2^-50 on every moved quotient, 2^-48 on
delta, e = (k (alphabet + 1) + 202) 2^-52 and 1e-300 on the ladder.  Slow on purpose: the tests keep nm * k * alphabet
small where B is large."""
import struct

import numpy as np

UP = 1.0 + 2.0 ** -50
DOWN = 1.0 - 2.0 ** -50
TINY = 1e-300
BIG = 2.0 ** 108
DBL_MAX = 1.7976931348623157e308


def g_of(k):
    return float(k + 2) * 2.0 ** -52


def e_of(k, A):
    return float(k * (A + 1) + 202) * 2.0 ** -52


def two_sided(S, k):
    """T+ and T- of one profile [k][A]"""
    g = g_of(k)
    e = np.maximum(g * np.abs(S), 1e-290)
    return np.where(S == 0.0, 0.0, S + e), np.where(S == 0.0, 0.0, S - e)


def up_rel(x):
    return x + abs(x) * 2.0 ** -50


def _side(T, g):
    o = T.max(axis=1)
    so = sabs = 0.0
    for v in o:
        so = so + float(v)
        sabs = sabs + abs(float(v))
    return o, so, g * up_rel(sabs) + 1e-290


def gap_hi(pr, t):
    g0 = (pr["so_hi"] - t) + pr["c_hi"]
    if not g0 < 1e300:
        return 1e300
    if not g0 > -1e300:
        return -1e300
    return g0 + abs(g0) * 2.0 ** -50


def gap_lo(pr, t):
    g0 = (pr["so_lo"] - t) - pr["c_lo"]
    if not g0 < 1e300:
        return 1e300
    if not g0 > -1e300:
        return -1e300
    return g0 - abs(g0) * 2.0 ** -50


def j_hi(pr, B, t):
    G = gap_hi(pr, t)
    if G < 0.0:
        return -1
    x = (G / pr["delta"]) * UP
    return B if not x < B else int(x)


def j_lo(pr, B, t):
    G = gap_lo(pr, t)
    if G < 0.0:
        return -1
    x = (G / pr["delta"]) * DOWN
    return B - 1 if not x < B else int(x)


def conv(q, bg, B):
    """q [k][A] -> cdf [B]"""
    k, A = q.shape
    cur = np.zeros(B)
    cur[0] = 1.0
    for p in range(k):
        nxt = np.zeros(B)
        for a in range(A):
            s = int(q[p, a])
            if s < B:
                nxt[s:] = nxt[s:] + bg[a] * cur[:B - s]
        cur = nxt
    nblk = (B + 63) // 64
    pad = np.zeros(nblk * 64)
    pad[:B] = cur
    run = np.cumsum(pad.reshape(nblk, 64), axis=1)       # (sequential: one rounded sum per step)
    base = np.zeros(nblk)
    for b in range(nblk - 1):
        base[b + 1] = base[b] + run[b, 63]
    return (base[:, None] + run).reshape(-1)[:B]


def profile(S, bg, t_lo, B, want_lower=True):
    """One profile S [k][A]: dict(so_hi, c_hi, so_lo, c_lo, delta, dead, q_dn, q_up, cdf_dn[, cdf_up])."""
    k, A = S.shape
    g = g_of(k)
    Tp, Tm = two_sided(S, k)
    oh, so_hi, c_hi = _side(Tp, g)
    ol, so_lo, c_lo = _side(Tm, g)
    pr = dict(so_hi=so_hi, c_hi=c_hi, so_lo=so_lo, c_lo=c_lo, delta=1.0, dead=0)
    span = gap_hi(pr, max(float(t_lo), -BIG))
    if span < 0.0:
        pr["dead"] = 1
    else:
        pr["delta"] = max((span / float(B - 1)) * (1.0 + 2.0 ** -48), TINY)
    delta = pr["delta"]
    with np.errstate(over="ignore", invalid="ignore"):
        x = ((oh[:, None] - Tp) / delta) * DOWN
        q_dn = np.where(x < B, np.floor(np.minimum(x, B)), B).astype(np.uint16)
        d = ol[:, None] - Tm
        x = (d / delta) * UP
        q_up = np.where(x <= B, np.ceil(np.minimum(x, B)), B)
        q_up = np.where((q_up == 0) & (d > 0.0), 1, q_up).astype(np.uint16)
    pr.update(q_dn=q_dn, q_up=q_up, cdf_dn=conv(q_dn, bg, B))
    if want_lower:
        pr["cdf_up"] = conv(q_up, bg, B)
    return pr


def ladder_hi(c, e):
    return c * (1.0 + e) + TINY


def ladder_lo(c, e):
    v = c * (1.0 - e) - TINY
    return v if v > 0.0 else 0.0


def lookup(pr, B, e, t, want_lower=True):
    jh = j_hi(pr, B, t)
    hi = 1.0 if jh >= B else 0.0 if jh < 0 else ladder_hi(float(pr["cdf_dn"][jh]), e)
    if not want_lower:
        return hi, None
    jl = j_lo(pr, B, t)
    return hi, 0.0 if jl < 0 else ladder_lo(float(pr["cdf_up"][jl]), e)


def _key(x):
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return b ^ (0xffffffffffffffff if b >> 63 else 0x8000000000000000)


def _unkey(u):
    b = u ^ (0x8000000000000000 if u >> 63 else 0xffffffffffffffff)
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def threshold(pr, B, e, t_lo, p):
    """(t_p, flag)"""
    lad = [ladder_hi(float(c), e) for c in pr["cdf_dn"]]
    ok = [j for j in range(B) if lad[j] <= p]
    if not ok or ok[0] != 0:        # (the ladder ascends: no bin at all iff bin 0 is not admissible)
        assert not ok
        return DBL_MAX, 2
    js = max(ok)
    assert ok == list(range(js + 1))
    if js == B - 1:
        return float(t_lo), 1
    lo, hi = _key(-DBL_MAX), _key(DBL_MAX)
    while lo < hi:
        mid = (lo + hi) // 2
        if j_hi(pr, B, _unkey(mid)) <= js:
            hi = mid
        else:
            lo = mid + 1
    t = _unkey(lo)
    return (0.0 if t == 0.0 else t), 0


def tables(S, bg, t_lo, B, want_lower=True):
    """S [nm][k][A] -> the list of profile()s"""
    nm = S.shape[0]
    t_lo = np.broadcast_to(np.asarray(0.0 if t_lo is None else t_lo, dtype=np.float64), (nm,))
    return [profile(S[m], bg, float(t_lo[m]), B, want_lower) for m in range(nm)]


def pvalues(prs, k, A, B, hit_m, hit_score, want_lower=True):
    e = e_of(k, A)
    out = [lookup(prs[int(m)], B, e, float(s), want_lower) for m, s in zip(hit_m, hit_score)]
    hi = np.array([o[0] for o in out], dtype=np.float64)
    lo = np.array([o[1] for o in out], dtype=np.float64) if want_lower else None
    return hi, lo


def thresholds(prs, k, A, B, t_lo, p):
    nm = len(prs)
    e = e_of(k, A)
    t_lo = np.broadcast_to(np.asarray(0.0 if t_lo is None else t_lo, dtype=np.float64), (nm,))
    p = np.broadcast_to(np.asarray(p, dtype=np.float64), (nm,))
    t, flag, hi, lo = np.empty(nm), np.empty(nm, np.uint32), np.empty(nm), np.empty(nm)
    for m in range(nm):
        t[m], flag[m] = threshold(prs[m], B, e, float(t_lo[m]), float(p[m]))
        hi[m], lo[m] = lookup(prs[m], B, e, float(t[m]))
    return dict(t=t, flag=flag, p_hi=hi, p_lo=lo)


def log_odds_profiles(rng, nm, k, A, bg, conc=0.5):
    """Dirichlet columns against bg in bits: the profiles the measurements and the tests use"""
    f = rng.dirichlet(np.full(A, conc), size=(nm, k))
    return np.log2(np.maximum(f, 1e-6) / bg)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
