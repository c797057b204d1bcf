"""The certainty rule of hs_proj.hip restated in numpy, and inputs built to ATTAIN its error bound: shared by
tests/test_proj_bound_cpu.py (the premises, no GPU) and tests/test_gpu_proj_bound.py (the device held to them).

The rule (header comment of hs_proj.hip):
    ex, ea   the largest e with rint(m 2^e) <= 32639, m = max |value| (per point; per coordinate table on the codes
             path; per plane)
    X = rint(x 2^ex), A = rint(a 2^ea), N = sum_i X_i A_i in exact integers
    T~ = (N 2^-(ex+ea) + b) (1/W)
    E  = x1 alpha + dx beta + 2^-49 |T~| + 2^-40
         alpha = 1.000001 (da + gamma max|a|) / W,  beta = 1.000001 |A|_1 2^-ea / W,  gamma = 1.01 (d+2) 2^-53,
         da = 2^-(ea+1), dx = 2^-(ex+1), x1 = |x|_1 (1 + 2^-40)  (codes path: the sum of the residues' l1 values)
    the value is kept when [T~ - E, T~ + E] holds no integer, recomputed in the reference's fp64 order otherwise.

The construction.  x_i = s_i (X_i + RHO) 2^-ex and a_i = sign s_i (A_i + RHO) 2^-ea with integers 8000 <= X_i, A_i <=
32000, one entry of every point / table / plane at 32000 (it pins the exponent), s_i = +-1.  Every rounding of the
quantiser then errs by RHO of its half-unit bound in the SAME direction of the product, so
    x.a - N 2^-(ex+ea) = sign 2^-(ex+ea) sum_i (RHO (X_i + A_i) + RHO^2) = sign 2 RHO (da |x|_1 + dx |A|_1 2^-ea):
the pair sits at 2 RHO of the bound's leading terms.  RHO is an input choice (how sharp the inputs are), not a
tolerance; 0.4999 still rounds to X and A and gives |t_ref - T~| / E = 0.9998.
"""
import functools

import numpy as np

QMAX = 32639
RHO = 0.4999
LO, HI = 8000, 32000
EX, EA = 12, 17                     # the intended exponents: |x| < 7.82, |a| < 0.245
ALPHABET = 23                       # rows of the custom coordinate table
BAND = (0.99, 1.01)                 # no pair but the attained ones may lie here: the flagged count is then exact


# ------------------------------------------------------------------------------------------------ the rule
def fixed_exponent(m):
    """largest e with rint(m 2^e) <= QMAX, for an array of m > 0"""
    _, e2 = np.frexp(m)
    e = 15 - e2
    return np.where(np.rint(np.ldexp(m, e)) > QMAX, e - 1, e)


def ref_dot(x, a):
    """sum_i x_i a_i strictly left to right in fp64, product and sum rounded separately (rows of x with rows of a)"""
    acc = np.zeros(np.broadcast(x[..., 0], a[..., 0]).shape)
    for i in range(x.shape[-1]):
        acc = acc + x[..., i] * a[..., i]
    return acc


def ref_t(dot, b, W):
    return (dot + b) / W


def model(pts, a, b, W, table=None, codes=None):
    """T~ and E of all n x F pairs, F = L K in the library's order (f = l K + c).  Points path: pts [n][d].  Codes path:
    table [alphabet][8] and codes [n][k] (pts is ignored): one ex for the table, x1 from the residues' l1."""
    a2 = np.asarray(a, dtype=np.float64).reshape(-1, a.shape[-1])
    bf = np.asarray(b, dtype=np.float64).reshape(-1)
    F, d = a2.shape
    ea = fixed_exponent(np.abs(a2).max(axis=1))
    A = np.rint(np.ldexp(a2, ea[:, None])).astype(np.int64)
    sa, da = np.ldexp(1.0, -ea), np.ldexp(1.0, -(ea + 1))
    gamma = 1.01 * (d + 2) * 2.0**-53
    alpha = 1.000001 * (da + gamma * np.abs(a2).max(axis=1)) / W
    beta = 1.000001 * (np.abs(A).sum(axis=1) * sa) / W
    if codes is not None:
        ex = np.full(len(codes), int(fixed_exponent(np.abs(table).max())))
        x = table[codes].reshape(len(codes), -1)
        x1 = (np.abs(table).sum(axis=1) * (1.0 + 2.0**-40))[codes].sum(axis=1) * (1.0 + 2.0**-40)
    else:
        x = np.asarray(pts, dtype=np.float64)
        ex = fixed_exponent(np.abs(x).max(axis=1))
        x1 = np.abs(x).sum(axis=1) * (1.0 + 2.0**-40)
    X = np.rint(np.ldexp(x, ex[:, None])).astype(np.int64)
    assert np.abs(X).max() <= QMAX and np.abs(A).max() <= QMAX
    sx, dx = np.ldexp(1.0, -ex), np.ldexp(1.0, -(ex + 1))
    N = (X @ A.T).astype(np.float64)                     # exact: |N| <= 416 * 32639^2 < 2^53
    T = (N * (sa[None, :] * sx[:, None]) + bf[None, :]) * (1.0 / W)
    E = x1[:, None] * alpha[None, :] + dx[:, None] * beta[None, :] + 2.0**-49 * np.abs(T) + 2.0**-40
    return dict(T=T, E=E, ex=ex, ea=ea, X=X, A=A)


def distance(T, E):
    """distance of T~ from the nearest integer in units of E; the device keeps its value iff this is >= 1 (> 1 above)"""
    frac = T - np.floor(T)
    return np.minimum(frac, 1.0 - frac) / E


def predict(case):
    m = model(case["pts"], case["a"], case["b"], case["W"], case.get("table"),
              case["codes"] if case["path"] == "codes" else None)
    return distance(m["T"], m["E"])


def counts(case):
    """(lo, hi): how many of the n F values the device must, and may, recompute: the pairs below BAND[0] -- and the
    attained pairs of a sharp case, which the bound covers by construction -- and the pairs below BAND[1]."""
    dist = predict(case)
    low, high = dist < BAND[0], dist < BAND[1]
    if case["kind"] == "sharp":
        low[case["pair_p"], case["pair_f"]] = True
    return int(low.sum()), int(high.sum())


# ------------------------------------------------------------------------------------------- the constructions
def _integers(rng, shape):
    v = rng.integers(LO, HI + 1, size=shape).astype(np.float64)
    flat = v.reshape(shape[0], -1)
    flat[np.arange(shape[0]), rng.integers(0, flat.shape[1], size=shape[0])] = HI   # pins the row's exponent
    return v


def _offsets_sharp(dot, m, W, sign):
    """b with t_ref = fl(fl(dot + b) / W) on the boundary m W, on the side away from T~: sign > 0 (T~ below m): the
    smallest b with t_ref >= m; sign < 0 (T~ above): the largest b with t_ref < m.  t_ref is monotone in b."""
    b = m * W - dot
    up, dn = np.full_like(b, np.inf), np.full_like(b, -np.inf)
    for _ in range(256):
        t = ref_t(dot, b, W)
        if sign > 0:
            step_up = t < m
            step_dn = ~step_up & (ref_t(dot, np.nextafter(b, dn), W) >= m)
        else:
            step_up = (t < m) & (ref_t(dot, np.nextafter(b, up), W) < m)
            step_dn = t >= m
        if not (step_up.any() or step_dn.any()):
            break
        b = np.where(step_up, np.nextafter(b, up), np.where(step_dn, np.nextafter(b, dn), b))
    else:
        raise AssertionError("no offset found")
    t = ref_t(dot, b, W)
    assert np.all(t >= m) if sign > 0 else np.all(t < m)
    return b


@functools.lru_cache(maxsize=None)
def _make(k, K, L, W, shift, path, sign, variant):
    """Both kinds of one case over the same points and planes; re-seeded until no pair but the attained ones lies in
    BAND, in either kind."""
    F, d = K * L, 8 * k
    n = F
    p = np.arange(n)
    f = (p + shift) % F
    for seed in range(200):
        rng = np.random.default_rng([k, K, L, shift, sign + 1, seed, len(variant), int(path == "codes")])
        A = _integers(rng, (F, d))
        table = codes = None
        scale = np.zeros(n, dtype=np.int64)
        if path == "codes":
            TX = _integers(rng, (1, ALPHABET * 8)).reshape(ALPHABET, 8)     # one ex for the whole table
            ts = np.where(rng.random((ALPHABET, 8)) < 0.5, -1.0, 1.0) if variant == "flip" else np.ones((ALPHABET, 8))
            table = np.ldexp(ts * (TX + RHO), -EX)
            codes = rng.integers(0, ALPHABET, size=(n, k), dtype=np.uint8)
            codes[0, 0], codes[n - 1, k - 1] = 0, ALPHABET - 1
            pts = table[codes].reshape(n, d)
            s = ts[codes].reshape(n, d)
        else:
            X = _integers(rng, (n, d))
            s = np.where(rng.random((n, d)) < 0.5, -1.0, 1.0) if variant == "flip" else np.ones((n, d))
            if variant == "scaled":
                scale = rng.integers(-3, 6, size=n)
                scale[:9] = np.arange(-3, 6)
            pts = np.ldexp(s * (X + RHO), (scale - EX)[:, None])
        a2 = np.empty((F, d))
        a2[f] = np.ldexp(sign * s * (A[f] + RHO), -EA)        # plane f carries the signs of its paired point
        a = a2.reshape(L, K, d)
        dot = ref_dot(pts, a2[f])
        # the boundary: 1 to 3 buckets from where the dot alone would land, so that b is no smaller than the dot's own
        # last place by much and a step of b by one ulp moves dot + b
        m = np.rint(dot / W) + rng.integers(1, 4, size=n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        b_sharp = np.empty(F)
        b_sharp[f] = _offsets_sharp(dot, m, W, sign)
        base = dict(k=k, K=K, L=L, W=float(W), shift=shift, path=path, sign=sign, variant=variant, n=n, F=F, pts=pts,
                    a=a, table=table, codes=codes, pair_p=p, pair_f=f, scale=scale, seed=seed, dot_ref=dot, m=m)
        sharp_case = dict(base, kind="sharp", b=b_sharp.reshape(L, K))
        # the clear kind: T~ of the paired point 1.25 E from the same integer, on the side it is on already
        mod = model(pts, a, sharp_case["b"], W, table, codes if path == "codes" else None)
        dotq =(mod["X"][p] * mod["A"][f]).sum(axis=1).astype(np.float64) * np.ldexp(1.0, -(mod["ex"][p] + mod["ea"][f]))
        b_clear = np.empty(F)
        b_clear[f] = (m - sign * 1.25 * mod["E"][p, f]) * W - dotq
        clear_case = dict(base, kind="clear", b=b_clear.reshape(L, K))
        ok = True
        for c in (sharp_case, clear_case):
            dist = predict(c)
            band = (dist >= BAND[0]) & (dist <= BAND[1])
            band[p, f] = False
            ok = ok and not band.any()
        if ok:
            return sharp_case, clear_case
    raise AssertionError("no seed keeps the band empty")


def sharp(k, K, L, W, shift, path, sign, variant="plain"):
    """n = F = K L points (path "points") or k-mers over a custom table (path "codes"), F planes and offsets such that
    every pair (p, (p + shift) mod F) attains the bound: t_ref within an ulp or two of an integer, T~ on its other
    side.  sign = +1: a > 0 where x > 0, T~ BELOW the integer (the (1 - frac) > E arm); sign = -1: above (frac >= E).
    variant "flip": x_i and a_i negated together at random positions; "scaled" (points): point p times 2^scale[p]."""
    return _make(k, K, L, float(W), shift, path, sign, variant)[0]


def clear(k, K, L, W, shift, path, sign, variant="plain"):
    """The same points and planes; offsets moved so that T~ of every paired point sits 1.25 E from its integer, on the
    same side: the fast pass is right there and must keep its value."""
    return _make(k, K, L, float(W), shift, path, sign, variant)[1]


# ------------------------------------------------------------------------------------------------- the cases
KS = (4, 16, 25, 40, 52)            # MFMA step counts 4, 4, 7, 10, 13; 16, 40 and 52 fill theirs exactly
SHAPES = ((7, 5), (32, 2))          # F = 35: a ragged second function tile; F = 64: K = 32 fills the per-table tiling
SHIFTS = (0, 1, 4, 17)


def width(k):
    """W with E ~ 4e-5 at every k (and 32 times that for a point scaled by 2^5)"""
    return 8.0 * k


def _cases():
    """Every k on both paths with both signs; the shapes, shifts and variants dealt round so that every (F, shift),
    every (F, path, sign) and every (path, variant) occurs (test_the_cases_cover_what_they_claim)."""
    out = []
    for ki, k in enumerate(KS):
        for pi, path in enumerate(("points", "codes")):
            for si, sign in enumerate((1, -1)):
                i = (ki * 2 + pi) * 2 + si
                K, L = SHAPES[(ki + pi + si) % 2]
                shift = SHIFTS[(i + ki) % 4]
                variant = (("plain", "flip", "scaled") if path == "points" else ("plain", "flip"))[(ki + si) % (3 - pi)]
                out.append((k, K, L, width(k), shift, path, sign, variant))
    return out


CASES = _cases()
# the codes-path cases that also go through index_build (the per-table tiling) and the query batch: both F, both signs
BUILD_CASES = [c for c in CASES if c[5] == "codes" and c[0] in (16, 25, 52)]


def case_id(c):
    return "k%d-F%d-shift%d-%s-%s-%s" % (c[0], c[1] * c[2], c[4], c[5], "below" if c[6] > 0 else "above", c[7])
