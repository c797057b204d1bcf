"""The rule of hs_pssm_compare in numpy (not collected): the contract, the int8 filter's tables and test, the column
transform, and the constructions the tests share.  Vectorised across PAIRS, never across residues or columns: every
product and every sum below is one rounded fp64 operation, in the contract's order."""
import numpy as np

MAX_ABS = 2.0 ** 100
TINY = 2.0 ** -900
U40 = 2.0 ** -40


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def offsets(k, v):
    """the allowed offsets in the tie order: 0, -1, +1, -2, +2, ..."""
    out = [0]
    for a in range(1, k - v + 1):
        out += [-a, a]
    return out


def score_all(X, Y, d):
    """score(x, y, d) for every pair: [nx][ny]"""
    k, A = X.shape[1:]
    sc = np.zeros((X.shape[0], Y.shape[0]))
    for p in range(max(0, -d), min(k, k - d)):
        col = np.zeros_like(sc)
        for r in range(A):
            col = col + X[:, p + d, r][:, None] * Y[:, p, r][None, :]
        sc = sc + col
    return sc


def best_all(X, Y, v):
    """(best [nx][ny], d [nx][ny]) under the tie rule"""
    k = X.shape[1]
    best = d_best = None
    for d in offsets(k, v):
        sc = score_all(X, Y, d)
        if best is None:
            best, d_best = sc, np.zeros(sc.shape, dtype=np.int32)
        else:
            up = sc > best
            best = np.where(up, sc, best)
            d_best = np.where(up, np.int32(d), d_best)
    return best, d_best


def compare(X, t, Y=None, v=1):
    """dict(x, y, d, score, cnt): the contract's hits in (x, y) order"""
    X = np.asarray(X, dtype=np.float64)
    nx = X.shape[0]
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (nx,))
    self_mode = Y is None
    Yp = X if self_mode else np.asarray(Y, dtype=np.float64)
    if nx == 0 or Yp.shape[0] == 0:
        z = np.zeros(0, dtype=np.uint32)
        return dict(x=z, y=z, d=np.zeros(0, np.int32), score=np.zeros(0), cnt=np.zeros(nx, np.uint64))
    best, d_best = best_all(X, Yp, v)
    hit = best >= t[:, None]
    if self_mode:
        hit &= np.arange(nx)[:, None] < np.arange(nx)[None, :]
    x, y = np.nonzero(hit)          # row-major: (x, y) ascending
    return dict(x=x.astype(np.uint32), y=y.astype(np.uint32), d=d_best[x, y].astype(np.int32), score=best[x, y],
                cnt=hit.sum(axis=1).astype(np.uint64))


# ---- the filter's tables and test (hs_pssm_compare.h) ----------------------------------------------------------------
def tables(X):
    """dict(q int8 [nx][k][A], s, l1, amax [nx]) in the header's order of operations"""
    X = np.asarray(X, dtype=np.float64)
    nx = X.shape[0]
    flat = np.abs(X.reshape(nx, -1))
    n = flat.shape[1]
    part = np.zeros((nx, 64))
    for i in range(n):
        part[:, i & 63] = part[:, i & 63] + flat[:, i]
    lanes = np.arange(64)
    for w in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ w]
    total = part[:, 0]
    amax = flat.max(axis=1) if n else np.zeros(nx)
    ok = amax >= TINY
    s = np.where(ok, amax / 127.0, 0.0)
    l1 = np.where(amax == 0.0, 0.0, np.where(ok, total + total * U40, np.inf))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(ok[:, None], np.rint(X.reshape(nx, -1) / np.where(ok, s, 1.0)[:, None]), 0.0)
    return dict(q=q.astype(np.int8).reshape(X.shape), s=s, l1=l1, amax=amax)


def int_sums(qx, qy, d):
    """I(x, y, d) = the exact integer sum of code products over the overlap: [nx][ny] int64"""
    k = qx.shape[1]
    lo, hi = max(0, -d), min(k, k - d)
    a = qx[:, lo + d:hi + d, :].astype(np.int64).reshape(qx.shape[0], -1)
    b = qy[:, lo:hi, :].astype(np.int64).reshape(qy.shape[0], -1)
    return a @ b.T


def int_max(qx, qy, v):
    k = qx.shape[1]
    out = None
    for d in offsets(k, v):
        I = int_sums(qx, qy, d)
        out = I if out is None else np.maximum(out, I)
    return out


def bound_terms(sx, l1x, amaxx, sy, l1y, n):
    """(E1, E2, E3, R): the three quantisation terms and the rounding slack, each as the test computes it"""
    ss = sx * sy
    return (0.5 * sx) * l1y, (0.5 * sy) * l1x, (0.25 * float(n)) * ss, (float(n) * 2.0 ** -52) * (amaxx * l1y)


def passes(I, sx, l1x, amaxx, sy, l1y, n, t, drop=None):
    """hs_pcmp_pass, vectorised over pairs.  drop in (0, 1, 2, 3): the model filter short of that term (tests only)"""
    with np.errstate(invalid="ignore", over="ignore"):
        ss = sx * sy
        c = ss * np.asarray(I, dtype=np.float64)
        e1, e2, e3, r = bound_terms(sx, l1x, amaxx, sy, l1y, n)
        if drop is not None:
            e1, e2, e3, r = [np.zeros_like(v) if i == drop else v for i, v in enumerate((e1, e2, e3, r))]
        E = e1 + e2 + e3
        M = np.abs(c) + E + r
        ub = c + E + r + U40 * M + 2.0 ** -1000
        return ~(ub < t)


def predicted_survivors(X, t, Y=None, v=1):
    """bool [nx][ny]: the pairs the device's filter passes, from the tables"""
    tx = tables(X)
    ty = tx if Y is None else tables(Y)
    nx, k, A = np.asarray(X).shape
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (nx,))
    I = int_max(tx["q"], ty["q"], v)
    ok = passes(I, tx["s"][:, None], tx["l1"][:, None], tx["amax"][:, None], ty["s"][None, :], ty["l1"][None, :], k * A,
                t[:, None])
    if Y is None:
        ok &= np.arange(nx)[:, None] < np.arange(nx)[None, :]
    return ok


def columns(X, mode):
    """hs_pssm_compare_columns in its order of operations (mode 0 Pearson, 1 cosine)"""
    X = np.asarray(X, dtype=np.float64)
    A = X.shape[-1]
    if mode == 0:
        total = np.zeros(X.shape[:-1])
        for r in range(A):
            total = total + X[..., r]
        Z = X - (total / float(A))[..., None]
    else:
        Z = X
    ssq = np.zeros(X.shape[:-1])
    for r in range(A):
        ssq = ssq + Z[..., r] * Z[..., r]
    norm = np.sqrt(ssq)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(norm[..., None] > 0.0, Z / norm[..., None], 0.0)


# ---- constructions ---------------------------------------------------------------------------------------------------
def planted_families(seed=7, k=25, A=20, families=12, members=6, n_random=300, width=45, draws=40):
    """(profiles [families * members + n_random][k][A] as Pearson columns, family [n] (-1: random), shift [n]): every
    family is `members` windows of one master of `width` columns, shifted by 0, 4, 8, ... and multinomially resampled;
    the random profiles are resampled Dirichlet columns of their own."""
    rng = np.random.default_rng(seed)
    prof, fam, shift = [], [], []
    for f in range(families):
        master = rng.dirichlet(np.full(A, 0.3), size=width)
        for j in range(members):
            s = 4 * j
            win = master[s:s + k]
            prof.append(np.stack([rng.multinomial(draws, c) / float(draws) for c in win]))
            fam.append(f)
            shift.append(s)
    for _ in range(n_random):
        cols = rng.dirichlet(np.full(A, 0.3), size=k)
        prof.append(np.stack([rng.multinomial(draws, c) / float(draws) for c in cols]))
        fam.append(-1)
        shift.append(0)
    return columns(np.array(prof), 0), np.array(fam), np.array(shift)


def forbidden_profiles(seed=11, n=24, k=25, A=20):
    """log-odds-like matrices of order 1 with a forbidden residue of -1e30 in some columns"""
    rng = np.random.default_rng(seed)
    S = rng.normal(0.0, 1.5, size=(n, k, A))
    for m in range(n):
        for p in rng.choice(k, size=3, replace=False):
            S[m, p, rng.integers(A)] = -1e30
    return S


def lined_up_pair(k, A, sign=1, mixed=False, seed=3, q_hi=126, frac=0.49):
    """A pair whose quantisation errors all line up at d = 0.  Entries s (q + frac) with one entry exactly 127 s, so
    that every code rounds DOWN by frac; sign = -1: both profiles negated (the products, the codes' products and the
    deviation keep their signs).  mixed: x = s (q - frac) > 0 against y = -s (p - frac) < 0 -- the codes overshoot, the
    score is negative (the cancellation side) and all three terms of E add up."""
    rng = np.random.default_rng(seed)
    n = k * A
    sx, sy = 2.0 ** -7, 2.0 ** -3          # powers of two: s (q + frac) and x / s are exact
    if mixed:
        q = rng.integers(1, q_hi + 1, size=n).astype(np.float64)
        p = rng.integers(1, q_hi + 1, size=n).astype(np.float64)
        x = sx * (q - frac)
        y = -sy * (p - frac)
    else:
        q = rng.integers(0, q_hi + 1, size=n).astype(np.float64)
        p = rng.integers(0, q_hi + 1, size=n).astype(np.float64)
        x = sx * (q + frac)
        y = sy * (p + frac)
    x[0] = 127.0 * sx
    y[n - 1] = (-127.0 if mixed else 127.0) * sy
    return (sign * x).reshape(1, k, A), (sign * y).reshape(1, k, A)


def attained_share(X, Y):
    """(real score - s_x s_y I) / E at d = 0 of the pair (X[0], Y[0]), in exact rational arithmetic; and E's three terms
    as shares of E"""
    from fractions import Fraction
    tx, ty = tables(X), tables(Y)
    x, y = X.reshape(-1), Y.reshape(-1)
    real = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(x, y))
    I = int(int_sums(tx["q"], ty["q"], 0)[0, 0])
    sx, sy = Fraction(float(tx["s"][0])), Fraction(float(ty["s"][0]))
    l1x, l1y = (sum(Fraction(abs(float(a))) for a in z) for z in (x, y))
    terms = [sx / 2 * l1y, sy / 2 * l1x, Fraction(len(x)) * sx * sy / 4]
    E = sum(terms)
    return float((real - sx * sy * I) / E), [float(v / E) for v in terms]
