"""The contract of hs_pssm_scan in numpy (include/hsearch.h): the fp64 left-to-right score, the hit rule, the order,
the counts -- and the decode table of the filter's six-bit e2m3 codes."""
import numpy as np

# value of a six-bit e2m3 code: sign, 2 exponent bits, 3 mantissa bits
E2M3 = np.zeros(64)
for _c in range(64):
    _m, _e = _c & 7, (_c >> 3) & 3
    _v = ((8 + _m) << (_e - 1)) if _e else _m
    E2M3[_c] = (-_v if _c & 32 else _v) / 8.0


def scores(S, codes):
    """S [nm][k][A] fp64, codes [n][k] uint8 -> [nm][n]: +0.0, then S[m][p][x_p] added for p = 0 .. k-1, every sum
    rounded to fp64 (numpy adds elementwise: no pairwise summation, no FMA)."""
    S = np.asarray(S, dtype=np.float64)
    codes = np.asarray(codes)
    nm, k, _ = S.shape
    acc = np.zeros((nm, codes.shape[0]))
    for p in range(k):
        acc = acc + S[:, p, :][:, codes[:, p]]
    return acc


def scan(S, t, codes):
    """dict(m, id, score, cnt): the hits score >= t[m] in (m, id) order, and the hits per profile."""
    sc = scores(S, codes)
    hit = sc >= np.asarray(t, dtype=np.float64)[:, None]
    m, i = np.nonzero(hit)  # row-major: (m, id) ascending
    return dict(m=m.astype(np.uint32), id=i.astype(np.uint32), score=sc[m, i], cnt=hit.sum(axis=1).astype(np.uint64))


def filter_values(code, codes):
    """F [nm][n]: the sum over p of E2M3[code[m][p][x_p]] (multiples of 1/8: exact in any order)."""
    return scores(E2M3[np.asarray(code)], codes)


def euclid_profiles(centers, coords):
    """The PSSM whose score is minus the squared distance to a centre: S[q][p][a] = -sum_j (coords[a][j] -
    c[8 p + j])^2.  centers [nq][8 k], coords [A][8] -> [nq][k][A]."""
    centers = np.asarray(centers, dtype=np.float64)
    nq = centers.shape[0]
    c = centers.reshape(nq, -1, 1, 8)
    return -((np.asarray(coords)[None, None, :, :] - c) ** 2).sum(axis=3)
