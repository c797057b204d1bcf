"""hs_pssm_compare without a GPU: the host rule (capi.pssm_compare_host) against the numpy contract of
tests/pssm_compare_ref.py bit for bit; the filter's tables against the reference; the invariant -- a pair whose rounded
score reaches t passes the filter's test -- on every (pair, offset) of a planted-family set and of matrices with a
forbidden residue; the symmetry score(x, y, d) == score(y, x, -d); the tie rule; attained thresholds; the pairs that
attain the bound; the filter's selectivity; every refused input on sentinel-filled outputs; the exports; and the header
under ASan + UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest

from hsearch_amd import capi

import pssm_compare_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 20), (3, 4), (25, 20), (26, 21), (75, 32)]


def _same_hits(got, want, what):
    for f in ("x", "y", "d"):
        assert np.array_equal(got[f], want[f]), (what, f)
    assert ref.same_bits(got["score"], want["score"]), (what, "score")
    assert np.array_equal(got["cnt"], want["cnt"]), (what, "cnt")


def _profiles(rng, n, k, A):
    """entries on a coarse grid, so that equal scores and exact cancellations do occur"""
    return rng.integers(-8, 9, size=(n, k, A)).astype(np.float64) / 4.0 * rng.integers(0, 2, size=(n, k, 1))


@pytest.fixture(scope="module")
def planted():
    P, fam, shift = ref.planted_families()
    k = P.shape[1]
    v = 13
    best, d_best = ref.best_all(P, P, v)
    tabs = ref.tables(P)
    return dict(P=P, fam=fam, shift=shift, k=k, v=v, best=best, d=d_best, tabs=tabs,
                imax=ref.int_max(tabs["q"], tabs["q"], v))


@pytest.mark.parametrize("k,A", SHAPES)
def test_host_rule_equals_numpy(k, A):
    rng = np.random.default_rng(1000 * k + A)
    sizes = [1, 15, 16, 17, 33] if k < 75 else [1, 17]
    X_all, Y_all = _profiles(rng, max(sizes), k, A), _profiles(rng, max(sizes), k, A)
    for v in sorted({1, (k + 1) // 2, k}):
        for nx, ny in zip(sizes, sizes[::-1]):
            X, Y = X_all[:nx], Y_all[:ny]
            sc = ref.best_all(X, Y, v)[0]
            t = np.quantile(sc, 0.7, axis=1)          # about a third of the pairs hit, some of them exactly at t
            t[::2] = sc[::2, 0]
            want = ref.compare(X, t, Y, v)
            assert len(want["x"]) > 0
            _same_hits(capi.pssm_compare_host(X, t, Y, v), want, (k, A, v, nx, ny))
        X = X_all[:sizes[-1]]
        t = np.quantile(ref.best_all(X, X, v)[0], 0.6, axis=1)
        want = ref.compare(X, t, None, v)
        assert np.all(want["x"] < want["y"])
        _same_hits(capi.pssm_compare_host(X, t, None, v), want, (k, A, v, "self"))


@pytest.mark.parametrize("k,A", SHAPES)
def test_tables_equal_numpy(k, A):
    rng = np.random.default_rng(k + A)
    X = rng.normal(0, 2, size=(9, k, A))
    X[1] = 0.0                                     # all zero: s = 0, codes 0
    X[2] *= 1e-290                                 # below 2^-900: no codes, l1 = +inf (every pair passes)
    X[3, 0, 0] = -1e30                             # a forbidden residue: everything else quantises to 0
    X[4] = np.abs(X[4]) * 2.0 ** 90
    X[5] = rng.integers(-127, 128, size=(k, A)) * 2.0 ** -5   # exact codes
    X[5, 0, 0] = 127 * 2.0 ** -5
    X[6] = (rng.integers(-126, 126, size=(k, A)) + 0.5) * 2.0 ** -5   # every entry on a tie: half to even
    X[6, 0, 0] = 127 * 2.0 ** -5
    got, want = capi.pssm_compare_tables(X), ref.tables(X)
    assert np.array_equal(got["q"], want["q"])
    for f in ("s", "l1", "amax"):
        assert ref.same_bits(got[f], want[f]), f
    assert got["s"][1] == 0 and got["l1"][1] == 0 and not got["q"][1].any()
    assert got["s"][2] == 0 and np.isinf(got["l1"][2]) and not got["q"][2].any()
    assert np.array_equal(got["q"][5], np.rint(X[5] * 32).astype(np.int8))
    assert np.all(got["q"][6].reshape(-1)[1:].astype(int) % 2 == 0)
    assert np.all(got["l1"] >= np.abs(X).reshape(9, -1).sum(axis=1) * (1 - 1e-12))
    assert np.abs(got["q"].astype(int)).max() <= 127


def _invariant_everywhere(P, v):
    """every (pair, offset): the rounded score, taken as the threshold, passes the test at that offset's own I"""
    n, k, A = P.shape
    tb = ref.tables(P)
    worst = 0.0
    for d in ref.offsets(k, v):
        sc = ref.score_all(P, P, d)
        I = ref.int_sums(tb["q"], tb["q"], d)
        ok = ref.passes(I, tb["s"][:, None], tb["l1"][:, None], tb["amax"][:, None], tb["s"][None, :], tb["l1"][None, :],
                        k * A, sc)
        assert ok.all(), (d, np.argwhere(~ok)[:3])
        e1, e2, e3, _ = ref.bound_terms(tb["s"][:, None], tb["l1"][:, None], tb["amax"][:, None], tb["s"][None, :],
                                        tb["l1"][None, :], k * A)
        with np.errstate(invalid="ignore", divide="ignore"):
            share = (sc - tb["s"][:, None] * tb["s"][None, :] * I) / (e1 + e2 + e3)
        worst = max(worst, float(np.nanmax(np.where(np.isfinite(share), share, 0.0))))
        # the symmetry: the same column pairs in the same order, and products commute
        assert ref.same_bits(sc, ref.score_all(P, P, -d).T), d
    return worst


def test_bound_and_symmetry_on_planted_families(planted):
    worst = _invariant_everywhere(planted["P"], planted["v"])
    assert 0.0 < worst < 1.0


def test_bound_with_forbidden_residues():
    S = ref.forbidden_profiles()
    _invariant_everywhere(S, 13)
    # ... and the filter simply passes more: the -1e30 entries own the scale, everything else quantises to zero
    tb = ref.tables(S)
    assert np.all(np.abs(tb["q"]).reshape(len(S), -1).sum(axis=1) == 3 * 127)
    best = ref.best_all(S, S, 13)[0]
    for t in (20.0, float(np.quantile(best, 0.9)), 1e61):
        pred = ref.predicted_survivors(S, t, None, 13)
        hits = ref.compare(S, t, None, 13)
        print("t = %g: %d hit pairs, %d passed" % (t, len(hits["x"]), pred.sum()))
        assert pred[hits["x"], hits["y"]].all() and pred.sum() >= len(hits["x"])
    assert len(hits["x"]) == 0


def test_tie_rule():
    k, A = 7, 4
    X = np.zeros((1, k, A))
    Y = np.zeros((2, k, A))
    X[0, 3, 1] = 1.0
    Y[0, 1, 1] = 1.0          # meets X's column at d = +2 ...
    Y[0, 5, 1] = 1.0          # ... and at d = -2: equal scores, -2 reported
    Y[1, 3, 1] = 1.0          # d = 0 ...
    Y[1, 2, 1] = 1.0          # ... and d = +1: 0 reported
    for fn in (ref.compare, capi.pssm_compare_host):
        got = fn(X, 1.0, Y, 1)
        assert list(got["y"]) == [0, 1] and list(got["d"]) == [-2, 0] and list(got["score"]) == [1.0, 1.0]
    # -0.0 and +0.0 are equal scores: the first offset in the order keeps its bits
    X2 = np.zeros((1, 3, 2))
    Y2 = np.zeros((1, 3, 2))
    X2[0, 0, 0], Y2[0, 1, 0] = -1.0, 0.0
    got = capi.pssm_compare_host(X2, 0.0, Y2, 1)
    want = ref.compare(X2, 0.0, Y2, 1)
    _same_hits(got, want, "zeros")
    assert list(got["d"]) == [0]


def test_attained_thresholds(planted):
    P, best = planted["P"][:40], planted["best"][:40, :40]
    v = planted["v"]
    x, y = 0, 1                                   # two shifts of one family
    assert planted["fam"][x] == planted["fam"][y] and planted["d"][x, y] == planted["shift"][y] - planted["shift"][x]
    t = np.full(40, np.inf)
    t = np.where(np.arange(40) == x, best[x, y], 1e300)
    got = capi.pssm_compare_host(P, t, None, v)
    at = np.flatnonzero((got["x"] == x) & (got["y"] == y))
    assert len(at) == 1 and ref.same_bits(got["score"][at], best[x, y:y + 1])
    t2 = np.where(np.arange(40) == x, np.nextafter(best[x, y], np.inf), 1e300)
    got2 = capi.pssm_compare_host(P, t2, None, v)
    assert not np.any((got2["x"] == x) & (got2["y"] == y))
    assert len(got2["x"]) == len(got["x"]) - int(np.sum(best[x, x + 1:] == best[x, y]))
    # the filter's test lets the attained threshold through
    assert ref.predicted_survivors(P, t, None, v)[x, y]


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("swap", [False, True])
def test_worst_case_of_the_bound(sign, swap):
    """The lined-up construction: every code rounds down by 0.49, all entries of one sign, d = 0.  It attains 0.97 of E
    (E's terms: 0.496, 0.501, 0.003).  A filter short of either large term rejects it.  The mixed-sign pair (the codes
    overshoot; the score is negative) adds all three terms: short of ANY of the three it is rejected.  No pair is built
    that a filter short of the rounding slack R alone loses: R is below 1e-11 of E, and E is attained to 0.97-0.998."""
    k, A = 25, 20
    X, Y = ref.lined_up_pair(k, A, sign)
    if swap:
        X, Y = Y, X
    share, terms = ref.attained_share(X, Y)
    assert share >= 0.9, share
    assert abs(terms[0] - 0.5) < 0.01 and abs(terms[1] - 0.5) < 0.01 and terms[2] < 0.01
    tx, ty = ref.tables(X), ref.tables(Y)
    sc = ref.score_all(X, Y, 0)[0, 0]
    I = ref.int_sums(tx["q"], ty["q"], 0)[0, 0]
    args = (I, tx["s"][0], tx["l1"][0], tx["amax"][0], ty["s"][0], ty["l1"][0], k * A, sc)
    assert ref.passes(*args) and capi.pssm_compare_pass(I, *args[1:6], k, A, sc)
    assert not ref.passes(*args, drop=0) and not ref.passes(*args, drop=1)
    got = capi.pssm_compare_host(X, sc, Y, k)
    assert list(got["d"]) == [0] and ref.same_bits(got["score"], [sc])
    assert ref.predicted_survivors(X, sc, Y, k).all()

    Xm, Ym = ref.lined_up_pair(k, A, sign, mixed=True, q_hi=2, frac=0.499)
    if swap:
        Xm, Ym = Ym, Xm
    share_m, terms_m = ref.attained_share(Xm, Ym)
    assert share_m >= 0.9 and min(terms_m) > 0.05, (share_m, terms_m)
    tx, ty = ref.tables(Xm), ref.tables(Ym)
    sc = ref.score_all(Xm, Ym, 0)[0, 0]
    assert sc < 0
    I = ref.int_sums(tx["q"], ty["q"], 0)[0, 0]
    args = (I, tx["s"][0], tx["l1"][0], tx["amax"][0], ty["s"][0], ty["l1"][0], k * A, sc)
    assert ref.passes(*args)
    for drop in (0, 1, 2):
        assert not ref.passes(*args, drop=drop), drop


def test_selectivity(planted):
    """at 0.4 k, 0.5 k and 0.6 k the filter passes at most 2 x the hit pairs (measured: see the printed figures)"""
    P, k, v = planted["P"], planted["k"], planted["v"]
    n = len(P)
    tb = planted["tabs"]
    upper = np.arange(n)[:, None] < np.arange(n)[None, :]
    assert upper.sum() == 69006
    for frac in (0.4, 0.5, 0.6):
        t = frac * k
        hits = (planted["best"] >= t) & upper
        ok = ref.passes(planted["imax"], tb["s"][:, None], tb["l1"][:, None], tb["amax"][:, None], tb["s"][None, :],
                        tb["l1"][None, :], k * P.shape[2], t) & upper
        print("t = %.1f: %d hit pairs, %d passed, ratio %.3f" % (t, hits.sum(), ok.sum(), ok.sum() / max(1, hits.sum())))
        assert hits.sum() > 0 and (ok | ~hits).all()
        assert ok.sum() <= 2 * hits.sum()
    # the planted shifts come back.  Column c of the master is column c - shift of a window, and column p of Y meets
    # column p + d of X: d = shift[y] - shift[x] wherever the two windows share at least v columns
    fam, shift = planted["fam"], planted["shift"]
    x, y = np.nonzero((fam[:, None] == fam[None, :]) & (fam[:, None] >= 0) & upper
                      & (np.abs(shift[:, None] - shift[None, :]) <= k - v))
    assert len(x) > 0 and np.array_equal(planted["d"][x, y], shift[y] - shift[x])
    near = shift[y] - shift[x] == 4               # 21 columns in common
    assert near.any() and (planted["best"][x, y][near] >= 0.6 * k).all()


def test_columns():
    rng = np.random.default_rng(5)
    X = rng.normal(0, 1, size=(4, 6, 20))
    X[0, 0] = 3.25                                  # a constant column: zeros under Pearson
    X[1, 1] = 0.0
    for mode, name in ((0, "pearson"), (1, "cosine")):
        got = capi.pssm_compare_columns(X, name)
        assert ref.same_bits(got, ref.columns(X, mode)), name
        nz = np.abs(got).sum(axis=2) > 0
        assert np.allclose((got ** 2).sum(axis=2)[nz], 1.0, rtol=0, atol=1e-14)
    pear = capi.pssm_compare_columns(X, "pearson")
    assert not pear[0, 0].any() and not pear[1, 1].any()
    assert np.allclose(pear.sum(axis=2), 0.0, atol=1e-14)
    assert np.allclose((pear[2] * pear[3]).sum(axis=1), [np.corrcoef(X[2, p], X[3, p])[0, 1] for p in range(6)])
    assert np.allclose(capi.pssm_compare_columns(X, "cosine")[0, 0], 1 / np.sqrt(20))
    with pytest.raises(capi.HsError):
        capi.pssm_compare_columns(X, 2)
    bad = X.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(capi.HsError):
        capi.pssm_compare_columns(bad, "pearson")


def test_refusals_write_nothing():
    import ctypes as C
    lib = capi.load()
    k, A = 3, 4
    X = np.full((2, k, A), 0.5)
    t = np.zeros(2)
    vp = capi._vp

    def call(X_=X, nx=2, Y_=None, ny=0, k_=k, A_=A, t_=t, v=1, cap=8, null_out=False):
        hx, hy = np.full(8, 9, np.uint32), np.full(8, 9, np.uint32)
        hd, hs, cnt = np.full(8, 9, np.int32), np.full(8, 9.0), np.full(2, 9, np.uint64)
        n = C.c_uint64(77)
        st = lib.hs_pssm_compare_host(vp(X_) if X_ is not None else None, C.c_uint64(nx), vp(Y_) if Y_ is not None else None,
                                      C.c_uint64(ny), C.c_uint32(k_), C.c_uint32(A_), vp(t_) if t_ is not None else None,
                                      C.c_uint32(v), None if null_out else vp(hx), vp(hy), vp(hd), vp(hs),
                                      C.c_uint64(cap), C.byref(n), vp(cnt))
        untouched = (hx == 9).all() and (hy == 9).all() and (hd == 9).all() and (hs == 9.0).all() and (cnt == 9).all()
        return st, untouched, n.value

    assert call()[0] == capi.HS_OK and call()[2] == 1
    Y = np.full((3, k, A), 0.25)
    nan_x, big_x, nan_y, inf_y = X.copy(), X.copy(), Y.copy(), Y.copy()
    nan_x[1, 2, 3], big_x[0, 0, 0], nan_y[2, 0, 1], inf_y[0, 0, 0] = np.nan, 2.6e30, np.nan, -np.inf
    cases = dict(v0=dict(v=0), v_above_k=dict(v=k + 1), nx_huge=dict(nx=1 << 27), ny_huge=dict(Y_=Y, ny=1 << 27),
                 nx0_with_y=dict(nx=0, Y_=Y, ny=3), ny0_with_x=dict(Y_=Y, ny=0), nan_x=dict(X_=nan_x),
                 big_x=dict(X_=big_x), nan_y=dict(Y_=nan_y, ny=3), inf_y=dict(Y_=inf_y, ny=3),
                 nan_t=dict(t_=np.array([0.0, np.nan])), inf_t=dict(t_=np.array([np.inf, 0.0])),
                 null_out=dict(null_out=True), null_x=dict(X_=None), null_t=dict(t_=None), k0=dict(k_=0), a0=dict(A_=0),
                 k76=dict(k_=76), a33=dict(A_=33))
    for name, kw in cases.items():
        st, untouched, n = call(**kw)
        assert st == capi.HS_ERR_INVALID and untouched and n == 0, name
    # a threshold of +-1.7e308 is a number, cap = 0 with null outputs counts, nothing asked is fine
    assert call(t_=np.array([1.7e308, -1.7e308]))[0] == capi.HS_OK
    st, _, n = call(cap=0, null_out=True)
    assert st == capi.HS_ERR_CAPACITY and n == 1
    assert call(nx=0)[0] == capi.HS_OK and call(nx=0, Y_=Y, ny=0)[0] == capi.HS_OK
    with pytest.raises(capi.HsError):
        capi.pssm_compare_tables(nan_x)


def test_exports_option_and_profile_fields():
    for name in ("hs_pssm_compare", "hs_pssm_compare_dev", "hs_pssm_compare_host", "hs_pssm_compare_tables",
                 "hs_pssm_compare_pass", "hs_pssm_compare_columns"):
        assert name in capi.EXPORTS and hasattr(capi.load(), name), name
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    assert capi.Engine.OPTIONS["pssm_cmp_filter"] == 29 and "HS_OPT_PSSM_CMP_FILTER = 29" in header
    assert '{"pssm_cmp_filter", HS_OPT_PSSM_CMP_FILTER}' in open(os.path.join(ROOT, "hsearch_amd", "csrc", "hs_capi.hip")).read()
    fields = [f[0] for f in capi._Profile._fields_]
    i = fields.index("summary_weight_items")
    assert fields[i + 1:i + 5] == ["pssm_cmp_pairs", "pssm_cmp_survivors", "pssm_cmp_steps", "pssm_rank_sample"]
    body = header[header.index("typedef struct hs_profile"):header.index("} hs_profile;")]
    assert re.findall(r"^\s*(?:double|uint64_t|uint32_t)\s+(\w+);", body, re.M) == fields


def test_header_under_asan_and_ubsan(tmp_path):
    """hs_pssm_compare.h with a stand-alone main (tests/pssm_compare_san.cpp), compiled and run under AddressSanitizer +
    UndefinedBehaviorSanitizer (the runtimes linked statically); nothing is loaded into python."""
    exe = tmp_path / "pssm_compare_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "pssm_compare_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pssm_compare_san ok" in res.stdout
