"""The premises of tests/test_gpu_proj_bound.py, proved on the numpy model of the certainty rule (proj_ref): no GPU.

The GPU tests hold hs_proj.hip to `bucket integers == oracle` and `hash_flagged == the count the model predicts` on
inputs that are claimed to attain the error bound E of the MFMA pass.  That means something only if, for every case
the GPU file runs,
  * the quantiser's exponents are the intended ones, so X and A are the integers the construction chose,
  * the fast pass ALONE is wrong at every attained pair: floor(T~) != floor(t_ref), t_ref being the oracle's,
  * the pair attains the bound: |t_ref - T~| / E >= 0.99,
  * the matching clear case (T~ at 1.25 E) is decided rightly by the fast pass, and
  * no other pair sits within 1 % of the bound, so the flagged count is one number.
The minimum attained ratio over all cases is 0.999799 (= 2 RHO / 1.000001 less the 2^-40 and 2^-49 |T~| terms): an E
more than 0.02 % too small -- alpha or beta off, a position missing from x1 (0.96 % of E at k = 52) -- turns into a
wrong bucket integer."""
import numpy as np
import pytest

import proj_ref
from proj_ref import CASES, case_id


def _model(case):
    return proj_ref.model(case["pts"], case["a"], case["b"], case["W"], case["table"],
                          case["codes"] if case["path"] == "codes" else None)


def _t_ref(case):
    """the reference's t of the paired pairs, from the model's left-to-right fp64 sum"""
    f = case["pair_f"]
    a2, bf = case["a"].reshape(case["F"], -1), case["b"].reshape(-1)
    return proj_ref.ref_t(proj_ref.ref_dot(case["pts"], a2[f]), bf[f], case["W"])


def test_the_cases_cover_what_they_claim():
    assert {(c[0], c[5], c[6]) for c in CASES} == {(k, p, s) for k in proj_ref.KS for p in ("points", "codes")
                                                   for s in (1, -1)}
    assert {(c[1] * c[2], c[4]) for c in CASES} == {(F, s) for F in (35, 64) for s in proj_ref.SHIFTS}
    assert {(c[1] * c[2], c[5], c[6]) for c in CASES} == {(F, p, s) for F in (35, 64) for p in ("points", "codes")
                                                          for s in (1, -1)}
    assert {(c[5], c[7]) for c in CASES} == {("points", "plain"), ("points", "flip"), ("points", "scaled"),
                                             ("codes", "plain"), ("codes", "flip")}
    assert {(c[1] * c[2], c[6]) for c in proj_ref.BUILD_CASES} == {(35, 1), (35, -1), (64, 1), (64, -1)}
    assert all(c[1] * c[2] <= 130 for c in CASES)
    # every function row of both tiles (the ragged one of F = 35 too) and every point lane holds an attained pair
    for c in CASES:
        s = proj_ref.sharp(*c)
        assert sorted(s["pair_f"]) == list(range(s["F"])) and sorted(s["pair_p"]) == list(range(s["n"]))


def test_fixed_exponent_is_the_largest():
    m = np.array([1.0, 0.99609375, 32639.4, 32639.6, 16319.7, 16319.8, 1e-7, 3e9, 2.0**-30, 0.2441444])
    e = proj_ref.fixed_exponent(m)
    assert np.all(np.rint(np.ldexp(m, e)) <= proj_ref.QMAX) and np.all(np.rint(np.ldexp(m, e + 1)) > proj_ref.QMAX)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_exponents_are_the_intended_ones(case):
    for c in (proj_ref.sharp(*case), proj_ref.clear(*case)):
        m = _model(c)
        assert np.array_equal(m["ea"], np.full(c["F"], proj_ref.EA))
        assert np.array_equal(m["ex"], proj_ref.EX - c["scale"])
        if c["variant"] == "scaled":
            assert set(c["scale"]) == set(range(-3, 6))
        # the integers the quantiser sees: within [8000, 32000], the maximum attained in every plane and point / table
        assert np.abs(m["A"]).min() >= proj_ref.LO and np.all(np.abs(m["A"]).max(axis=1) == proj_ref.HI)
        assert np.abs(m["X"]).min() >= proj_ref.LO and np.abs(m["X"]).max() == proj_ref.HI
        if c["path"] == "points":
            assert np.all(np.abs(m["X"]).max(axis=1) == proj_ref.HI)
            # ... and the residuals all lie RHO from the integer, on the side of the value's sign
            r = np.ldexp(c["pts"], m["ex"][:, None]) - m["X"]
            assert np.allclose(r * np.sign(m["X"]), proj_ref.RHO, rtol=0, atol=1e-9)
        if c["variant"] == "flip":
            assert (m["X"] < 0).any() and (m["X"] > 0).any()
            assert (m["X"] % 256 >= 128).any()          # negative low digits too


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_sharp_pairs_attain_the_bound_and_fool_the_fast_pass(oracle, case):
    c = proj_ref.sharp(*case)
    m, p, f = _model(c), c["pair_p"], c["pair_f"]
    want = oracle.hash_all(c["a"], c["b"], c["W"], c["pts"]).reshape(c["n"], c["F"])
    t_ref = _t_ref(c)
    assert np.array_equal(np.floor(t_ref).astype(np.int32), want[p, f])     # the model's t_ref is the oracle's
    T, E = m["T"][p, f], m["E"][p, f]
    bad = np.flatnonzero(np.floor(T).astype(np.int32) == want[p, f])
    assert bad.size == 0, "pair (%d, %d): the fast pass alone is right" % (p[bad[0]], f[bad[0]])
    # T~ lies on the side the case names, t_ref within a few ulps of the integer on the other
    edge = np.rint(T)
    assert np.all(T < edge) if c["sign"] > 0 else np.all(T >= edge)
    assert np.all(t_ref >= edge) if c["sign"] > 0 else np.all(t_ref < edge)
    assert np.all(np.abs(t_ref - edge) <= 2.0**-44)     # one ulp of b (|b| < 32 W) over W, one of t (|t| < 32)
    ratio = np.abs(t_ref - T) / E
    print("%s: |t_ref - T~| / E in [%.6f, %.6f], E in [%.3g, %.3g]" % (case_id(case), ratio.min(), ratio.max(),
                                                                      E.min(), E.max()))
    assert ratio.min() >= 0.99 and ratio.max() <= 1.0
    # the bound holds at every other pair as well (it is a proven bound: this checks the MODEL against the oracle)
    all_ref = proj_ref.ref_t(proj_ref.ref_dot(c["pts"][:, None, :], c["a"].reshape(1, c["F"], -1)), c["b"].reshape(-1),
                             c["W"])
    assert np.array_equal(np.floor(all_ref).astype(np.int32), want)
    assert np.all(np.abs(all_ref - m["T"]) <= m["E"])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_clear_pairs_are_decided_by_the_fast_pass(oracle, case):
    c = proj_ref.clear(*case)
    m, p, f = _model(c), c["pair_p"], c["pair_f"]
    want = oracle.hash_all(c["a"], c["b"], c["W"], c["pts"]).reshape(c["n"], c["F"])
    assert np.array_equal(np.floor(m["T"][p, f]).astype(np.int32), want[p, f])
    dist = proj_ref.distance(m["T"], m["E"])[p, f]
    assert np.all(np.abs(dist - 1.25) < 1e-3)
    s = proj_ref.sharp(*case)
    assert np.array_equal(c["pts"], s["pts"]) and np.array_equal(c["a"], s["a"]) and c["codes"] is s["codes"]
    # the same side of the same integer as in the sharp case
    assert np.array_equal(np.rint(m["T"][p, f]), np.rint(_model(s)["T"][p, f]))
    assert np.all(m["T"][p, f] < np.rint(m["T"][p, f])) if c["sign"] > 0 else np.all(m["T"][p, f] > np.rint(m["T"][p, f]))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_no_other_pair_near_the_bound(case):
    """... so the count of recomputed values is one number: lo == hi."""
    for c in (proj_ref.sharp(*case), proj_ref.clear(*case)):
        dist = proj_ref.predict(c)
        band = (dist >= proj_ref.BAND[0]) & (dist <= proj_ref.BAND[1])
        paired = np.zeros_like(band)
        paired[c["pair_p"], c["pair_f"]] = True
        if c["kind"] == "sharp":
            assert np.all(dist[paired] >= proj_ref.BAND[0]) and np.all(dist[paired] < 1.0)
            assert not (band & ~paired).any()
        else:
            assert not band.any()
        lo, hi = proj_ref.counts(c)
        assert lo == hi and lo == int((dist < 1.0).sum())
        assert (lo >= c["n"]) if c["kind"] == "sharp" else (lo < c["n"])


def test_minimum_attained_ratio():
    """The figure the docstring and DESIGN.md 5 quote."""
    worst = min(np.min(np.abs(_t_ref(c) - _model(c)["T"][c["pair_p"], c["pair_f"]]) / _model(c)["E"][c["pair_p"], c["pair_f"]])
                for c in (proj_ref.sharp(*case) for case in CASES))
    print("minimum attained |t_ref - T~| / E over %d cases: %.6f" % (len(CASES), worst))
    assert worst >= 0.99
    assert abs(worst - 0.999799) < 2e-6
