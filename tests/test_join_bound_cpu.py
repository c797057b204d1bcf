"""The premises of tests/test_gpu_join_bound.py, without a GPU: the pairs tests/join_bound_ref.py builds are true hits
that share a bucket (so the join filters see them), they use the slack of the documented bounds almost completely
under the numpy restatement of the rules, and a filter whose slack lacks one term rejects every one of them -- so a
device that passes the GPU file cannot be short of any of these terms."""
import math

import numpy as np
import pytest

from tests import join_bound_ref as jb
from tests import onradius_ref as orr

MIN_PAIRS = 200
ACC_MAX, SHARE_MIN = 8, 0.995
# refine8's margin in the int8 filters' units: twice the largest value measured (join_bound_ref's docstring)
REFINE_CAP = 17.5


def fp16_cap(R):
    """How far below 0 G of an attained pair may lie: the slack of 1.5, what 1.01 * 1.002 grants beyond the largest
    fp16 rounding error (1.3 % of 2^-9 |x1^||c1| < 0.23 at |x1||c1| < 9000), 0.1 for the hi/lo halves of the norms,
    and the part of e_c |x1^| that Cauchy-Schwarz grants and a pair at distance R cannot use:
    2^-9 (|x1||c1| - x1.c1) <= 2^-9 R^2 / 2."""
    return 1.5 + 0.23 + 0.1 + R * R / 1024.0


_ALL = ([("points",) + c for c in jb.POINTS] + [("codes",) + c for c in jb.CODES] +
        [("saturated", 25, "narrow", "narrow")])


def _case(spec):
    if spec[0] == "points":
        return jb.points_case(spec[1], spec[2]), spec[3]
    if spec[0] == "saturated":
        return jb.points_case(25, "narrow", True), "narrow"
    return jb.codes_case(spec[1]), spec[2]


def _id(spec):
    return "-".join(str(s) for s in spec)


def attained_hits(oracle, ix, case, r):
    """The attained pairs among the oracle's hits at r's radius, and the premise of the run one double below: they
    are exactly the hits that disappear there.  Returns (mask over the queries, hits at R, hits below)."""
    want = ix.query(r["pts"], r["R"])
    hits = set(zip(want["q"].tolist(), want["id"].tolist()))
    found = np.array([(q, int(i)) in hits for q, i in enumerate(r["pair_id"])])
    below = None
    if r["R"] > 0.0:
        below = ix.query(r["pts"], math.nextafter(r["R"], 0.0))
        gone = hits - set(zip(below["q"].tolist(), below["id"].tolist()))
        assert gone == {(q, int(i)) for q, i in enumerate(r["pair_id"]) if found[q]}, (len(gone), int(found.sum()))
    return found, want, below


@pytest.mark.parametrize("spec", _ALL, ids=_id)
def test_the_pairs_are_hits_where_the_filters_see_them(oracle, spec):
    case, _ = _case(spec)
    ix = oracle.Index(case["a"], case["b"], case["W"], case["db"])
    try:
        for r in case["radii"]:
            x = jb.embed(case["table"], case["db_codes"][r["pair_id"]])
            d2 = np.array([oracle.pairwise_square(x[i:i + 1], r["pts"][i:i + 1])[0, 0] for i in range(len(x))])
            assert np.all(d2 == r["d2"]) and np.array_equal(case["db_codes"][r["pair_id"]], r["members"])
            assert r["R"] == orr.covering_radius(r["d2"])
            found, want, below = attained_hits(oracle, ix, case, r)
            print("%s R = %.4f: %d attained hits of %d pairs, %d hits in all, %d below" % (
                _id(spec), r["R"], found.sum(), len(found), len(want["q"]), -1 if below is None else len(below["q"])))
            assert found.sum() >= MIN_PAIRS
            assert len(want["q"]) < 64 * len(r["pts"])          # (the search's default capacity)
    finally:
        ix.close()
    radii = [r["R"] for r in case["radii"]]
    if spec[0] != "saturated":
        assert radii[0] == 0.0 and 2.0 <= radii[1] <= 8.0 and radii[2] >= 11.5    # none, small, large


def _expected_loss(case, r):
    """what a pinned coordinate cannot use of its share (join_bound_ref's docstring): 63.5 + u / 2, u = 6 then 9"""
    if not case["saturated"]:
        return np.zeros(len(r["members"]))
    pins = (r["members"] == 0).sum(axis=1)
    return np.where(pins == 1, 63.5 + 3.0, 127.0 + 7.5)


@pytest.mark.parametrize("spec", _ALL, ids=_id)
def test_the_int8_pairs_are_tight(spec):
    case, form = _case(spec)
    figures = jb.int8_figures(case, form)
    for g, (r, f) in enumerate(zip(case["radii"], figures)):
        if g not in jb.tight_radii(case, form):
            assert f["rho_fits"].all() and f["gamma_fits"].all() and f["safe"].all() and np.all(f["acc"] >= 0)
            continue
        loss = _expected_loss(case, r)
        share = 1.0 - f["acc"] / f["slack"]
        print("%s (%s rows) R = %.4f: acc %d..%d, slack %.0f..%.0f, share >= %.5f" % (
            _id(spec), form, r["R"], f["acc"].min(), f["acc"].max(), f["slack"].min(), f["slack"].max(), share.min()))
        assert f["rho_fits"].all() and f["gamma_fits"].all() and f["safe"].all()
        assert np.all(f["acc"] >= 0) and np.all(f["acc"] <= ACC_MAX + loss)
        if case["saturated"]:
            assert np.all(f["pen"] >= 127.5 * 5.5) and np.all(share >= 1.0 - (ACC_MAX + loss) / f["slack"])
            assert share.min() >= 0.95
        else:
            assert share.min() >= SHARE_MIN
        if case["source"] == "points" and not case["saturated"]:
            assert np.all(f["pen"] == 0.0)


def _concerned(drop, spec, case, form):
    if spec[0] == "saturated":
        # (a pinned coordinate leaves more unused than dims/4 or one position's L1 amount to)
        return drop in ("l1x", "l1c", "pen")
    if drop == "dims4k":
        return form == "wide"
    if drop == "recpos":
        return form == "narrow" and 8 * jb.ks_of(case["k"]) - 8 < case["k"]
    return drop != "pen"


@pytest.mark.parametrize("drop", jb.DROPS)
def test_a_filter_short_of_one_term_rejects_every_pair(drop):
    seen = 0
    for spec in _ALL:
        case, form = _case(spec)
        if not _concerned(drop, spec, case, form):
            continue
        seen += 1
        figures = jb.int8_figures(case, form, drop)
        for f in [figures[g] for g in jb.tight_radii(case, form)]:
            assert np.all(f["acc"] < 0), (drop, _id(spec), int(f["acc"].max()))
    assert seen >= 1


def test_the_wide_pairs_need_all_eight_columns_counted():
    """... and the narrow-form model over the wide cases' pairs, for contrast: the all8 shifts are NOT tight for
    the 4-column filter (part of the distance lies in columns 4..7), which is why those cases are read as wide"""
    case = jb.points_case(23, "all8")
    f = jb.int8_figures(case, "narrow")[2]
    assert f["acc"].min() > 100


@pytest.mark.parametrize("k", [25, 39, 50])
def test_the_all8_pairs_are_tight_for_refine8(k):
    case = jb.points_case(k, "all8")
    T = jb.tables(case["table"])
    for r in case["radii"]:
        f = jb.refine8(T, r["members"], r["pts"], r["R"])
        margin = (f["rhs"] + f["tol"] - f["lhs"]) * f["units"]
        print("refine8 k = %d R = %.4f: margin %.3f..%.3f units, of which tol %.3f..%.3f" % (
            k, r["R"], margin.min(), margin.max(), (f["tol"] * f["units"]).min(), (f["tol"] * f["units"]).max()))
        assert np.all(margin >= 0.0) and np.all(margin <= REFINE_CAP)
    # the narrow shifts leave columns 4..7 alone: tight there as well
    case = jb.points_case(k, "narrow")
    for r in case["radii"]:
        f = jb.refine8(T, r["members"], r["pts"], r["R"])
        margin = (f["rhs"] + f["tol"] - f["lhs"]) * f["units"]
        assert np.all(margin >= 0.0) and np.all(margin <= REFINE_CAP)


def test_the_fp16_pairs_are_tight(oracle):
    case = jb.fp16_case()
    t = case["table"]
    assert np.all(np.abs(t[:, :4]).astype(np.float16).astype(np.float64) < np.abs(t[:, :4]))      # all round down
    ix = oracle.Index(case["a"], case["b"], case["W"], case["db"])
    try:
        for r in case["radii"]:
            found, want, _ = attained_hits(oracle, ix, case, r)
            assert found.sum() >= MIN_PAIRS
            G = jb.fp16_G(t, r["members"], r["pts"], r["R"])
            half = jb.fp16_G(t, r["members"], r["pts"], r["R"], ec_factor=0.5)
            nc = (r["pts"].reshape(len(G), 25, 8)[:, :, :4] ** 2).sum(axis=(1, 2))
            print("fp16 R = %.4f: G %.4f..%.4f; with e_c halved %.4f..%.4f; |c1|^2 <= %.0f, %d hits" % (
                r["R"], G.min(), G.max(), half.min(), half.max(), nc.max(), len(want["q"])))
            assert np.all(G < 0.0) and np.all(G >= -fp16_cap(r["R"]))
            assert np.all(half > 0.0)                      # the weakened filter rejects every pair
            assert nc.max() < 30000.0 and r["R"] ** 2 < 30000.0
    finally:
        ix.close()


def test_the_cases_cover_what_they_claim():
    narrow = {jb.ks_of(k) for k, _, form in jb.POINTS if form == "narrow"}
    assert narrow == {4, 6, 8}
    assert {jb.ks_of(k, True) for k, _, form in jb.POINTS if form == "wide"} == {6, 8}
    assert {jb.ks_of(k, True) for k, form in jb.CODES if form == "wide"} == {6, 8}
    assert {jb.ks_of(k) for k, form in jb.CODES if form == "narrow"} == {4, 6, 8}
    # the record's position exists in a narrow case of 4 and of 6 k-steps (8 k-steps: never, k <= 50 < 56)
    assert {jb.ks_of(k) for k, _, form in jb.POINTS if form == "narrow" and 8 * jb.ks_of(k) - 8 < k} == {4, 6}
    # the scales are exactly 8 and the float roundings of the device change nothing
    for k in sorted({c[0] for c in jb.POINTS} | {c[0] for c in jb.CODES}):
        T = jb.tables(jb.int8_table(k))
        assert (T["s"], T["s2"], T["sw"], T["half"], T["halfw"]) == (8.0, 8.0, 8.0, 32.0, 32.0)
        assert np.abs(T["q4"][1:]).max() <= 40 and T["q4"][0, 0] == 127 and T["qB"][0, 0] == -127
        assert np.array_equal(T["qw"][:, :4], T["q4"]) and np.array_equal(T["qw"][:, 4:], T["qB"])
        # families: columns 4..7 shared, columns 0..3 apart by integers over s
        t = jb.int8_table(k)
        for f in range(jb.FAMILIES):
            rows = t[1 + 4 * f:5 + 4 * f]
            assert np.all(rows[:, 4:] == rows[0, 4:])
            d = (rows[:, None, :4] - rows[None, :, :4]) * jb.S
            assert np.all(d == np.rint(d)) and len(np.unique(rows[:, :4], axis=0)) == 4
    # no attained member holds the pin residue, except where the case is about it
    for spec in _ALL:
        case, _ = _case(spec)
        for r in case["radii"]:
            assert ((r["members"] == 0).sum() > 0) == (spec[0] == "saturated")
    assert {c["source"] for c in (_case(s)[0] for s in _ALL)} == {"points", "codes"}
