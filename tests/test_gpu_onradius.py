"""Every filter and every hit rule with pairs exactly on the radius (tests/onradius_ref.py; the premises are proved
on the CPU by tests/test_onradius_cpu.py).  A script family puts hundreds of co-bucketed pairs on one double d2;
the radii R_on (smallest double with R*R >= d2), R_sqrt = sqrt(d2) and R_off (one double below both) then decide
those pairs by the last bit, so a filter that is not one-sided -- a gamma or rho one unit too large, a float radius
term rounded to nearest, a filter fed R*R where the decision is sqrt(d2) <= R -- loses hits here and nowhere else
in the suite.  Everything is compared for exact equality with the oracle; nothing is tolerance-based and no kernel
routing is asserted."""
import numpy as np
import pytest

import hsearch_amd
from hsearch_amd import Engine
from tests import annotate_ref as ar
from tests import multiprobe_ref as mp
from tests import onradius_ref as orr
from tests import radii_ref as rr

pytestmark = pytest.mark.gpu

_FIELDS = ("q", "id", "table", "dist", "cand")
_DEFAULTS = {"seg_mode": 0, "join_resident": 0, "wide_rows": 0, "query_batch": 0, "refine8": 1, "join_min_q": 1,
             "join_min_m": 1, "recognise_kmers": 1, "self_codes": 1}
_MODES = ("auto", "stream", "join", "join16")
# the path options of step 1 (auto mode)
_OPTION_RUNS = [dict(refine8=0), dict(seg_mode=1), dict(seg_mode=2), dict(join_min_q=3, join_min_m=16),
                dict(query_batch=37), dict(join_resident=1), dict(join_resident=2), dict(wide_rows=1),
                dict(wide_rows=2)]


class _Findings(list):
    """Every comparison of a case runs; the test fails at its end with all that differed."""

    def same(self, got, want, what, fields=_FIELDS):
        for f in fields:
            if not np.array_equal(got[f], want[f]):
                self.append((what, f, "got %d want %d" % (len(got[f]), len(want[f]))))
        if "dist" in fields and len(got["dist"]) == len(want["dist"]):
            if not np.array_equal(got["dist"].view(np.uint64), want["dist"].view(np.uint64)):
                self.append((what, "dist bits"))

    def check(self, ok, what):
        if not ok:
            self.append(what)


class _Case:
    def __init__(self, oracle, name, which):
        f = orr.case_family(oracle, name, which)
        self.o, self.f, self.name = oracle, f, (name, which)
        self.table = f["table"]
        self.db_codes, self.q_codes = f["db"], f["centres"]
        self.db = orr.embed(oracle, f["db"], self.table)
        self.kmers = orr.embed(oracle, f["centres"], self.table)
        self.radii = sorted(set(f["radii"]), reverse=True)      # R_on, (R_sqrt,) R_off
        self.ix = oracle.Index(f["a"], f["b"], f["W"], self.db)
        self.eng = Engine(f["k"], f["K"], f["L"], f["W"], f["a"], f["b"], coords=self.table)
        self.eng.index_build(self.db_codes)
        self.bad = _Findings()
        self.want = {R: self.ix.query(self.kmers, R) for R in self.radii}
        q, i, _ = orr.on_radius_pairs(oracle, self.ix, self.kmers, f["radii"])
        self.on = set(zip(q.tolist(), i.tolist()))
        assert len(self.on) >= 256            # (tests/test_onradius_cpu.py proves it; never an empty premise)
        # centres that are not k-mers, and every centre's own radius (per-query radii, annotate)
        self.jit = orr.jittered(self.kmers)
        self.own_j, _ = orr.own_radii(oracle, self.ix, self.db, self.jit, orr.RANK)
        self.own_k, _ = orr.own_radii(oracle, self.ix, self.db, self.kmers, orr.RANK + 2)

    def options(self, opts):
        for name, value in opts.items():
            self.eng.set_option(name, value)

    def reset(self, opts):
        self.options({name: _DEFAULTS[name] for name in opts})
        self.eng.set_verify_mode("auto")

    def forms(self):
        """The three ways a k-mer centre enters: codes, embedded with recognition, as a point."""
        return (("codes", {}, lambda R: self.eng.query_codes(self.q_codes, R)),
                ("k-mers", {}, lambda R: self.eng.query(self.kmers, R)),
                ("points", dict(recognise_kmers=0), lambda R: self.eng.query(self.kmers, R)))

    def close(self):
        self.eng.close()
        self.ix.close()


def _scalar_search(c):
    for mode, opts in [(m, {}) for m in _MODES] + [("auto", o) for o in _OPTION_RUNS]:
        for form, form_opts, call in c.forms():
            c.eng.set_verify_mode(mode)
            c.options(dict(opts, **form_opts))
            for R in c.radii:
                c.bad.same(call(R), c.want[R], ("search", mode, opts, form, R))
            c.reset(dict(opts, **form_opts))
    if c.f["k"] <= 20:
        # 4-column rows for short k-mers: the member records change form, so the option drops the index -- one
        # rebuild for all three forms, one more on the way back
        c.eng.set_option("wide_rows", 3)
        c.eng.index_build(c.db_codes)
        for form, form_opts, call in c.forms():
            c.options(form_opts)
            for R in c.radii:
                c.bad.same(call(R), c.want[R], ("search", "auto", "wide_rows=3", form, R))
            c.reset(form_opts)
        c.eng.set_option("wide_rows", 0)
        c.eng.index_build(c.db_codes)
    if c.name[0] == "k23":  # (printed, not asserted: which row form the radius chose, against wide_rows = 2)
        for value in (0, 2):
            c.eng.set_option("wide_rows", value)
            c.eng.query_codes(c.q_codes, c.radii[0])
            prof = c.eng.profile()
            print("k23 %s R_on wide_rows=%d: join_wide %d, join_row_bytes %d, provisional %d, hits %d" %
                  (c.name[1], value, prof["join_wide"], prof["join_row_bytes"], prof["provisional"], prof["hits"]))
        c.eng.set_option("wide_rows", 0)


def _per_query_radii(c):
    nq = len(c.kmers)
    rng = np.random.default_rng(31)
    drawn = np.array(c.f["radii"])[rng.integers(0, 3, nq)]
    jit, own_j, own_k = c.jit, c.own_j, c.own_k
    calls = [("drawn", c.kmers, drawn), ("own jittered", jit, own_j), ("own k-mers", c.kmers, own_k),
             ("own jittered, lowered", jit, orr.lowered(own_j)), ("own k-mers, lowered", c.kmers, orr.lowered(own_k))]
    for what, pts, radii in calls:
        want, _ = rr.stitch(c.ix.query, pts, radii)
        c.bad.check(len(want["q"]) > 0, ("per-query radii: empty premise", what))
        runs = [(m, {}) for m in _MODES] + [("auto", dict(wide_rows=1)), ("auto", dict(query_batch=37)),
                                            ("auto", dict(recognise_kmers=0)), ("auto", dict(refine8=0))]
        for mode, opts in runs:
            c.eng.set_verify_mode(mode)
            c.options(opts)
            c.bad.same(c.eng.query_radii(pts, radii), want, ("radii", what, mode, opts))
            if pts is c.kmers:
                c.bad.same(c.eng.query_radii(c.q_codes, radii, codes=True), want, ("radii codes", what, mode, opts))
            c.reset(opts)


def _annotate(c):
    jit, own_j, own_k = c.jit, c.own_j, c.own_k
    for R in (c.radii[0], c.radii[-1]):
        want = ar.annotate(c.want[R])
        for what, got in (("codes", c.eng.annotate(c.q_codes, R=R, codes=True)), ("k-mers", c.eng.annotate(c.kmers, R=R))):
            c.bad.same(got, want, ("annotate", what, R), ar.FIELDS)
    # an on-radius hit is the farthest of its id: the rows at R_on and R_off differ
    hi, lo = ar.annotate(c.want[c.radii[0]]), ar.annotate(c.want[c.radii[-1]])
    c.bad.check(len(hi["id"]) != len(lo["id"]) or not np.array_equal(hi["q"], lo["q"]), "annotate: R_on == R_off rows")
    for what, pts, radii in (("own jittered", jit, own_j), ("own k-mers", c.kmers, own_k)):
        want = ar.annotate(rr.stitch(c.ix.query, pts, radii)[0])
        c.bad.same(c.eng.annotate(pts, radii=radii), want, ("annotate", what), ar.FIELDS)
    want = ar.annotate(rr.stitch(c.ix.query, c.kmers, own_k)[0])
    c.bad.same(c.eng.annotate(c.q_codes, radii=own_k, codes=True), want, ("annotate", "own codes"), ar.FIELDS)


def _multiprobe(c, T=4):
    f = c.f
    c.eng.set_multiprobe(T)
    for R in (c.radii[0], c.radii[-1]):
        want = mp.search(c.o, f["a"], f["b"], f["W"], c.db, c.kmers, R, T)
        for mode in _MODES:
            c.eng.set_verify_mode(mode)
            c.bad.same(c.eng.query(c.kmers, R), want, ("multi-probe", mode, "k-mers", R))
            c.bad.same(c.eng.query_codes(c.q_codes, R), want, ("multi-probe", mode, "codes", R))
        c.eng.set_verify_mode("auto")
    c.eng.set_multiprobe(0)


def _bruteforce(c, which):
    fields = ("q", "id", "dist")
    for R in c.radii:
        got = c.eng.bruteforce(c.kmers, R)
        c.bad.same(got, c.o.bruteforce(c.db, c.kmers, R), ("brute force", R), fields)
        if which == "split" and R == c.f["radii"][1]:
            # sqrt(d2) == R_sqrt although d2 > R_sqrt * R_sqrt: brute force has the pairs, the search has none
            lsh = c.eng.query(c.kmers, R)
            c.bad.check(c.on <= set(zip(got["q"].tolist(), got["id"].tolist())), "brute force lacks on-radius pairs")
            c.bad.check(not (c.on & set(zip(lsh["q"].tolist(), lsh["id"].tolist()))), "search has on-radius pairs")
    drawn = np.array(c.f["radii"])[np.random.default_rng(37).integers(0, 3, len(c.kmers))]
    want, _ = rr.stitch(lambda p, R: c.o.bruteforce(c.db, p, R), c.kmers, drawn, fields=fields)
    c.bad.same(c.eng.bruteforce_radii(c.kmers, drawn), want, "brute force radii", fields)


def _self_join_and_clustering(c, which):
    f = c.f
    pairs = orr.bucket_pairs(c.o, f["a"], f["b"], f["W"], c.db, c.radii[0])
    fields = ("i", "j", "table", "dist")
    edges = {}
    for self_codes in (1, 0):
        c.options(dict(self_codes=self_codes))
        for R in c.radii:
            for sq in (True, False):
                want = orr.edges_at(pairs, R, sq)
                got = c.eng.self_join(R, sqrt_test=sq)
                c.bad.same(got, want, ("self-join", self_codes, R, sq), fields)
                edges[(R, sq)] = set(zip(got["i"].tolist(), got["j"].tolist()))
    c.reset(dict(self_codes=1))
    # (centre, member) edges are on the radius; centre ids in the DB
    where = {row.tobytes(): i for i, row in enumerate(c.db_codes)}
    ids = [where[row.tobytes()] for row in c.q_codes]
    on = {(ids[q], i) for q, i in c.on} | {(i, ids[q]) for q, i in c.on}
    c.bad.check(on <= edges[(c.radii[0], True)] and on <= edges[(c.radii[0], False)], "self-join lacks on-radius edges")
    c.bad.check(not (on & edges[(c.radii[-1], True)]) and not (on & edges[(c.radii[-1], False)]), "edges at R_off")
    if which == "split":
        r_sqrt = f["radii"][1]
        # the two rules differ by exactly the pairs with sqrt(d2) <= R_sqrt < the covering radius of d2
        more = edges[(r_sqrt, True)] - edges[(r_sqrt, False)]
        between = (np.sqrt(pairs["d2"]) <= r_sqrt) & ~(pairs["d2"] <= r_sqrt * r_sqrt)
        want_more = set(zip(pairs["i"][between].tolist(), pairs["j"][between].tolist()))
        at_d2 = pairs["d2"] == f["d2"]
        c.bad.check(edges[(r_sqrt, False)] <= edges[(r_sqrt, True)] and more == want_more and on <= more and
                    set(zip(pairs["i"][at_d2].tolist(), pairs["j"][at_d2].tolist())) <= more,
                    "the two self-join rules at R_sqrt")
    for R in (f["radii"][1], f["radii"][2]):
        want_merged, want_owner = c.o.clustering(f["a"], f["b"], f["W"], R, c.db)
        merged, owner, _ = hsearch_amd.clustering(f["k"], f["K"], f["L"], f["W"], f["a"], f["b"], c.db_codes, R,
                                                  coords=c.table)
        c.bad.check(np.array_equal(merged, want_merged) and np.array_equal(owner, want_owner), ("clustering", R))


def _far_centres(c):
    far = c.jit.copy()
    far[:3] *= 50.0            # far outside the table: the join filters must step aside ...
    far[3:6] += 4.0e4
    radii, _ = orr.own_radii(c.o, c.ix, c.db, far, orr.RANK)
    want, _ = rr.stitch(c.ix.query, far, radii)
    c.bad.check(len(want["q"]) >= 64, "far centres: empty premise")   # ... without losing the other queries' hits
    for mode in _MODES:
        c.eng.set_verify_mode(mode)
        c.bad.same(c.eng.query_radii(far, radii), want, ("far centres", mode))
    c.eng.set_verify_mode("auto")


@pytest.mark.parametrize("name,which", orr.FAMILIES)
def test_pairs_on_the_radius(oracle, name, which):
    c = _Case(oracle, name, which)
    try:
        _scalar_search(c)
        _per_query_radii(c)
        _annotate(c)
        if name in ("k25", "k15"):
            _multiprobe(c)
        _bruteforce(c, which)
        _self_join_and_clustering(c, which)
        _far_centres(c)
    finally:
        c.close()
    assert not c.bad, (len(c.bad), c.bad[:25])
