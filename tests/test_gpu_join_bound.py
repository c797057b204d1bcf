"""The join filters held to their error bounds: true hits whose quantisation errors all line up, so that a pair uses
at least 99.5 % of the slack its int8 filter's bound grants (96.9 % in the saturated case: join_bound_ref.py says why;
the premises are proved on the CPU by tests/test_join_bound_cpu.py: the pairs are hits that share a bucket, the numpy
restatement of the int8 rule passes them by 5 or 6 units of 1231..6551, and a filter short of any one term of its
slack rejects them all).  A device
filter short of such a term -- dims/4 dropped, the saturation penalty not charged, L1 without the record's position, 4k
for 8k on the wide rows, e_c a factor of two small -- loses these hits.

Everything is compared with the oracle for exact equality (dist bit for bit), at every radius of a case and, on the
radius, one double below it, where the attained pairs must disappear and nothing else.  A profile counter proves per
run that the filter form the case is about ran: a silent fallback fails the test.  Survivor counts are not asserted."""
import math

import numpy as np
import pytest

from hsearch_amd import Engine
from tests import join_bound_ref as jb
from tests import onradius_ref as orr

pytestmark = pytest.mark.gpu

_FIELDS = ("q", "id", "table", "dist", "cand")
_WANT = {}                 # the oracle's answers, computed once per (case, radius, on / below)




class _Run:
    """one Engine and one oracle index over a case's DB"""

    def __init__(self, oracle, case, form, options=None):
        self.o, self.case, self.form = oracle, case, form
        self.ix = oracle.Index(case["a"], case["b"], case["W"], case["db"])
        self.eng = Engine(case["k"], case["K"], case["L"], case["W"], case["a"], case["b"], coords=case["table"],
                          options=options)
        self.eng.index_build(case["db_codes"])

    def close(self):
        self.eng.close()
        self.ix.close()

    def options(self, **opts):
        for name, value in opts.items():
            self.eng.set_option(name, value)

    def want(self, g, below=False, first=None):
        """the oracle's hits of radius g's queries (the first `first` of them) at R, or one double below"""
        r = self.case["radii"][g]
        key = (self.case["name"], g, below, first)
        if key not in _WANT:
            R = math.nextafter(r["R"], 0.0) if below else r["R"]
            _WANT[key] = (R, self.ix.query(r["pts"][:first], R))
        return _WANT[key]

    def radii(self):
        """(g, below) of every run of the case: each radius, and the ones > 0 one double below as well"""
        out = []
        for g, r in enumerate(self.case["radii"]):
            out.append((g, False))
            if r["R"] > 0.0:
                out.append((g, True))
        return out

    def explain(self, g, got, want, R):
        """the first hit the library lacks, with the model's figures if it is an attained pair"""
        r = self.case["radii"][g]
        have = set(zip(got["q"].tolist(), got["id"].tolist()))
        lost = [(q, i) for q, i in zip(want["q"].tolist(), want["id"].tolist()) if (q, i) not in have]
        if not lost:
            return "no hit lost; got %d hits, oracle %d" % (len(got["q"]), len(want["q"]))
        q, i = lost[0]
        msg = "%d hits lost; first: query %d, id %d at R = %r" % (len(lost), q, i, R)
        if int(r["pair_id"][q]) != i:
            return msg + " (not an attained pair)"
        if self.form not in ("narrow", "wide"):
            return msg + " (an attained pair)"
        T = jb.tables(self.case["table"])
        wide = self.form == "wide"
        mem = jb.members(T, r["members"][q:q + 1], wide)
        if self.case["source"] == "codes":
            qry = jb.queries_codes(T, r["codes"][q:q + 1], R, wide)
        else:
            qry = jb.queries_points(T, r["pts"][q:q + 1], self.case["k"], R, wide)
        acc, slack = jb.acc_of(mem, qry)
        return msg + "; model (%s rows): x^.c^ = %d, rho = %d, gamma = %d, acc = %d of a slack of %.2f, pen = %.2f" % (
            self.form, acc[0] + mem["rho"][0] + qry["gamma"][0], mem["rho"][0], qry["gamma"][0], acc[0], slack[0],
            qry["pen"][0])

    def check(self, g, below, got, what, first=None):
        R, want = self.want(g, below, first)
        for f in _FIELDS:
            assert np.array_equal(got[f], want[f]), (what, f, self.explain(g, got, want, R))
        assert np.array_equal(got["dist"].view(np.uint64), want["dist"].view(np.uint64)), (what, "dist bits")
        # the attained pairs: among the hits on the radius, gone one double below, and nothing else with them
        r = self.case["radii"][g]
        n = len(r["pts"][:first])
        hits = set(zip(got["q"].tolist(), got["id"].tolist()))
        att = {(q, int(i)) for q, i in enumerate(r["pair_id"][:n])}
        if below:
            _, on = self.want(g, False, first)
            assert not (att & hits), what
            n_on = len(att & set(zip(on["q"].tolist(), on["id"].tolist())))
            assert len(on["q"]) - len(got["q"]) == n_on and n_on >= min(200, n - 8), what
        else:
            assert len(att & hits) >= min(200, n - 8), what

    def sweep(self, call, what, proof=None, first=None):
        """every radius of the case through `call(g, R)`; proof(profile) after each"""
        for g, below in self.radii():
            R, _ = self.want(g, below, first)
            got = call(g, R)
            prof = self.eng.profile()
            self.check(g, below, got, (what, g, below), first)
            if proof:
                proof(prof)

    def other_modes(self, call, what, first=None):
        """verify modes auto and stream: whatever they choose, equality only"""
        for mode in ("auto", "stream"):
            self.eng.set_verify_mode(mode)
            self.sweep(call, (what, mode), None, first)
        self.eng.set_verify_mode("join")


def _points(run, first=None):
    return lambda g, R: run.eng.query(run.case["radii"][g]["pts"][:first], R)


def _codes(run):
    return lambda g, R: run.eng.query_codes(run.case["radii"][g]["codes"], R)


@pytest.mark.parametrize("shifts", ["narrow", "all8"])
def test_k25_points_on_4_column_rows(oracle, shifts):
    """hs_join8x_kernel, hs_join8r_kernel and hs_refine8_kernel<1>: narrow shifts are tight for the join, all8 shifts
    for the refinement"""
    case = jb.points_case(25, shifts)
    run = _Run(oracle, case, "narrow", dict(recognise_kmers=0, wide_rows=2))
    try:
        run.eng.set_verify_mode("join")

        def streaming(prof):
            assert prof["join_i8_batches"] > 0 and prof["join_items_resident"] == 0 and prof["join_wide"] == 0
            assert prof["join_row_bytes"] == 128

        def resident(prof):
            assert prof["join_i8_batches"] > 0 and prof["join_items_resident"] > 0 and prof["join_wide"] == 0

        for refine8 in (1, 0):
            run.options(refine8=refine8, join_resident=1)
            run.sweep(_points(run), ("join8x", refine8), streaming)
            # at most 64 probing queries per bucket: every segment is in the resident kernel's class
            run.options(join_resident=2)
            run.sweep(_points(run, 64), ("join8r", refine8), resident, first=64)
        run.options(refine8=1, join_resident=0)
        run.other_modes(_points(run), "k25")
    finally:
        run.close()


@pytest.mark.parametrize("k,shifts", [(39, "narrow"), (39, "all8"), (41, "narrow"), (50, "narrow"), (50, "all8")])
def test_long_kmers_as_points(oracle, k, shifts):
    """hs_join8w_kernel<2,6> (k = 39, 41: 192-byte rows; k = 41 has the record's position 40) and <2,8> (k = 50:
    256-byte rows), hs_refine8_kernel<2>"""
    case = jb.points_case(k, shifts)
    run = _Run(oracle, case, "narrow", dict(recognise_kmers=0))
    try:
        run.eng.set_verify_mode("join")

        def proof(prof):
            assert prof["join_i8_batches"] > 0 and prof["join_wide"] == 0
            assert prof["join_row_bytes"] == (192 if k <= 41 else 256)

        for refine8 in (1, 0):
            run.options(refine8=refine8)
            run.sweep(_points(run), ("join8w", refine8), proof)
        run.options(refine8=1)
        run.other_modes(_points(run), "long")
    finally:
        run.close()


@pytest.mark.parametrize("k", [15, 23])
def test_wide_rows(oracle, k):
    """hs_join8xw_kernel (k = 15: wide by itself) and hs_join8w_kernel<2,8,true> (k = 23 with wide_rows = 1), queries
    as points and as codes"""
    opts = dict(recognise_kmers=0, join_f6=0)
    if k == 23:
        opts["wide_rows"] = 1

    def proof(prof):
        assert prof["join_i8_batches"] > 0 and prof["join_wide"] > 0
        assert prof["join_row_bytes"] == (192 if k == 15 else 256)

    run = _Run(oracle, jb.points_case(k, "all8"), "wide", opts)
    try:
        run.eng.set_verify_mode("join")
        run.sweep(_points(run), "wide points", proof)
        run.other_modes(_points(run), "wide points")
    finally:
        run.close()
    run = _Run(oracle, jb.codes_case(k), "wide", opts)
    try:
        run.eng.set_verify_mode("join")
        run.sweep(_codes(run), "wide codes", proof)
        run.other_modes(_codes(run), "wide codes")
    finally:
        run.close()


def test_k15_on_4_column_rows(oracle):
    """wide_rows = 3: the 4-column rows for short k-mers too (the index is rebuilt for them)"""
    case = jb.points_case(15, "narrow")
    run = _Run(oracle, case, "narrow", dict(recognise_kmers=0, wide_rows=3))
    try:
        run.eng.set_verify_mode("join")

        def proof(prof):
            assert prof["join_i8_batches"] > 0 and prof["join_wide"] == 0 and prof["join_row_bytes"] == 128

        run.sweep(_points(run), "k15 narrow", proof)
        run.other_modes(_points(run), "k15 narrow")
        # and the same DB on the wide rows a default handle takes: set back, rebuilt
        run.options(wide_rows=0)
        run.eng.index_build(case["db_codes"])
        run.form = "wide"

        def wide(prof):
            assert prof["join_i8_batches"] > 0 and prof["join_wide"] > 0 and prof["join_row_bytes"] == 192

        run.sweep(_points(run), "k15 back on wide rows", wide)
    finally:
        run.close()


def test_saturated_queries(oracle):
    """the penalty term of hs_qprep8_kernel carries the pair: coordinates pushed past +-127/s where the member holds
    the pin residue"""
    case = jb.points_case(25, "narrow", True)
    run = _Run(oracle, case, "narrow", dict(recognise_kmers=0, wide_rows=2))
    try:
        run.eng.set_verify_mode("join")

        def proof(prof):      # (an unsafe batch leaves the int8 join: the penalty was charged, not avoided)
            assert prof["join_i8_batches"] > 0 and prof["join_wide"] == 0

        for refine8 in (1, 0):
            for resident in (1, 0):
                run.options(refine8=refine8, join_resident=resident)
                run.sweep(_points(run), ("saturated", refine8, resident), proof)
        run.options(refine8=1, join_resident=0)
        run.other_modes(_points(run), "saturated")
    finally:
        run.close()


@pytest.mark.parametrize("k", [25, 39, 50])
def test_kmer_queries_on_the_int8_join(oracle, k):
    """hs_qprep8_codes_kernel and hs_refine_codes_kernel in front of the int8 kernels (join_f6 = 0): queries given as
    codes, and centres recognised as k-mers"""
    case = jb.codes_case(k)
    run = _Run(oracle, case, "narrow", dict(join_f6=0, wide_rows=2))
    try:
        run.eng.set_verify_mode("join")

        def proof(prof):
            assert prof["join_i8_batches"] > 0 and prof["join_f6_batches"] == 0 and prof["join_wide"] == 0

        def recognised(prof):
            proof(prof)
            assert prof["queries_recognised"] == jb.N_ATT

        run.sweep(_codes(run), "codes", proof)
        run.sweep(_points(run), "recognised", recognised)
        run.options(join_resident=1)
        run.sweep(_codes(run), "codes, streaming kernel only", proof)
        run.options(join_resident=0)
        run.other_modes(_codes(run), "codes")
    finally:
        run.close()


@pytest.mark.parametrize("k", [25, 21])
def test_kmer_queries_on_the_fp6_join(oracle, k):
    """both FP6 forms.  Its bound is per residue pair and this table does not make it tight by design: the smallest
    host-side F over the attained pairs is printed, not asserted"""
    case = jb.codes_case(k)
    run = _Run(oracle, case, "f6", dict(join_f6=1, wide_rows=2))
    try:
        run.eng.set_verify_mode("join")
        for r in case["radii"]:
            F = jb.f6_figure(case["table"], r["members"], r["codes"], r["R"])
            print("FP6 k = %d R = %.4f: F = %d .. %d (units of 2^-6) over the attained pairs" % (
                k, r["R"], F.min(), F.max()))

        def proof(prof):
            assert prof["join_f6_batches"] > 0

        for form in (0, 1):
            # join_resident = 1: every segment through the FP6 streaming kernel, none through hs_join8r_kernel
            run.options(join_f6_form=form, join_resident=1)
            run.sweep(_codes(run), ("fp6", form), proof)
        run.options(join_resident=0)
        run.sweep(_codes(run), ("fp6", "default classes"), proof)
        run.other_modes(_codes(run), "fp6")
    finally:
        run.close()


@pytest.mark.parametrize("k", [25, 15])
def test_self_join(oracle, k):
    """the self-join's rows: the attained pairs are edges at the radius (both directions) and absent one double below,
    and all edges equal the oracle's bucket pairs"""
    case = jb.codes_case(k)
    fields = ("i", "j", "table", "dist")
    for g in (1, 2):
        r = case["radii"][g]
        # the members of this radius, their queries and a part of the bucket mates: a DB of its own
        rest = np.setdiff1d(np.arange(len(case["db_codes"])), np.concatenate([r["pair_id"], r["self_id"]]))[:800]
        codes = np.ascontiguousarray(np.concatenate([r["members"], r["codes"], case["db_codes"][rest]]))
        pts = jb.embed(case["table"], codes)
        n = len(r["members"])
        R_on, R_off = r["R"], math.nextafter(r["R"], 0.0)
        pairs = orr.bucket_pairs(oracle, case["a"], case["b"], case["W"], pts, R_on)
        att = {(i, n + i) for i in range(n)} | {(n + i, i) for i in range(n)}
        want_on = orr.edges_at(pairs, R_on, False)
        shared = att & set(zip(want_on["i"].tolist(), want_on["j"].tolist()))
        assert len(shared) >= 400                         # (both directions of >= 200 pairs share a bucket)
        eng = Engine(k, case["K"], case["L"], case["W"], case["a"], case["b"], coords=case["table"],
                     options=dict(wide_rows=2) if k > 20 else None)
        try:
            eng.index_build(codes)
            # (k = 25 from codes would take the FP6 rows by default: the int8 rows first, those second); then verify
            # modes auto and stream -- under stream the self-join runs from the embedded centres -- for equality only
            runs = [("join", 1, 0), ("join", 0, 0)] + ([("join", 1, 1)] if k > 20 else [])
            runs += [(mode, sc, 1) for mode in ("auto", "stream") for sc in (1, 0)]
            for mode, self_codes, join_f6 in runs:
                eng.set_verify_mode(mode)
                eng.set_option("self_codes", self_codes)
                eng.set_option("join_f6", join_f6)
                for R in (R_on, R_off):
                    for sq in (False, True):
                        want = orr.edges_at(pairs, R, sq)
                        got = eng.self_join(R, sqrt_test=sq)
                        prof = eng.profile()
                        for f in fields:
                            assert np.array_equal(got[f], want[f]), (k, g, mode, self_codes, join_f6, R, sq, f,
                                                                     len(got[f]), len(want[f]))
                        assert np.array_equal(got["dist"].view(np.uint64), want["dist"].view(np.uint64))
                        if mode == "join":
                            assert prof["join_i8_batches"] > 0 and (prof["join_f6_batches"] > 0) == bool(join_f6)
                        edges = set(zip(got["i"].tolist(), got["j"].tolist()))
                        if R == R_on:
                            assert shared <= edges
                        elif not sq:
                            assert not (att & edges)
        finally:
            eng.close()


def test_fp16_join(oracle):
    """hs_qprep_kernel and hs_join_kernel (verify mode join16) on a table whose every entry rounds down in fp16 by the
    largest relative error (test_join_bound_cpu.py: the model's G of these pairs is -1.6 .. -3.8, and positive with
    e_c halved); here the device returns the oracle's hits on them, and the counters show the fp16 form ran"""
    case = jb.fp16_case()
    run = _Run(oracle, case, "fp16", dict(recognise_kmers=0))
    try:
        run.eng.set_verify_mode("join16")

        def proof(prof):
            assert prof["join_batches"] > 0 and prof["join_i8_batches"] == 0

        run.sweep(_points(run), "fp16", proof)
        for mode in ("auto", "stream", "join"):
            run.eng.set_verify_mode(mode)
            run.sweep(_points(run), ("fp16 table", mode))
            run.sweep(_codes(run), ("fp16 table, codes", mode))
    finally:
        run.close()
