"""hs_join6x_kernel: the bucket join for queries that are k-mers on FP6 (e2m3) MFMA, against the oracle.

The planted case is tests/test_gpu_join8x_issue.py's (`_case`: buckets of 129 / 128 / 127 / 1 / 700 members against
segments of 129 / 65 / 96 / 97 / 127 queries, a survivor on every member and query slot of an item, pairs exactly on
the radius and one double below), built at k = 25, 21 and 23.  Every result is compared with the oracle's, with
HS_OPT_JOIN_F6 at 1 and at 0; `join_f6_batches` says which kernel ran, so a silent fallback to the int8 kernel fails
the first arm.  The tile product itself -- lane map, accumulation at the format's extremes -- is the library's
hs_join6_selftest (int64 arithmetic on the device).  The CPU side of the bound: tests/test_join6_tables_cpu.py."""
import importlib.util
import os

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth

from tests import test_gpu_join8x_issue as planted

_CASES = {}


def _case(oracle, k):
    """planted._case at k-mer length k (its module works at one length at a time: set, build, restore)."""
    if k not in _CASES:
        keep = planted.K_MER
        try:
            planted.K_MER = k
            planted._CASE.clear()
            _CASES[k] = dict(planted._case(oracle))
        finally:
            planted.K_MER = keep
            planted._CASE.clear()
    return _CASES[k]


def _engine(c, k, f6, **opts):
    # join_resident=1: every segment through the query-streaming kernel (the kernel under test)
    opts = dict(dict(join_resident=1, join_f6=f6), **opts)
    eng = Engine(k, planted.KK, planted.L, planted.W, c["a"], c["b"], options=opts)
    eng.index_build(c["codes"])
    eng.set_verify_mode("join")
    return eng


def _selectivity_tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "f6_filter_selectivity.py")
    spec = importlib.util.spec_from_file_location("f6_filter_selectivity", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_tile_product_is_exact():
    n, bad = capi.join6_selftest(0, 0)
    assert n == 0, "hs_join6_selftest: %d accumulators differ; first (case, lane*4+reg, bits, want64) = %r" % (n, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [25, 21, 23])
def test_planted_case_equals_the_oracle(oracle, k):
    c = _case(oracle, k)
    for f6 in (1, 0):
        for opts in (dict(), dict(join_resident=2, join_xcd_run=2, join_chunk=3)):
            eng = _engine(c, k, f6, **opts)
            for R, want in ((c["R"], c["want"]), (c["R_off"], c["want_off"])):
                got = eng.query_codes(c["qcodes"], R)
                p = eng.profile()
                assert p["join_i8_batches"] > 0 and p["join_items"] > p["join_items_resident"], p
                assert (p["join_f6_batches"] > 0) == bool(f6), (k, f6, p)
                assert p["join_row_bytes"] == 128
                planted._assert_equal(got, want, (k, f6, opts, R))
            eng.close()


@pytest.mark.gpu
def test_entry_points(oracle):
    k = 25
    c = _case(oracle, k)
    pts, cpts = oracle.embed_codes(c["codes"]), oracle.embed_codes(c["qcodes"])
    nq = len(c["qcodes"])
    # per-query radii: even queries at the radius, odd ones a double below
    radii = np.where(np.arange(nq) % 2 == 0, c["R"], c["R_off"])
    parts = [{f: w[f][(w["q"] % 2) == par] for f in ("q", "id", "table", "dist")}
             for par, w in ((0, c["want"]), (1, c["want_off"]))]
    order = np.argsort(np.concatenate([p["q"] for p in parts]), kind="stable")
    want_radii = {f: np.concatenate([p[f] for p in parts])[order] for f in ("q", "id", "table", "dist")}
    want_radii["cand"] = c["want"]["cand"]
    # the self-join: the oracle's search of the database for its own k-mers, without the pairs (i, i)
    ix = oracle.Index(c["a"], c["b"], planted.W, pts)
    me = ix.query(pts, c["R"])
    ix.close()
    other = me["q"] != me["id"]
    want_self = sorted(zip(me["q"][other].tolist(), me["id"][other].tolist(), me["dist"][other].tolist()))
    jit = cpts + np.random.default_rng(5).normal(0.0, 0.05, size=cpts.shape)
    ix = oracle.Index(c["a"], c["b"], planted.W, pts)
    want_jit = ix.query(jit, c["R"])
    ix.close()
    for f6 in (1, 0):
        eng = _engine(c, k, f6)
        ran = lambda: eng.profile()["join_f6_batches"] > 0      # noqa: E731
        planted._assert_equal(eng.query_codes(c["qcodes"], c["R"]), c["want"], (f6, "codes"))
        assert ran() == bool(f6)
        planted._assert_equal(eng.query(cpts, c["R"]), c["want"], (f6, "recognised centres"))
        assert eng.profile()["queries_recognised"] == nq and ran() == bool(f6)
        planted._assert_equal(eng.query_radii(c["qcodes"], radii, codes=True), want_radii, (f6, "radii"))
        assert ran() == bool(f6)
        sj = eng.self_join(c["R"])
        assert ran() == bool(f6)
        assert sorted(zip(sj["i"].tolist(), sj["j"].tolist(), sj["dist"].tolist())) == want_self, (f6, "self-join")
        # centres that are no k-mers have no residue-pair table: the int8 kernel, whatever the option says
        planted._assert_equal(eng.query(jit, c["R"]), want_jit, (f6, "jittered"))
        p = eng.profile()
        assert p["join_f6_batches"] == 0 and p["join_i8_batches"] > 0 and p["queries_recognised"] == 0, p
        eng.close()


@pytest.mark.gpu
def test_selectivity_cap(oracle):
    """The FP6 filter may pass more non-hits than the int8 one, not many more: at most twice the survivors on the
    planted case (the figures of tools/f6_filter_selectivity.py give about 1.02 x).  A cap, not a measurement."""
    k = 25
    c = _case(oracle, k)
    prov = {}
    for f6 in (1, 0):
        eng = _engine(c, k, f6)
        eng.query_codes(c["qcodes"], c["R"])
        prov[f6] = eng.profile()["provisional"]
        eng.close()
    print("provisional: FP6 %d, int8 %d" % (prov[1], prov[0]))
    assert prov[0] > 0 and prov[1] <= 2 * prov[0], prov


def test_selectivity_cap_on_the_oracle(oracle):
    """No GPU: the same cap from the bounds alone, over the in-bucket pairs of the planted case (table 0 and 1), with
    the thresholds the library hands out -- and no pair within the radius fails either bound."""
    k = 25
    c = _case(oracle, k)
    tool = _selectivity_tool()
    t = synth.coords()
    pts, cpts = oracle.embed_codes(c["codes"]), oracle.embed_codes(c["qcodes"])
    ints = oracle.hash_all(c["a"], c["b"], planted.W, np.concatenate([pts, cpts]))
    xi, ci = [], []
    for l in range(planted.L):
        b = planted._bucket_ids(ints, l)
        db_b, q_b = b[:len(pts)], b[len(pts):]
        order = np.argsort(db_b, kind="stable")
        lo, hi = np.searchsorted(db_b[order], q_b, "left"), np.searchsorted(db_b[order], q_b, "right")
        for q in range(len(cpts)):
            xi.append(order[lo[q]:hi[q]])
            ci.append(np.full(hi[q] - lo[q], q))
    xi, ci = np.concatenate(xi), np.concatenate(ci)
    x, q = c["codes"][xi], c["qcodes"][ci]
    r2 = c["R"] ** 2
    d2 = ((t[x] - t[q]) ** 2).sum(axis=(1, 2))
    f6 = tool.pass_f6(t, x, q, r2)
    i8 = tool.pass_int8(t, x, q, r2)
    hit = d2 <= r2
    assert hit.sum() >= 138 and f6[hit].all() and i8[hit].all()
    print("in-bucket pairs %d: hits %d, FP6 passes %d, int8 passes %d" % (len(d2), hit.sum(), f6.sum(), i8.sum()))
    assert f6.sum() <= 2 * i8.sum()
