"""hs_proj.hip held to its error bound: (point, function) pairs that ATTAIN the bound E of the MFMA pass, with the
reference's t one ulp on the far side of a bucket boundary (proj_ref.sharp; premises proved in test_proj_bound_cpu.py:
the fast pass alone returns the wrong floor at every such pair, |t_ref - T~| / E >= 0.999799).

Per case: the bucket integers equal the oracle's at all n F pairs, and the number of values the pass hands to the exact
kernel is the one the documented rule predicts -- the attained pairs inside it (sharp), the same pairs moved to 1.25 E
outside it (clear).  Together that pins the device's E between 0.99 and 1.25 of the rule pair by pair, on both arms of
the certainty test, for every MFMA step count, both operand sources, a ragged function tile and K = 32.  The same
inputs then go through the per-table path of the index build and through the query batch."""
import numpy as np
import pytest

import proj_ref
from hsearch_amd import Engine
from proj_ref import BUILD_CASES, CASES, case_id

pytestmark = pytest.mark.gpu


def _engine(c):
    eng = Engine(c["k"], c["K"], c["L"], c["W"], c["a"], c["b"], coords=c["table"])
    eng.set_hash_mode("mfma")
    return eng


def _hash(eng, c):
    return eng.hash_codes(c["codes"]) if c["path"] == "codes" else eng.hash_points(c["pts"])


def _first_wrong(c, got, want):
    """the failing pair with the model's figures for it"""
    p, l, kk = np.argwhere(got != want)[0]
    f = l * c["K"] + kk
    m = proj_ref.model(c["pts"], c["a"], c["b"], c["W"], c["table"], c["codes"] if c["path"] == "codes" else None)
    a2, bf = c["a"].reshape(c["F"], -1), c["b"].reshape(-1)
    t_ref = proj_ref.ref_t(proj_ref.ref_dot(c["pts"][p], a2[f]), bf[f], c["W"])
    return "pair (%d, %d): got %d, oracle %d; model T~ = %r, E = %r, t_ref = %r" % (
        p, f, got[p, l, kk], want[p, l, kk], m["T"][p, f], m["E"][p, f], float(t_ref))


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("kind", ["sharp", "clear"])
def test_attained_pairs(oracle, kind, case):
    c = getattr(proj_ref, kind)(*case)
    n, F = c["n"], c["F"]
    want = oracle.hash_all(c["a"], c["b"], c["W"], c["pts"])
    lo, hi = proj_ref.counts(c)
    eng = _engine(c)
    got = _hash(eng, c)
    prof = eng.profile()
    eng.close()
    print("%s %s: flagged %d of %d, predicted [%d, %d]" % (case_id(case), kind, prof["hash_flagged"], n * F, lo, hi))
    assert np.array_equal(got, want), _first_wrong(c, got, want)
    assert prof["hash_values"] == n * F
    assert lo <= prof["hash_flagged"] <= hi
    assert (lo >= n) if kind == "sharp" else (hi < n)     # the attained pairs: inside lo, outside hi


@pytest.mark.parametrize("case", BUILD_CASES, ids=case_id)
def test_attained_pairs_through_build_and_query(oracle, tmp_path, case):
    """The per-table path (table >= 0, out_stride = K: every build) and the batch path (every query) on the k-mers of
    the codes-path cases.  As query POINTS the k-mers' coordinates quantise to the same integers (every point holds an
    entry above 16320, so its own exponent is the table's), hence attain the bound on the points path as well."""
    c = proj_ref.sharp(*case)
    n, F = c["n"], c["F"]
    lo, hi = proj_ref.counts(c)
    assert np.array_equal(proj_ref.model(c["pts"], c["a"], c["b"], c["W"])["X"],
                          proj_ref.model(None, c["a"], c["b"], c["W"], c["table"], c["codes"])["X"])
    ix = oracle.Index(c["a"], c["b"], c["W"], c["pts"])
    sizes = ix.table_sizes()
    R = 1.5 * np.sqrt(8 * c["k"])                         # well under the typical distance between two of the k-mers
    want = ix.query(c["pts"], R)
    ix.close()
    res = {}
    for mode in ("mfma", "exact"):
        eng = Engine(c["k"], c["K"], c["L"], c["W"], c["a"], c["b"], coords=c["table"])
        eng.set_hash_mode(mode)
        info = eng.index_build(c["codes"])
        pb = eng.profile()
        path = tmp_path / (mode + ".idx")
        eng.index_save(path)
        qc = eng.query_codes(c["codes"], R)
        pqc = eng.profile()
        qp = eng.query(c["pts"], R)
        pqp = eng.profile()
        eng.close()
        res[mode] = (path.read_bytes(), qc, qp)
        assert info["n_buckets"] == sizes
        if mode == "mfma":
            print("%s: build flagged %d, query_codes %d, query %d; attained %d, predicted %d" % (
                case_id(case), pb["hash_flagged"], pqc["hash_flagged"], pqp["hash_flagged"], n, lo))
            assert pb["hash_values"] == n * F and pqc["hash_values"] == n * F and pqp["hash_values"] == n * F
            # a build hashes every table: every attained pair belongs to one of them
            # (and the rule counts a pair alike on every path: the same numbers as hash_codes gives)
            assert n <= lo <= pb["hash_flagged"] <= hi
            assert lo <= pqc["hash_flagged"] <= hi and lo <= pqp["hash_flagged"] <= hi
        else:
            assert pb["hash_values"] == 0 and pqc["hash_values"] == 0 and pqp["hash_values"] == 0
    assert res["mfma"][0] == res["exact"][0]              # the saved index, byte for byte
    for i in (1, 2):
        for fld in ("q", "id", "table", "dist", "cand"):
            assert np.array_equal(res["mfma"][i][fld], res["exact"][i][fld]), fld
        for fld in ("q", "id", "table", "dist", "cand"):
            assert np.array_equal(res["mfma"][i][fld], want[fld]), fld
    # every k-mer finds itself in every table: its query buckets are its build buckets
    assert np.all(want["cand"] >= 1) and len(want["q"]) >= n
