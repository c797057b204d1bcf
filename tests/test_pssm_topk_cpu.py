"""hs_pssm_topk without a GPU: the host rule (capi.pssm_topk_hits) against the numpy contract of tests/pssm_topk_ref.py,
the key transform of hsearch_amd/csrc/hs_pssm_topk.h, the argument that makes the sampled threshold exact (checked as
a superset), the survivor count the host tables predict at the sampled thresholds, and the header under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hsearch_amd import HsError, capi

import pssm_ref
import pssm_topk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ID = 0xffffffff


def _tuples(rng, nm, n_ids, nt):
    """nt random (m, id) pairs -- repeats included -- with a small integer score per (m, id): heavy ties, negative
    scores and +0.0."""
    table = rng.integers(-3, 4, size=(nm, n_ids)).astype(np.float64)
    m = rng.integers(0, nm, size=nt).astype(np.uint32)
    i = rng.integers(0, n_ids, size=nt).astype(np.uint32)
    return m, i, table[m, i], table


def _want(m, i, table, nm, topk):
    """The reference rows of the distinct (m, id) among the tuples."""
    sc = np.full(table.shape, -np.inf)
    sc[m, i] = table[m, i]
    floor = np.full(nm, -1e300)   # -inf marks an absent id: below every floor
    return ref.rows_from_scores(sc, topk, floor)


@pytest.mark.parametrize("topk", [1, 3, 10, 64])
def test_hits_rule_equals_reference(topk):
    rng = np.random.default_rng(40 + topk)
    for nm, n_ids, nt in ((1, 5, 40), (7, 100, 900), (4, 300, 200), (3, 70, 0)):
        m, i, s, table = _tuples(rng, nm, n_ids, nt)
        got = capi.pssm_topk_hits(m, i, s, nm, topk)
        ref.same_rows(got, _want(m, i, table, nm, topk), (nm, n_ids, nt, topk))
        assert got["count"].max(initial=0) <= topk
        # any order of the tuples gives the same rows
        p = rng.permutation(nt)
        ref.same_rows(capi.pssm_topk_hits(m[p], i[p], s[p], nm, topk), got, "permuted")
    assert (table == 0).any() and (table < 0).any()


def test_padding_fed_back_in_and_duplicates():
    rng = np.random.default_rng(7)
    nm, topk = 5, 8
    m, i, s, table = _tuples(rng, nm, 40, 300)
    rows = capi.pssm_topk_hits(m, i, s, nm, topk)
    # rows of two halves of the list, padding included, merged: the rows of the whole list
    half = len(m) // 2
    a = capi.pssm_topk_hits(m[:half], i[:half], s[:half], nm, topk)
    b = capi.pssm_topk_hits(m[half:], i[half:], s[half:], nm, topk)
    mm = np.repeat(np.arange(nm, dtype=np.uint32), topk)
    merged = capi.pssm_topk_hits(np.concatenate([mm, mm]), np.concatenate([a["id"].ravel(), b["id"].ravel()]),
                                 np.concatenate([a["score"].ravel(), b["score"].ravel()]), nm, topk)
    ref.same_rows(merged, rows, "merge of halves")
    only_pad = capi.pssm_topk_hits(mm, np.full(nm * topk, NO_ID, np.uint32), np.full(nm * topk, -np.inf), nm, topk)
    assert np.all(only_pad["id"] == NO_ID) and np.all(np.isneginf(only_pad["score"])) and np.all(only_pad["count"] == 0)
    # a repeated (m, id) counts once
    d = capi.pssm_topk_hits([0, 0, 0], [5, 5, 6], [1.5, 1.5, 1.5], 1, 4)
    assert d["id"][0].tolist() == [5, 6, NO_ID, NO_ID] and d["count"][0] == 2
    # -0.0 is read as +0.0 and ties with it
    z = capi.pssm_topk_hits([0, 0], [9, 3], [0.0, -0.0], 1, 2)
    assert z["id"][0].tolist() == [3, 9] and not np.signbit(z["score"]).any()


def test_refused_inputs_write_nothing():
    lib = capi.load()
    m = np.array([0, 0, 1], np.uint32)
    i = np.array([4, 4, 2], np.uint32)
    tid, ts, tc = np.full(4, 9, np.uint32), np.full(4, 9.0), np.full(2, 9, np.uint32)

    def call(mm, ii, ss, nt, nm, topk, out=(tid, ts, tc)):
        o = [capi._vp(x) if x is not None else None for x in out]
        return lib.hs_pssm_topk_hits(capi._vp(mm), capi._vp(ii), capi._vp(np.asarray(ss, np.float64)), nt, nm, topk, *o)

    bad = capi.HS_ERR_INVALID
    assert call(m, i, [1.0, 2.0, 0.5], 3, 2, 2) == bad            # two scores for (0, 4)
    assert call(m, i, [1.0, 1.0, np.nan], 3, 2, 2) == bad         # a NaN
    assert call(m, i, [1.0, 1.0, 0.5], 3, 1, 2) == bad            # m >= nm
    assert call(m, i, [1.0, 1.0, 0.5], 3, 2, 0) == bad            # topk
    assert call(m, i, [1.0, 1.0, 0.5], 3, 2, 65) == bad
    assert call(m, i, [1.0, 1.0, 0.5], 3, 2, 2, out=(None, ts, tc)) == bad
    assert np.all(tid == 9) and np.all(ts == 9.0) and np.all(tc == 9)
    assert call(m, i, [1.0, 1.0, 0.5], 3, 2, 2) == capi.HS_OK
    assert tid.tolist() == [4, NO_ID, 2, NO_ID] and tc.tolist() == [1, 1]
    with pytest.raises(HsError):
        capi.pssm_topk_hits([0], [1], [np.nan], 1, 1)
    with pytest.raises(HsError):
        capi.pssm_topk_hits([0], [1], [1.0], 1, 65)


def _key_functions():
    """The transform of hs_pssm_topk.h, read from the header's own expressions (a check that the numpy below is it)."""
    text = open(os.path.join(ROOT, "hsearch_amd", "csrc", "hs_pssm_topk.h")).read()
    assert re.search(r"bits \^ \(\(bits >> 63\) \? 0xffffffffffffffffull : 0x8000000000000000ull\)", text)
    assert re.search(r"u \^ \(\(u >> 63\) \? 0x8000000000000000ull : 0xffffffffffffffffull\)", text)
    ones, top = np.uint64(0xffffffffffffffff), np.uint64(1 << 63)
    key = lambda b: b ^ np.where(b >> np.uint64(63), ones, top)
    back = lambda u: u ^ np.where(u >> np.uint64(63), top, ones)
    return key, back


def test_key_transform_round_trips_and_orders():
    key, back = _key_functions()
    rng = np.random.default_rng(3)
    x = rng.integers(0, 1 << 64, size=12000, dtype=np.uint64).view(np.float64)
    x = x[np.isfinite(x)][:9000]
    sub = rng.integers(1, 1 << 52, size=500, dtype=np.uint64)
    sub = np.concatenate([sub, sub | np.uint64(1 << 63)]).view(np.float64)     # subnormals of both signs
    x = np.concatenate([x, sub, [0.0, 1.0, -1.0, 5e-324, -5e-324, np.finfo(float).max, -np.finfo(float).max]])
    x = x[~((x == 0) & np.signbit(x))]                                         # no score is -0.0
    assert len(x) >= 10000 and (np.abs(sub) < 2.3e-308).all()
    b = x.view(np.uint64)
    u = key(b)
    assert np.array_equal(back(u), b)
    assert np.array_equal(x[np.argsort(u, kind="stable")], np.sort(x))
    d = ~u                                                                     # the descending key
    assert np.array_equal(x[np.argsort(d, kind="stable")], np.sort(x)[::-1])
    assert not (d == np.uint64(0xffffffffffffffff)).any()                      # the padding key is no score's
    # the library's rule orders the same doubles the same way
    got = capi.pssm_topk_hits(np.zeros(64, np.uint32), np.arange(64, dtype=np.uint32), x[:64], 1, 64)
    assert np.array_equal(got["score"][0], np.sort(x[:64])[::-1])


_SUP = {}


def _superset_case():
    """50 random log-odds profiles over 20 000 random 25-mers, and their scores (computed once)."""
    if not _SUP:
        rng = np.random.default_rng(2024)
        n, k, A, nm = 20000, 25, 20, 50
        codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
        counts = np.stack([np.stack([rng.multinomial(30, rng.dirichlet(np.full(A, 0.3))) for _ in range(k)])
                           for _ in range(nm)])
        S = capi.pssm_log_odds(counts, background=np.full(A, 1.0 / A), pseudo=1.0)
        _SUP.update(codes=codes, S=S, sc=pssm_ref.scores(S, codes))
    return _SUP


@pytest.mark.parametrize("topk", [1, 10, 64])
def test_sampled_threshold_keeps_the_row(topk):
    """The argument, checked: the k-mers with score >= t_used are a superset of the reference row, whatever the sample."""
    case = _superset_case()
    sc = case["sc"]
    n = sc.shape[1]
    want = ref.rows_from_scores(sc, topk)
    for sample in (1, 64, 4096, n):
        tu = ref.t_used_from_scores(sc, topk, sample)
        for m in range(sc.shape[0]):
            kept = np.nonzero(sc[m] >= tu[m])[0]
            assert set(want["id"][m].tolist()) <= set(kept.tolist()), (sample, m)
            assert len(kept) >= topk
        if sample >= topk:
            assert np.all(tu > ref.NO_FLOOR)
        else:
            assert np.all(tu == ref.NO_FLOOR)
    # a floor never lowers the threshold, and a row under a floor may be short
    floor = np.sort(sc, axis=1)[:, -3] + 0.0
    tu = ref.t_used_from_scores(sc, topk, 4096, floor)
    assert np.array_equal(tu, np.maximum(floor, ref.t_used_from_scores(sc, topk, 4096)))
    short = ref.rows_from_scores(sc, topk, floor)
    assert np.all(short["count"] == min(topk, 3))
    for m in range(sc.shape[0]):
        assert set(short["id"][m, :short["count"][m]].tolist()) <= set(np.nonzero(sc[m] >= tu[m])[0].tolist())


def test_survivors_predicted_at_the_sampled_thresholds():
    """sample = 4096, topk = 10: the filter tables at t_used pass far fewer than a quarter of the pairs (about
    topk * n / n_s = 49 hits per profile are expected, times the tables' overshoot)."""
    case = _superset_case()
    sc = case["sc"]
    nm, n = sc.shape
    tu = ref.t_used_from_scores(sc, 10, 4096)
    T = capi.pssm_tables(case["S"], tu)
    F = pssm_ref.filter_values(T["code"], case["codes"])
    surv = int(((F >= T["tau"][:, None]) & (T["dead"] == 0)[:, None]).sum())
    hits = int((sc >= tu[:, None]).sum())
    assert T["dead"].sum() == 0
    assert nm * 10 <= hits <= surv < nm * n // 4, (hits, surv)
    assert hits < 10 * nm * 49      # the sample really stands for the index: within 10 x of the expectation


def test_exports_and_option_name():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in ("hs_pssm_topk", "hs_pssm_topk_dev", "hs_pssm_topk_hits"):
        assert re.search(r"HS_API hs_status %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name)
    assert capi.Engine.OPTIONS["pssm_topk_sample"] == 24 and "HS_OPT_PSSM_TOPK_SAMPLE = 24" in header
    fields = [f for f, _ in capi._Profile._fields_]
    assert fields[-2:] == ["pssm_topk_sample", "pssm_topk_raised"]
    struct = header[header.index("typedef struct hs_profile"):header.index("} hs_profile;")]
    declared = re.findall(r"^\s*(?:double|uint64_t|uint32_t)\s+(\w+);", struct, flags=re.M)
    assert declared == fields


def test_header_under_asan_and_ubsan(tmp_path):
    """hs_pssm_topk.h with a stand-alone main (tests/pssm_topk_san.cpp), compiled and run under AddressSanitizer +
    UndefinedBehaviorSanitizer (the runtimes linked statically); nothing is loaded into python."""
    exe = tmp_path / "pssm_topk_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "pssm_topk_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pssm_topk_san ok" in res.stdout
