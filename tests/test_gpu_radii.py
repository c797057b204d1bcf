"""Per-query radii on the GPU (hs_query_radii / hs_query_radii_dev / hs_bruteforce_radii): the output is the
concatenation over the queries of what the scalar call returns for each query at its own radius -- against the CPU
oracle, against the scalar GPU call, with multi-probe and a bucket partition, brute force, errors and edges."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import multiprobe_ref as mp
from tests import radii_ref as rr
from tests.test_gpu_multiprobe import _case

pytestmark = pytest.mark.gpu

_FIELDS = ("q", "id", "table", "dist", "cand")


def _assert_same(got, want, what="", fields=_FIELDS):
    for f in fields:
        assert np.array_equal(got[f], want[f]), (what, f)


def _engine(k, a, b, W, codes):
    eng = Engine(k, a.shape[1], a.shape[0], W, a, b)
    eng.index_build(codes)
    return eng


@pytest.mark.parametrize("k", [15, 25, 39])
def test_hits_match_oracle_across_paths(oracle, k):
    a, b, W, codes, qcodes, centers = _case(k)
    radii = rr.draw_radii(k, len(centers))
    ix = oracle.Index(a, b, W, oracle.embed_codes(codes))
    want, hits = rr.stitch(ix.query, centers, radii)
    want_c, hits_c = rr.stitch(ix.query, synth.embed(qcodes), radii)
    for r in set(rr.RADIUS_SETS[k]):
        if r > 0:
            assert hits[r] > 0 and hits_c[r] > 0, r
    eng = _engine(k, a, b, W, codes)
    runs = [("verify", m, {}) for m in ("auto", "stream", "join", "join16")]
    runs += [("hash", m, {}) for m in ("auto", "exact", "mfma")]
    runs += [("opt", None, dict(seg_mode=1)), ("opt", None, dict(seg_mode=2)),
             ("opt", None, dict(join_resident=1)), ("opt", None, dict(join_resident=2)),
             ("opt", None, dict(wide_rows=1)), ("opt", None, dict(query_batch=37))]
    for what, mode, opts in runs:
        if what == "verify":
            eng.set_verify_mode(mode)
        elif what == "hash":
            eng.set_hash_mode(mode)
        for name, value in opts.items():
            eng.set_option(name, value)
        _assert_same(eng.query_radii(centers, radii), want, (what, mode, opts))
        _assert_same(eng.query_radii(qcodes, radii, codes=True), want_c, (what, mode, opts, "codes"))
        assert eng.profile()["candidates"] == int(want_c["cand"].sum())
        # recognised k-mer centres give the bits of the codes
        _assert_same(eng.query_radii(synth.embed(qcodes), radii), want_c, (what, mode, opts, "k-mer centres"))
        for name in opts:
            eng.set_option(name, {"seg_mode": 0, "join_resident": 0, "wide_rows": 0, "query_batch": 0}[name])
        eng.set_verify_mode("auto")
        eng.set_hash_mode("auto")
    eng.close()
    ix.close()


@pytest.mark.parametrize("k", [15, 25, 39])
def test_contract_against_scalar_calls(k):
    a, b, W, codes, qcodes, centers = _case(k)
    nq = 40
    radii = rr.draw_radii(k, nq, seed=5)
    eng = _engine(k, a, b, W, codes)
    for queries, codes_in in ((centers[:nq], False), (qcodes[:nq], True)):
        scalar = eng.query_codes if codes_in else eng.query
        parts = [scalar(queries[q:q + 1], float(radii[q])) for q in range(nq)]
        want = {f: np.concatenate([p[f] for p in parts]) for f in _FIELDS}
        want["q"] = np.concatenate([np.full(len(p["q"]), q, dtype=np.uint32) for q, p in enumerate(parts)])
        assert len(want["q"]) > 0
        _assert_same(eng.query_radii(queries, radii, codes=codes_in), want, ("one by one", codes_in))
    # uniform radii: the scalar call, bit for bit
    for R in sorted(set(rr.RADIUS_SETS[k])):
        for queries, codes_in in ((centers, False), (qcodes, True)):
            base = (eng.query_codes if codes_in else eng.query)(queries, R)
            cand = eng.profile()["candidates"]
            got = eng.query_radii(queries, np.full(len(queries), R), codes=codes_in)
            _assert_same(got, base, ("uniform", R, codes_in))
            assert eng.profile()["candidates"] == cand
    eng.close()


def test_dev_entry_point_matches_host():
    import torch
    k = 25
    a, b, W, codes, qcodes, centers = _case(k)
    radii = rr.draw_radii(k, len(centers))
    eng = _engine(k, a, b, W, codes)
    for queries, codes_in in ((centers, False), (qcodes, True)):
        want = eng.query_radii(queries, radii, codes=codes_in)
        n_want = len(want["q"])
        d_in = torch.from_numpy(queries).cuda()
        d_r = torch.from_numpy(radii).cuda()
        cap = n_want
        d_q, d_id, d_t = (torch.zeros(max(cap, 1), dtype=torch.int32, device="cuda") for _ in range(3))
        d_d = torch.zeros(max(cap, 1), dtype=torch.float64, device="cuda")
        d_c = torch.zeros((len(queries), eng.L), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(capi.HsError) as e:  # the two-call pattern
            eng.query_radii_dev(d_in.data_ptr(), len(queries), d_r.data_ptr(), d_q.data_ptr(), d_id.data_ptr(),
                                d_t.data_ptr(), d_d.data_ptr(), n_want - 1, codes=codes_in)
        assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == n_want
        n = eng.query_radii_dev(d_in.data_ptr(), len(queries), d_r.data_ptr(), d_q.data_ptr(), d_id.data_ptr(),
                                d_t.data_ptr(), d_d.data_ptr(), cap, d_cand=d_c.data_ptr(), codes=codes_in)
        assert n == n_want
        got = dict(q=d_q[:n].cpu().numpy().astype(np.uint32), id=d_id[:n].cpu().numpy().astype(np.uint32),
                   table=d_t[:n].cpu().numpy().astype(np.uint32), dist=d_d[:n].cpu().numpy(),
                   cand=d_c.cpu().numpy().astype(np.uint64))
        _assert_same(got, want, ("dev", codes_in))
    eng.close()


def test_with_multiprobe(oracle):
    k, T = 25, 6
    a, b, W, codes, qcodes, centers = _case(k)
    radii = rr.draw_radii(k, len(centers))
    db = oracle.embed_codes(codes)
    want, hits = rr.stitch(lambda pts, R: mp.search(oracle, a, b, W, db, pts, R, T), centers, radii)
    want_c, _ = rr.stitch(lambda pts, R: mp.search(oracle, a, b, W, db, pts, R, T), synth.embed(qcodes), radii)
    assert all(hits[r] > 0 for r in hits if r > 0)
    eng = _engine(k, a, b, W, codes)
    eng.set_multiprobe(T)
    for opts in ({}, dict(query_batch=37), dict(wide_rows=1)):
        for name, value in opts.items():
            eng.set_option(name, value)
        _assert_same(eng.query_radii(centers, radii), want, ("multi-probe", opts))
        _assert_same(eng.query_radii(qcodes, radii, codes=True), want_c, ("multi-probe codes", opts))
        for name in opts:
            eng.set_option(name, 0)
    eng.close()


@pytest.mark.parametrize("T", [0, 4])
def test_with_bucket_partition(T):
    import torch
    k = 25
    a, b, W, codes, _, centers = _case(k)
    radii = rr.draw_radii(k, len(centers))
    eng = _engine(k, a, b, W, codes)
    eng.set_multiprobe(T)
    full = eng.query_radii(centers, radii)
    assert len(full["q"]) > 0
    n_parts = 3
    lists = []
    for part in range(n_parts):
        eng.set_bucket_partition(part, n_parts)
        lists.append(eng.query_radii(centers, radii))
    eng.set_bucket_partition(0, 1)
    cat = {f: np.concatenate([x[f] for x in lists]) for f in ("q", "id", "table", "dist")}
    dev = {f: torch.from_numpy(cat[f].astype(np.int32) if f != "dist" else cat[f]).cuda() for f in cat}
    torch.cuda.synchronize()
    n = eng.merge_first_table_dev(dev["q"].data_ptr(), dev["id"].data_ptr(), dev["table"].data_ptr(),
                                  dev["dist"].data_ptr(), len(cat["q"]))
    for f in ("q", "id", "table", "dist"):
        got = dev[f][:n].cpu().numpy()
        assert np.array_equal(got.astype(full[f].dtype), full[f]), f
    eng.close()


@pytest.mark.parametrize("k", [15, 25, 39])
def test_bruteforce_radii(oracle, k):
    a, b, W, codes, qcodes, centers = _case(k, n=6000, nq=120)
    radii = rr.draw_radii(k, len(centers))
    db = oracle.embed_codes(codes)
    fields = ("q", "id", "dist")
    eng = _engine(k, a, b, W, codes)
    for pts in (centers, synth.embed(qcodes)):
        want, hits = rr.stitch(lambda p, R: oracle.bruteforce(db, p, R), pts, radii, fields=fields)
        assert all(hits[r] > 0 for r in hits if r > 0)
        got = eng.bruteforce_radii(pts, radii)
        _assert_same(got, want, "brute force", fields)
        lsh = eng.query_radii(pts, radii)
        assert len(lsh["q"]) > 0
        truth = dict(zip(zip(got["q"].tolist(), got["id"].tolist()), got["dist"].tolist()))
        for q, i, d in zip(lsh["q"].tolist(), lsh["id"].tolist(), lsh["dist"].tolist()):
            assert truth.get((q, i)) == d, (q, i)
    # a negative radius: what the scalar calls do with it (brute force: nothing; the search: its square)
    neg = -np.abs(radii)
    assert len(eng.bruteforce_radii(centers, neg)["q"]) == 0
    for R in sorted(set(neg.tolist())):
        assert len(eng.bruteforce(centers[neg == R], R)["q"]) == 0
    want, _ = rr.stitch(eng.query, centers, neg)
    _assert_same(eng.query_radii(centers, neg), want, "negative radii")
    eng.close()


def _raw_radii_call(eng, centers, qcodes, nq, radii, cap):
    """hs_query_radii with caller-filled outputs: (status, n_hits, the output arrays)."""
    out = dict(q=np.full(cap, 0xabababab, dtype=np.uint32), id=np.full(cap, 0xabababab, dtype=np.uint32),
               table=np.full(cap, 0xabababab, dtype=np.uint32), dist=np.full(cap, -7.0))
    n = C.c_uint64(99)
    st = eng._lib.hs_query_radii(eng._h, None if centers is None else capi._vp(centers),
                                 None if qcodes is None else capi._vp(qcodes), nq, capi._vp(radii),
                                 capi._vp(out["q"]), capi._vp(out["id"]), capi._vp(out["table"]), capi._vp(out["dist"]),
                                 cap, C.byref(n), None)
    return st, int(n.value), out


def test_errors_and_edges():
    import torch
    k, R = 25, 40.0
    a, b, W, codes, qcodes, centers = _case(k)
    nq = len(centers)
    radii = rr.draw_radii(k, nq)
    eng = _engine(k, a, b, W, codes)
    fresh = _engine(k, a, b, W, codes)
    base = fresh.query(centers, R)
    good = eng.query_radii(centers, radii)
    # NaN anywhere: an error, nothing written (host)
    bad = radii.copy()
    bad[nq - 3] = np.nan
    with pytest.raises(capi.HsError) as e:
        eng.query_radii(centers, bad)
    assert e.value.status == capi.HS_ERR_INVALID
    with pytest.raises(capi.HsError):
        eng.bruteforce_radii(centers, bad)
    st, n, out = _raw_radii_call(eng, centers, None, nq, bad, 4096)
    assert st == capi.HS_ERR_INVALID and n == 0
    assert (out["q"] == 0xabababab).all() and (out["id"] == 0xabababab).all() and (out["dist"] == -7.0).all()
    # ... and on the device
    d_in, d_r = torch.from_numpy(centers).cuda(), torch.from_numpy(bad).cuda()
    cap = len(good["q"]) + 16
    d_q, d_id, d_t = (torch.full((cap,), 77, dtype=torch.int32, device="cuda") for _ in range(3))
    d_d = torch.full((cap,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(capi.HsError) as e:
        eng.query_radii_dev(d_in.data_ptr(), nq, d_r.data_ptr(), d_q.data_ptr(), d_id.data_ptr(), d_t.data_ptr(),
                            d_d.data_ptr(), cap)
    assert e.value.status == capi.HS_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((d_q == 77).all()) and bool((d_id == 77).all()) and bool((d_t == 77).all()) and bool((d_d == -7.0).all())
    # both or neither of centres / codes
    for c_in, q_in in ((centers, qcodes), (None, None)):
        st, n, _ = _raw_radii_call(eng, c_in, q_in, nq, radii, 4096)
        assert st == capi.HS_ERR_INVALID and n == 0
    d_ok = torch.from_numpy(radii).cuda()
    torch.cuda.synchronize()
    for c_in, q_in in ((d_in.data_ptr(), d_in.data_ptr()), (None, None)):
        n = C.c_uint64(99)
        st = eng._lib.hs_query_radii_dev(eng._h, c_in, q_in, nq, d_ok.data_ptr(), d_q.data_ptr(), d_id.data_ptr(),
                                         d_t.data_ptr(), d_d.data_ptr(), cap, C.byref(n), None)
        assert st == capi.HS_ERR_INVALID and n.value == 0
    # no queries
    none = eng.query_radii(centers[:0], radii[:0])
    assert len(none["q"]) == 0 and none["cand"].shape == (0, eng.L)
    assert len(eng.bruteforce_radii(centers[:0], radii[:0])["q"]) == 0
    # capacity: the first call reports the size, the second fits exactly
    st, n, _ = _raw_radii_call(eng, centers, None, nq, radii, 1)
    assert st == capi.HS_ERR_CAPACITY and n == len(good["q"])
    st, n2, out = _raw_radii_call(eng, centers, None, nq, radii, n)
    assert st == capi.HS_OK and n2 == n
    for f in ("q", "id", "table", "dist"):
        assert np.array_equal(out[f], good[f]), f
    _assert_same(eng.query_radii(centers, radii, cap=1), good, "cap = 1")
    # nothing of a radii call stays behind in the handle: the scalar call equals a fresh handle's, profile included
    _assert_same(eng.query(centers, R), base, "scalar after radii")
    fresh.query(centers, R)
    prof_f = fresh.profile()
    eng.query(centers, R)
    prof_e = eng.profile()
    for f in ("candidates", "hits", "join_wide", "join_row_bytes"):
        assert prof_e[f] == prof_f[f], f
    # a radius too large for the join's rows (R^2 >= 30000) sends the call to the streaming filter; same hits
    big = radii.copy()
    big[::50] = 180.0
    want, _ = rr.stitch(fresh.query, centers, big)
    _assert_same(eng.query_radii(centers, big), want, "one huge radius")
    eng.close()
    fresh.close()
