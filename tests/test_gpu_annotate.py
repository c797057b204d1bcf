"""hs_annotate / hs_annotate_dev on the GPU: the nearest centre of every DB k-mer reached, reduced on the device,
against the numpy rule (tests/annotate_ref.py) applied to the CPU oracle's hit lists and to the same engine's own
query output -- across the filter and grouping paths, batches, radii, multi-probe and bucket partitions -- plus the
capacity protocol, the edges, the errors and the state the reduction keeps on the handle."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import annotate_ref as ar
from tests import radii_ref as rr
from tests.test_gpu_multiprobe import _case

pytestmark = pytest.mark.gpu

_R = {15: 30.0, 25: 40.0, 39: 50.0}
_RESET = {"seg_mode": 0, "query_batch": 0}


def _engine(k, a, b, W, codes):
    eng = Engine(k, a.shape[1], a.shape[0], W, a, b)
    eng.index_build(codes)
    return eng


@pytest.mark.parametrize("k", [15, 25, 39])
def test_annotation_matches_oracle_across_paths(oracle, k):
    R = _R[k]
    a, b, W, codes, qcodes, centers = _case(k)
    ix = oracle.Index(a, b, W, oracle.embed_codes(codes))
    hits, hits_c = ix.query(centers, R), ix.query(synth.embed(qcodes), R)
    ix.close()
    want, want_c = ar.annotate(hits), ar.annotate(hits_c)
    assert 0 < len(want["id"]) <= len(hits["id"]) and 0 < len(want_c["id"]) <= len(hits_c["id"])
    eng = _engine(k, a, b, W, codes)
    runs = [(m, {}) for m in ("auto", "stream", "join", "join16")]
    runs += [("auto", dict(seg_mode=1)), ("auto", dict(seg_mode=2)), ("auto", dict(query_batch=37))]
    for mode, opts in runs:
        eng.set_verify_mode(mode)
        for name, value in opts.items():
            eng.set_option(name, value)
        ar.assert_same(eng.annotate(centers, R), want, (mode, opts, "points"))
        assert eng.profile()["hits"] == len(hits["id"])
        ar.assert_same(eng.annotate(qcodes, R, codes=True), want_c, (mode, opts, "codes"))
        ar.assert_same(eng.annotate(synth.embed(qcodes), R), want_c, (mode, opts, "k-mer centres"))
        assert eng.profile()["queries_recognised"] == len(qcodes)
        for name in opts:
            eng.set_option(name, _RESET[name])
    eng.close()


@pytest.mark.parametrize("k", [15, 25, 39])
def test_duplicate_centres_reach_the_tie_levels(oracle, k):
    R = _R[k]
    a, b, W, codes, qcodes, centers = _case(k)
    # the same k-mer as two centres, far apart in the call: with query_batch = 37 in different batches
    dup = np.concatenate([qcodes, qcodes[:80][::-1]])
    ix = oracle.Index(a, b, W, oracle.embed_codes(codes))
    hits = ix.query(synth.embed(dup), R)
    ix.close()
    by_table, by_q = ar.tie_levels(hits)
    print("k = %d: ids decided by table %d, by q %d, of %d" % (k, by_table, by_q, len(set(hits["id"].tolist()))))
    assert by_q > 0, "no id of the oracle's list is decided by the centre number"
    want = ar.annotate(hits)
    eng = _engine(k, a, b, W, codes)
    for qb in (0, 37, 64):
        eng.set_option("query_batch", qb)
        ar.assert_same(eng.annotate(dup, R, codes=True), want, ("codes", qb))
        ar.assert_same(eng.annotate(synth.embed(dup), R), want, ("k-mer centres", qb))
    eng.set_option("query_batch", 0)
    eng.set_option("recognise_kmers", 0)
    ar.assert_same(eng.annotate(synth.embed(dup), R), want, "as points")
    eng.close()


@pytest.mark.parametrize("k", [15, 25, 39])
def test_annotation_is_the_rule_on_the_engines_own_hits(k):
    R = _R[k]
    a, b, W, codes, qcodes, centers = _case(k)
    dup = np.concatenate([qcodes, qcodes[:80][::-1]])
    radii = rr.draw_radii(k, len(centers))
    radii_d = rr.draw_radii(k, len(dup), seed=3)
    eng = _engine(k, a, b, W, codes)
    # per-query radii
    for qb in (0, 37):
        eng.set_option("query_batch", qb)
        ar.assert_same(eng.annotate(centers, radii=radii), ar.annotate(eng.query_radii(centers, radii)), ("radii", qb))
        ar.assert_same(eng.annotate(dup, radii=radii_d, codes=True),
                       ar.annotate(eng.query_radii(dup, radii_d, codes=True)), ("radii codes", qb))
    eng.set_option("query_batch", 0)
    # multi-probe: the merged list of every chunk is what is reduced
    for T in (1, 4):
        eng.set_multiprobe(T)
        for qb in (0, 37):
            eng.set_option("query_batch", qb)
            ar.assert_same(eng.annotate(centers, R), ar.annotate(eng.query(centers, R)), ("multiprobe", T, qb))
            ar.assert_same(eng.annotate(dup, R, codes=True), ar.annotate(eng.query_codes(dup, R)),
                           ("multiprobe codes", T, qb))
        eng.set_option("query_batch", 0)
        ar.assert_same(eng.annotate(centers, radii=radii), ar.annotate(eng.query_radii(centers, radii)),
                       ("multiprobe radii", T))
    eng.set_multiprobe(0)
    # bucket partition: every part's annotation is the rule on that part's hits, and merged they are the whole
    whole = eng.annotate(dup, R, codes=True)
    ar.assert_same(whole, ar.annotate(eng.query_codes(dup, R)), "unpartitioned")
    parts = []
    for part in range(3):
        eng.set_bucket_partition(part, 3)
        parts.append(eng.annotate(dup, R, codes=True))
        ar.assert_same(parts[-1], ar.annotate(eng.query_codes(dup, R)), ("part", part))
        assert len(parts[-1]["id"]) > 0
    eng.set_bucket_partition(0, 1)
    merged = ar.concat(parts)
    ar.assert_same(capi.merge_best(merged["id"], merged["q"], merged["table"], merged["dist"]), whole, "parts merged")
    eng.close()


def _dev_buffers(torch, cap, fill=0):
    ints = [torch.full((max(cap, 1),), fill, dtype=torch.int32, device="cuda") for _ in range(3)]
    return ints + [torch.full((max(cap, 1),), float(fill), dtype=torch.float64, device="cuda")]


def _dev_rows(bufs, n):
    d_id, d_q, d_t, d_d = bufs
    return dict(id=d_id[:n].cpu().numpy().astype(np.uint32), q=d_q[:n].cpu().numpy().astype(np.uint32),
                table=d_t[:n].cpu().numpy().astype(np.uint32), dist=d_d[:n].cpu().numpy())


def test_dev_form_and_two_call_capacity():
    import torch
    k = 25
    R = _R[k]
    a, b, W, codes, qcodes, centers = _case(k)
    radii = rr.draw_radii(k, len(centers))
    eng = _engine(k, a, b, W, codes)
    for queries, codes_in, rad in ((centers, False, None), (qcodes, True, None), (centers, False, radii),
                                   (qcodes, True, radii)):
        want = eng.annotate(queries, R=None if rad is not None else R, radii=rad, codes=codes_in)
        need = len(want["id"])
        assert need > 1
        d_in = torch.from_numpy(queries).cuda()
        d_r = torch.from_numpy(rad).cuda() if rad is not None else None
        r_ptr = d_r.data_ptr() if d_r is not None else None
        bufs = _dev_buffers(torch, need, fill=-7)
        ptrs = [t.data_ptr() for t in bufs]
        torch.cuda.synchronize()
        with pytest.raises(capi.HsError) as e:
            eng.annotate_dev(d_in.data_ptr(), len(queries), R, r_ptr, *ptrs, need - 1, codes=codes_in)
        assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == need
        assert all(bool((t == -7).all()) for t in bufs), "a call that reports the capacity writes no row"
        n = eng.annotate_dev(d_in.data_ptr(), len(queries), R, r_ptr, *ptrs, need, codes=codes_in)
        assert n == need
        ar.assert_same(_dev_rows(bufs, n), want, ("dev", codes_in, rad is not None))
    # the host form: the required size, then success; sized once at the index's n it always fits
    small = [np.empty(3, dtype=np.uint32) for _ in range(3)] + [np.empty(3)]
    n_out = C.c_uint64(0)
    st = eng._lib.hs_annotate(eng._h, capi._vp(centers), None, len(centers), R, None, *[capi._vp(x) for x in small], 3,
                              C.byref(n_out))
    assert st == capi.HS_ERR_CAPACITY and n_out.value == len(eng.annotate(centers, R)["id"])
    got = eng.annotate(centers, R, cap=len(codes))
    ar.assert_same(got, ar.annotate(eng.query(centers, R)), "cap = n")
    assert len(got["id"]) <= len(codes)
    eng.close()


def test_edges_and_errors():
    import torch
    k = 25
    R = _R[k]
    a, b, W, codes, qcodes, centers = _case(k)
    eng = _engine(k, a, b, W, codes)
    # no query
    got = eng.annotate(centers[:0], R)
    assert all(len(got[f]) == 0 for f in ar.FIELDS)
    got = eng.annotate(qcodes[:0], radii=np.empty(0), codes=True)
    assert all(len(got[f]) == 0 for f in ar.FIELDS)
    # a radius that yields no hit (the centres are jittered: none is a k-mer of the database)
    assert len(eng.query(centers, 0.0)["q"]) == 0
    got = eng.annotate(centers, 0.0)
    assert all(len(got[f]) == 0 for f in ar.FIELDS)
    got = eng.annotate(centers, radii=np.zeros(len(centers)))
    assert all(len(got[f]) == 0 for f in ar.FIELDS)
    # a NaN radius: HS_ERR_INVALID, the outputs untouched (host and device form)
    bad = rr.draw_radii(k, len(centers)).copy()
    bad[len(bad) // 2] = np.nan
    oid, oq, ot = (np.full(len(codes), 0xABCD, dtype=np.uint32) for _ in range(3))
    od = np.full(len(codes), -3.0)
    n_out = C.c_uint64(5)
    st = eng._lib.hs_annotate(eng._h, capi._vp(centers), None, len(centers), 0.0, capi._vp(bad), capi._vp(oid),
                              capi._vp(oq), capi._vp(ot), capi._vp(od), len(codes), C.byref(n_out))
    assert st == capi.HS_ERR_INVALID and n_out.value == 0
    assert (oid == 0xABCD).all() and (oq == 0xABCD).all() and (ot == 0xABCD).all() and (od == -3.0).all()
    bufs = _dev_buffers(torch, len(codes), fill=-7)
    d_in, d_r = torch.from_numpy(centers).cuda(), torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    with pytest.raises(capi.HsError) as e:
        eng.annotate_dev(d_in.data_ptr(), len(centers), 0.0, d_r.data_ptr(), *[t.data_ptr() for t in bufs], len(codes))
    assert e.value.status == capi.HS_ERR_INVALID
    assert all(bool((t == -7).all()) for t in bufs)
    with pytest.raises(capi.HsError) as e:
        eng.annotate(centers, float("nan"))
    assert e.value.status == capi.HS_ERR_INVALID
    # a query code outside the alphabet, in a late batch: an error, no row, and the next call is clean
    broken = qcodes.copy()
    broken[-3, 4] = 31
    eng.set_option("query_batch", 37)
    with pytest.raises(capi.HsError) as e:
        eng.annotate(broken, R, codes=True)
    assert e.value.status == capi.HS_ERR_INVALID
    eng.set_option("query_batch", 0)
    ar.assert_same(eng.annotate(centers, R), ar.annotate(eng.query(centers, R)), "after the failed call")
    # both and neither of centers / qcodes
    n_out = C.c_uint64(0)
    for c_ptr, q_ptr in ((capi._vp(centers), capi._vp(qcodes)), (None, None)):
        assert eng._lib.hs_annotate(eng._h, c_ptr, q_ptr, 4, R, None, None, None, None, None, 0,
                                    C.byref(n_out)) == capi.HS_ERR_INVALID
    eng.close()
    # an index that was never built
    eng = Engine(k, a.shape[1], a.shape[0], W, a, b)
    with pytest.raises(capi.HsError) as e:
        eng.annotate(centers, R)
    assert e.value.status == capi.HS_ERR_STATE
    eng.close()


def test_state_does_not_leak_between_calls():
    k = 15
    R = _R[k]
    a, b, W, codes, qcodes, centers = _case(k)
    eng = _engine(k, a, b, W, codes)
    fields = ("q", "id", "table", "dist", "cand")
    before = eng.query(centers, R)
    before_c = eng.query_codes(qcodes, R)
    first = eng.annotate(centers, R)
    # the scalar calls after an annotation return what they returned before
    after = eng.query(centers, R)
    after_c = eng.query_codes(qcodes, R)
    for f in fields:
        assert np.array_equal(before[f], after[f]) and np.array_equal(before_c[f], after_c[f]), f
    ar.assert_same(first, ar.annotate(before), "first")
    # other centres, fewer of them, a smaller radius: nothing of the first call's slots shows
    others, _ = synth.make_queries(codes, 120, jitter=0.25, seed=41)
    want = ar.annotate(eng.query(others, R - 8.0))
    assert 0 < len(want["id"]) < len(first["id"])
    ar.assert_same(eng.annotate(others, R - 8.0), want, "second")
    # a call whose rows were refused for capacity leaves nothing behind either
    with pytest.raises(capi.HsError):
        n_out = C.c_uint64(0)
        eng._check(eng._lib.hs_annotate(eng._h, capi._vp(centers), None, len(centers), R, None, None, None, None, None,
                                        0, C.byref(n_out)))
    ar.assert_same(eng.annotate(others, R - 8.0), want, "after a refused call")
    ar.assert_same(eng.annotate(centers, R), first, "the first again")
    # a rebuilt, smaller index on the same handle
    eng.index_build(codes[:5000])
    got = eng.annotate(centers, R)
    ar.assert_same(got, ar.annotate(eng.query(centers, R)), "rebuilt")
    assert len(got["id"]) == 0 or got["id"].max() < 5000
    eng.close()
