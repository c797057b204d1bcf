"""hs_seq_match / hs_seq_match_dev on the GPU: a search's hits reduced per (query group, database protein, diagonal)
on the device, bit for bit against the numpy rule (tests/seqmatch_ref.py) applied to the list call's own output on the
same handle -- across batch sizes (rows that span batches), codes against points, radii, multi-probe, a bucket
partition, without groups, without diagonals --, the capacity protocol, the _dev error paths, and the other sinks
after it."""
import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import annotate_ref as ar
from tests import knn_ref as kr
from tests import seqmatch_ref as sr

pytestmark = pytest.mark.gpu

_K, _R = sr.K_MER, sr.R


@pytest.fixture(scope="module")
def case():
    P = sr.make_proteins()
    id_start = capi.window_id_start(P["db_start"], _K)
    Q = capi.protein_queries(P["qry"], P["qry_start"], _K)
    a, b = synth.make_planes(_K, sr.LSH["K"], sr.LSH["L"], sr.LSH["W"])
    eng = Engine(_K, sr.LSH["K"], sr.LSH["L"], sr.LSH["W"], a, b)
    info, _ = eng.index_build_windows(P["db"], P["db_start"])
    assert int(id_start[-1]) == info["n"] and len(id_start) - 1 == 60 and 3000 < info["n"] < 5000
    c = dict(eng=eng, id_start=id_start, n_groups=len(P["qry_start"]) - 1, **Q)
    c["hits"] = eng.query_codes(Q["qcodes"], _R)
    c["want"] = sr.seq_match(c["hits"], id_start, Q["q_group"], Q["q_off"])
    yield c
    eng.close()


def _match(c, queries=None, **kw):
    args = dict(R=_R, codes=True, q_group=c["q_group"], n_groups=c["n_groups"], q_off=c["q_off"])
    args.update(kw)
    return c["eng"].seq_match(c["qcodes"] if queries is None else queries, c["id_start"], **args)


def _check(got, hits, want, what):
    sr.assert_same(got, want, what)
    assert got["n_hits"] == len(hits["q"]) == int(want["count"].astype(np.int64).sum()), what
    assert len(got["count"]) <= got["n_hits"]


def test_the_construction_is_a_test(case):
    want, hits, id_start = case["want"], case["hits"], case["id_start"]
    lens = np.diff(id_start.astype(np.int64))
    print("hits %d, rows %d, largest %d, single %d" % (len(hits["q"]), len(want["count"]), want["count"].max(),
                                                     (want["count"] == 1).sum()))
    assert want["count"].max() >= 130, "no row of more than two waves"
    big = int(np.argmax(want["count"]))
    assert want["best_dist"][big] == 0.0  # ... and its best is decided by (q, id)
    assert (want["count"] == 1).sum() >= 50
    assert (want["diag"] < 0).any() and (want["diag"] > 0).any()
    assert ((want["lo"] == 0) & (want["hi"] == lens[want["seq"]] - 1)).any() or \
        ((want["lo"] == 0).any() and (want["hi"] == lens[want["seq"]] - 1).any())
    # at 37 queries per batch some row has hits of two batches
    q = hits["q"].astype(np.int64)
    s = np.searchsorted(id_start.astype(np.int64), hits["id"], side="right") - 1
    off = hits["id"] - id_start.astype(np.int64)[s]
    key = np.stack([case["q_group"][q].astype(np.int64), s, off - case["q_off"][q].astype(np.int64)], 1)
    spans = {}
    for kk, batch in zip(map(tuple, key), q // 37):
        spans.setdefault(kk, set()).add(int(batch))
    assert max(len(v) for v in spans.values()) >= 2


def test_batch_sizes_give_identical_rows(case):
    eng = case["eng"]
    for qb in (0, 37):
        eng.set_option("query_batch", qb)
        _check(_match(case), case["hits"], case["want"], ("query_batch", qb))
    # one query per batch: every row of more than one hit spans batches
    eng.set_option("query_batch", 1)
    try:
        got = _match(case)
    finally:
        eng.set_option("query_batch", 0)
    _check(got, case["hits"], case["want"], ("query_batch", 1))


def test_rows_that_span_workgroups(case):
    # every query protein seven times over, all copies in the protein's group: the long diagonal holds 7 x 151 hits at
    # distance +0 -- more than four workgroups of the reduction -- and its best is the smallest (q, id) of them
    eng = case["eng"]
    rep = dict(case, qcodes=np.tile(case["qcodes"], (7, 1)), q_group=np.tile(case["q_group"], 7),
               q_off=np.tile(case["q_off"], 7))
    hits = eng.query_codes(rep["qcodes"], _R)
    want = sr.seq_match(hits, case["id_start"], rep["q_group"], rep["q_off"])
    assert len(hits["q"]) == 7 * len(case["hits"]["q"]) and want["count"].max() >= 7 * 130
    assert np.array_equal(want["best_q"], case["want"]["best_q"]) and len(want["count"]) == len(case["want"]["count"])
    for qb in (0, 1000):
        eng.set_option("query_batch", qb)
        _check(_match(rep), hits, want, ("tiled", qb))
    eng.set_option("query_batch", 0)
    # one group, no diagonals: one row per protein that is hit at all
    one = np.zeros(len(rep["qcodes"]), dtype=np.uint32)
    _check(_match(rep, q_group=one, n_groups=1, q_off=None), hits, sr.seq_match(hits, case["id_start"], one, None),
           "one group")


def test_codes_against_points(case):
    eng = case["eng"]
    pts = synth.embed(case["qcodes"])
    _check(_match(case, pts, codes=False), case["hits"], case["want"], "k-mer centres")
    eng.set_option("recognise_kmers", 0)
    try:
        hits = eng.query(pts, _R)
        got = _match(case, pts, codes=False)
    finally:
        eng.set_option("recognise_kmers", 1)
    _check(got, hits, sr.seq_match(hits, case["id_start"], case["q_group"], case["q_off"]), "as points")
    jit = pts + np.random.default_rng(2).normal(0, 0.2, size=pts.shape)
    hits = eng.query(jit, _R)
    assert 0 < len(hits["q"])
    _check(_match(case, jit, codes=False), hits, sr.seq_match(hits, case["id_start"], case["q_group"], case["q_off"]),
           "jittered points")


def test_radii(case):
    eng = case["eng"]
    radii = np.random.default_rng(4).choice(np.array([0.0, 6.0, 12.0, 20.0, -1.0]), len(case["qcodes"]))
    hits = eng.query_radii(case["qcodes"], radii, codes=True)
    want = sr.seq_match(hits, case["id_start"], case["q_group"], case["q_off"])
    assert 0 < len(want["count"]) and len(hits["q"]) != len(case["hits"]["q"])
    for qb in (0, 37):
        eng.set_option("query_batch", qb)
        _check(_match(case, R=None, radii=radii), hits, want, ("radii", qb))
    eng.set_option("query_batch", 0)


def test_multiprobe(case):
    eng = case["eng"]
    eng.set_multiprobe(3)
    try:
        hits = eng.query_codes(case["qcodes"], _R)
        want = sr.seq_match(hits, case["id_start"], case["q_group"], case["q_off"])
        assert len(hits["q"]) >= len(case["hits"]["q"])
        for qb in (0, 37):
            eng.set_option("query_batch", qb)
            _check(_match(case), hits, want, ("multiprobe", qb))
    finally:
        eng.set_option("query_batch", 0)
        eng.set_multiprobe(0)


def test_bucket_partition(case):
    eng = case["eng"]
    parts, lists = [], []
    try:
        for part in range(3):
            eng.set_bucket_partition(part, 3)
            hits = eng.query_codes(case["qcodes"], _R)
            got = _match(case)
            _check(got, hits, sr.seq_match(hits, case["id_start"], case["q_group"], case["q_off"]), ("part", part))
            assert len(got["count"]) > 0
            parts.append(got)
            lists.append(hits)
    finally:
        eng.set_bucket_partition(0, 1)
    # the parts' LISTS (one (q, id) may be in several) through the host form are the whole
    q, id, dist = (np.concatenate([h[f] for h in lists]) for f in ("q", "id", "dist"))
    assert len(q) > len(case["hits"]["q"])
    whole = capi.seq_match_hits(q, id, dist, len(case["qcodes"]), case["id_start"], q_group=case["q_group"],
                                n_groups=case["n_groups"], q_off=case["q_off"])
    sr.assert_same(whole, case["want"], "parts through seq_match_hits")


def test_without_groups_and_without_diagonals(case):
    hits, id_start = case["hits"], case["id_start"]
    got = _match(case, q_group=None, n_groups=None)
    _check(got, hits, sr.seq_match(hits, id_start, None, case["q_off"]), "rows per centre")
    assert len(got["count"]) == len(hits["q"])  # a centre meets a window once
    got = _match(case, q_off=None)
    want = sr.seq_match(hits, id_start, case["q_group"], None)
    _check(got, hits, want, "no diagonals")
    assert (got["diag"] == 0).all() and len(want["count"]) < len(case["want"]["count"])
    assert (want["hi"] > want["lo"]).any()
    got = _match(case, q_group=None, n_groups=None, q_off=None)
    _check(got, hits, sr.seq_match(hits, id_start, None, None), "neither")
    # no query, and a radius without hits
    got = _match(case, case["qcodes"][:0], q_group=case["q_group"][:0], q_off=case["q_off"][:0])
    assert got["n_hits"] == 0 and all(len(got[f]) == 0 for f in sr.FIELDS)
    far = synth.make_db(40, _K, seed=99)  # random k-mers: nothing within R
    assert len(case["eng"].query_codes(far, _R)["q"]) == 0
    got = case["eng"].seq_match(far, id_start, R=_R, codes=True, q_off=np.arange(40, dtype=np.uint32))
    assert got["n_hits"] == 0 and all(len(got[f]) == 0 for f in sr.FIELDS)
    # a negative radius behaves as it does in the list call
    hits = case["eng"].query_codes(case["qcodes"], -1.0)
    _check(_match(case, R=-1.0), hits, sr.seq_match(hits, id_start, case["q_group"], case["q_off"]), "R = -1")


def _dev(torch, case, cap, fill=-7):
    bufs = [torch.full((max(cap, 1),), fill, dtype=torch.float64 if t == np.float64 else torch.int32, device="cuda")
            for _, t in capi.SEQ_MATCH_FIELDS]
    ins = dict(q=torch.from_numpy(case["qcodes"]).cuda(), g=torch.from_numpy(case["q_group"].view(np.int32)).cuda(),
               o=torch.from_numpy(case["q_off"].view(np.int32)).cuda(),
               s=torch.from_numpy(case["id_start"].view(np.int64)).cuda())
    torch.cuda.synchronize()
    return bufs, ins


def _dev_call(case, bufs, ins, cap, R=_R, d_radii=None, n_groups=None, id_start=None):
    return case["eng"].seq_match_dev(ins["q"].data_ptr(), len(case["qcodes"]), R, d_radii, ins["g"].data_ptr(),
                                     case["n_groups"] if n_groups is None else n_groups, ins["o"].data_ptr(),
                                     (ins["s"] if id_start is None else id_start).data_ptr(), len(case["id_start"]) - 1,
                                     [t.data_ptr() for t in bufs], cap, codes=True)


def _dev_rows(bufs, n):
    return {name: t[:n].cpu().numpy().view(dtype) if dtype != np.float64 else t[:n].cpu().numpy()
            for (name, dtype), t in zip(capi.SEQ_MATCH_FIELDS, bufs)}


def test_dev_form_and_two_call_capacity(case):
    import ctypes as C
    import torch
    need = len(case["want"]["count"])
    bufs, ins = _dev(torch, case, need)
    with pytest.raises(capi.HsError) as e:
        _dev_call(case, bufs, ins, need - 1)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == need
    assert all(bool((t == -7).all()) for t in bufs), "a call that reports the capacity writes no row"
    n, nh = _dev_call(case, bufs, ins, need)
    assert (n, nh) == (need, len(case["hits"]["q"]))
    sr.assert_same(_dev_rows(bufs, n), case["want"], "dev")
    # the host form: cap one too small, nothing written, *n_out right
    outs = [np.full(need, 0x5A, dtype=t) for _, t in capi.SEQ_MATCH_FIELDS]
    n_out, n_hits = C.c_uint64(0), C.c_uint64(0)
    eng = case["eng"]
    st = eng._lib.hs_seq_match(eng._h, None, capi._vp(case["qcodes"]), len(case["qcodes"]), _R, None,
                               capi._vp(case["q_group"]), case["n_groups"], capi._vp(case["q_off"]),
                               capi._vp(case["id_start"]), len(case["id_start"]) - 1, *[capi._vp(o) for o in outs],
                               need - 1, C.byref(n_out), C.byref(n_hits))
    assert st == capi.HS_ERR_CAPACITY and n_out.value == need and n_hits.value == len(case["hits"]["q"])
    assert all((o == 0x5A).all() for o in outs)


def test_dev_error_paths_write_nothing(case):
    import torch
    cap = len(case["want"]["count"])
    bufs, ins = _dev(torch, case, cap)
    bad_start = case["id_start"].copy()
    bad_start[7], bad_start[8] = bad_start[8] + 1, bad_start[7]
    assert (np.diff(bad_start.astype(np.int64)) < 0).any()
    short = case["id_start"].copy()
    short[-1] -= 1
    radii = np.full(len(case["qcodes"]), _R)
    radii[len(radii) // 2] = np.nan
    d_bad, d_short = (torch.from_numpy(x.view(np.int64)).cuda() for x in (bad_start, short))
    d_radii = torch.from_numpy(radii).cuda()
    torch.cuda.synchronize()
    for what, kw in (("id_start descends", dict(id_start=d_bad)), ("id_start ends before n", dict(id_start=d_short)),
                     ("a group out of range", dict(n_groups=case["n_groups"] - 2)),
                     ("a NaN radius", dict(d_radii=d_radii.data_ptr()))):
        with pytest.raises(capi.HsError) as e:
            _dev_call(case, bufs, ins, cap, **kw)
        assert e.value.status == capi.HS_ERR_INVALID, what
        assert all(bool((t == -7).all()) for t in bufs), what
    # the host form finds the same
    for kw in (dict(id_start=bad_start), dict(n_groups=case["n_groups"] - 2), dict(R=None, radii=radii),
               dict(R=float("nan"))):
        with pytest.raises(capi.HsError) as e:
            if "id_start" in kw:
                case["eng"].seq_match(case["qcodes"], kw["id_start"], R=_R, codes=True, q_group=case["q_group"],
                                      n_groups=case["n_groups"], q_off=case["q_off"])
            else:
                _match(case, **kw)
        assert e.value.status == capi.HS_ERR_INVALID, kw.keys()
    # and the next call is clean
    n, nh = _dev_call(case, bufs, ins, cap)
    sr.assert_same(_dev_rows(bufs, n), case["want"], "after the refused calls")


def test_the_other_sinks_after_it(case):
    eng = case["eng"]
    _check(_match(case), case["hits"], case["want"], "once more")
    hits = eng.query_codes(case["qcodes"], _R)
    for f in ("q", "id", "table", "dist", "cand"):
        assert np.array_equal(hits[f], case["hits"][f]), f
    ar.assert_same(eng.annotate(case["qcodes"], _R, codes=True), ar.annotate(hits), "annotate")
    got = eng.query_topk(case["qcodes"], 5, R=_R, codes=True)
    assert kr.same_rows(got, kr.topk_rows(hits["q"], hits["id"], hits["table"], hits["dist"], len(case["qcodes"]), 5))
