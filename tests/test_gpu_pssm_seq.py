"""hs_pssm_seq_scan on the GPU against the numpy rule of tests/pssm_seq_ref.py over tests/pssm_ref.py's scan: rows,
n_hits, cnt and seq_cnt bit for bit -- over a windows index of proteins around k, over runs cut by one and by many
wave edges, over a search deeper than the LDS samples; identical rows across the filter setting, the profile batch, a
forced survivor split, a loaded index and device pointers; the capacity protocol, every refusal, and the handle's
other calls around it."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import pssm_ref, pssm_seq_ref as ref, seqmatch_ref

pytestmark = pytest.mark.gpu

K, A = 15, 20


def _engine(k=K, codes=None, hooks=False, options=None):
    a, b = synth.make_planes(k, 2, 1, 200.0, seed=3)
    eng = Engine(k, 2, 1, 200.0, a, b, hooks=hooks, options=options)
    if codes is not None:
        eng.index_build(codes)
    return eng


def _windows(residues, seq_start, k=K):
    """codes [n][k] of the windows index over the proteins, and id_start"""
    lens = np.diff(seq_start.astype(np.int64))
    pos = np.concatenate([np.arange(s, s + max(0, l - k + 1)) for s, l in zip(seq_start[:-1].astype(np.int64), lens)]
                         + [np.empty(0, dtype=np.int64)]).astype(np.int64)
    codes = residues[pos[:, None] + np.arange(k)[None, :]] if len(pos) else np.empty((0, k), np.uint8)
    return np.ascontiguousarray(codes, dtype=np.uint8), capi.window_id_start(seq_start, k)


_CASE = {}


def _proteins():
    """The proteins of seqmatch_ref.make_proteins (0, fewer than k, exactly k, 300 residues; about 4000 windows), the
    33 profiles of tests/test_gpu_pssm.py's mix, the reference hits and rows of all 33 -- computed once."""
    if not _CASE:
        P = seqmatch_ref.make_proteins(K)
        codes, id_start = _windows(P["db"], P["db_start"])
        n = len(codes)
        rng = np.random.default_rng(1000 * K + n)
        S = rng.normal(0, 2, size=(33, K, A))
        S[::2] = rng.integers(-16, 17, size=S[::2].shape) / 4.0      # dyadic entries: equal scores are common
        S[3, :, 0] = -1e30                                           # a forbidden residue
        S[11] = rng.integers(-1, 2, size=S[11].shape) / 2.0          # very coarse: the best of a row is often tied
        sc = pssm_ref.scores(S, codes)
        t = np.sort(sc, axis=1)[:, -max(1, n // 20)].copy()          # an attained score: about a twentieth hit
        t[5] = sc[5].max() + 1e3                                     # dead
        t[7] = -1e6                                                  # everything hits
        t[9] = sc[9].max()                                           # attained by (almost surely) one window
        t[11] = np.sort(sc[11])[-n // 3]
        hit = sc >= t[:, None]
        m, i = np.nonzero(hit)
        hits = dict(m=m.astype(np.uint32), id=i.astype(np.uint32), score=sc[m, i])
        _CASE.update(P=P, codes=codes, id_start=id_start, S=S, t=t, sc=sc, hits=hits, n=n)
    return _CASE


def _want(case, nm):
    keep = case["hits"]["m"] < nm
    return ref.rows_from_hits(case["hits"]["m"][keep], case["hits"]["id"][keep], case["hits"]["score"][keep], nm,
                              case["id_start"])


@pytest.fixture(scope="module")
def prot():
    case = _proteins()
    eng = _engine()
    info, _ = eng.index_build_windows(case["P"]["db"], case["P"]["db_start"])
    assert info["n"] == case["n"] == int(case["id_start"][-1]) and 3000 < case["n"] < 5000
    yield dict(case, eng=eng)
    eng.close()


def test_the_construction_is_a_test():
    case = _proteins()
    want = _want(case, 33)
    lens = np.diff(case["P"]["db_start"].astype(np.int64))
    assert (lens == 0).any() and ((lens > 0) & (lens < K)).any() and (lens == K).any() and (lens == 300).any()
    wins = np.diff(case["id_start"].astype(np.int64))
    # the dead profile has no row; the everything-hits profile one row per protein that has windows
    assert want["seq_cnt"][5] == 0 and want["cnt"][5] == 0
    all_hit = want["m"] == 7
    assert np.array_equal(want["seq"][all_hit], np.flatnonzero(wins > 0))
    assert np.array_equal(want["count"][all_hit], wins[wins > 0]) and np.all(want["lo"][all_hit] == 0)
    assert np.array_equal(want["hi"][all_hit], wins[wins > 0] - 1)
    assert want["cnt"][9] == 1 and want["seq_cnt"][9] == 1
    # ties for the best of a row exist, and the row took the smaller id
    h, tied = case["hits"], 0
    for r in np.flatnonzero(want["m"] == 11):
        s = int(want["seq"][r])
        sel = (h["m"] == 11) & (h["score"] == want["best_score"][r])
        sel &= (h["id"] >= case["id_start"][s]) & (h["id"] < case["id_start"][s + 1])
        tied += int(sel.sum() > 1)
        assert want["best_id"][r] == h["id"][sel].min()
    assert tied >= 5
    assert int(want["count"].sum()) == want["n_hits"] == len(h["m"])


@pytest.mark.parametrize("nm", [1, 17, 33])
def test_rows_equal_the_rule(prot, nm):
    eng = prot["eng"]
    want = _want(prot, nm)
    got = eng.pssm_seq_scan(prot["S"][:nm], prot["t"][:nm], prot["id_start"])
    ref.same_rows(got, want, nm)
    p = eng.profile()
    assert p["pssm_seq_rows"] == len(want["m"]) and p["hits"] == want["n_hits"]
    listed = eng.pssm_scan(prot["S"][:nm], prot["t"][:nm])
    assert eng.profile()["pssm_survivors"] == p["pssm_survivors"] and eng.profile()["pssm_dead"] == p["pssm_dead"]
    # the list call on the same handle, reduced on the host, is the same rows
    ref.same_rows(capi.pssm_seq_hits(listed["m"], listed["id"], listed["score"], nm, prot["id_start"]), got, "list")


def _run_db(wins, k=K, seed=3):
    """a database whose sequences have exactly `wins` windows (0: a sequence shorter than k)"""
    rng = np.random.default_rng(seed)
    lens = [w + k - 1 if w else int(rng.integers(0, k)) for w in wins]
    residues = rng.integers(0, A, size=sum(lens)).astype(np.uint8)
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return residues, seq_start


def test_run_boundaries():
    """Sequences of 1, 63, 64, 65, 129 and 4097 windows under the everything-hits profile: runs inside a wave, cut by
    one and by many wave edges, one row holding most of the batch; then with a second profile, whose first row starts
    inside a wave (4419 = 69 x 64 + 3 hits before it)."""
    wins = [1, 63, 64, 65, 129, 4097]
    residues, seq_start = _run_db(wins)
    codes, id_start = _windows(residues, seq_start)
    rng = np.random.default_rng(17)
    S = rng.integers(-2, 3, size=(2, K, A)) / 2.0        # coarse: the best of 4097 windows is tied across waves
    t = np.array([-1e6, -1e6])
    sc = pssm_ref.scores(S, codes)
    assert (sc[0] == sc[0].max()).sum() >= 2 and sum(wins) % 64 != 0
    eng = _engine()
    try:
        info, _ = eng.index_build_windows(residues, seq_start)
        assert info["n"] == sum(wins)
        for nm in (1, 2):
            want = ref.rows(pssm_ref.scan(S[:nm], t[:nm], codes), nm, id_start)
            assert want["count"].tolist() == wins * nm
            got = eng.pssm_seq_scan(S[:nm], t[:nm], id_start)
            ref.same_rows(got, want, nm)
            assert got["seq_cnt"].tolist() == [6] * nm and got["cnt"].tolist() == [sum(wins)] * nm
        # a threshold that leaves the long sequence a sparse run, and rows whose hits are few
        t2 = np.sort(sc, axis=1)[:, -300].copy()
        want = ref.rows(pssm_ref.scan(S, t2, codes), 2, id_start)
        ref.same_rows(eng.pssm_seq_scan(S, t2, id_start), want, "sparse")
    finally:
        eng.close()


def test_deep_search_one_sequence_and_a_plain_index():
    """1000 sequences of 0 .. 8 windows: four global steps of the search below the 256 LDS samples.  n_seq = 1.  An
    id_start over a plain (non-windows) index."""
    rng = np.random.default_rng(29)
    wins = rng.integers(0, 9, size=1000)
    wins[[0, 1, 500, 998, 999]] = 0
    n = int(wins.sum())
    codes = rng.integers(0, A, size=(n, K)).astype(np.uint8)
    id_start = np.concatenate([[0], np.cumsum(wins)]).astype(np.uint64)
    S = rng.integers(-8, 9, size=(5, K, A)) / 4.0
    t = np.sort(pssm_ref.scores(S, codes), axis=1)[:, -n // 10].copy()
    t[2] = -1e6
    hits = pssm_ref.scan(S, t, codes)
    eng = _engine(codes=codes)
    try:
        want = ref.rows(hits, 5, id_start)
        assert want["seq_cnt"][2] == (wins > 0).sum() and len(want["m"]) > 1000
        ref.same_rows(eng.pssm_seq_scan(S, t, id_start), want, "1000 sequences")
        one = np.array([0, n], dtype=np.uint64)
        want1 = ref.rows(hits, 5, one)
        assert len(want1["m"]) == 5 and want1["count"].tolist() == hits["cnt"].tolist()
        ref.same_rows(eng.pssm_seq_scan(S, t, one), want1, "one sequence")
        # every k-mer its own sequence: as many rows as hits
        each = np.arange(n + 1, dtype=np.uint64)
        got = eng.pssm_seq_scan(S, t, each)
        ref.same_rows(got, ref.rows(hits, 5, each), "one id per sequence")
        assert len(got["m"]) == got["n_hits"] == len(hits["m"])
    finally:
        eng.close()


def test_filter_and_batches_do_not_show(prot):
    want = _want(prot, 33)
    eng = prot["eng"]
    surv = None
    try:
        for filt in (1, 0):
            eng.set_option("pssm_filter", filt)
            for batch in (1, 16, 0):
                eng.set_option("query_batch", batch)
                ref.same_rows(eng.pssm_seq_scan(prot["S"], prot["t"], prot["id_start"]), want, (filt, batch))
                s = eng.profile()["pssm_survivors"]
                eng.pssm_scan(prot["S"], prot["t"])
                assert s == eng.profile()["pssm_survivors"]
                if filt:
                    surv = s if surv is None else surv
                    assert s == surv < 33 * prot["n"]
                else:
                    assert s == 33 * prot["n"]
    finally:
        eng.set_option("pssm_filter", 1)
        eng.set_option("query_batch", 0)


def test_forced_split_and_loaded_index(prot, monkeypatch, tmp_path):
    """The TEST build reports a survivor-counter overflow for every batch of more than 4 profiles: the same profiles
    run again in smaller batches and nothing shows.  The same rows from a saved and loaded index."""
    want = _want(prot, 33)
    path = tmp_path / "p.idx"
    prot["eng"].index_save(path)
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "4")
    eng = _engine(hooks=True)
    try:
        eng.index_load(path)
        ref.same_rows(eng.pssm_seq_scan(prot["S"], prot["t"], prot["id_start"]), want, "split, loaded")
        p = eng.profile()
        assert p["verify_launches"] >= 9
        eng.pssm_scan(prot["S"], prot["t"])
        assert eng.profile()["pssm_survivors"] == p["pssm_survivors"]
    finally:
        eng.close()


def _dev_rows(torch, cap, fill=7):
    return [torch.full((cap,), fill, dtype=torch.float64 if t == np.float64 else torch.int32, device="cuda")
            for _, t in capi.PSSM_SEQ_FIELDS]


def _dev_dict(rows, n, dc, ds, nh):
    got = {name: r[:n].cpu().numpy().astype(t) for (name, t), r in zip(capi.PSSM_SEQ_FIELDS, rows)}
    got.update(n_hits=nh, cnt=dc.cpu().numpy().astype(np.uint64), seq_cnt=ds.cpu().numpy().astype(np.uint64))
    return got


def test_device_pointers_capacity_and_refusals(prot):
    import torch
    eng, nm = prot["eng"], 33
    want = _want(prot, nm)
    n_rows = len(want["m"])
    dS, dt = torch.from_numpy(prot["S"]).cuda(), torch.from_numpy(prot["t"]).cuda()
    dI = torch.from_numpy(prot["id_start"].astype(np.int64)).cuda()
    n_seq = len(prot["id_start"]) - 1
    cap = n_rows + 5
    rows = _dev_rows(torch, cap)
    dc = torch.full((nm,), 7, dtype=torch.int64, device="cuda")
    ds = torch.full((nm,), 7, dtype=torch.int64, device="cuda")
    ptrs = [r.data_ptr() for r in rows]
    torch.cuda.synchronize()
    n, nh = eng.pssm_seq_scan_dev(dS.data_ptr(), dt.data_ptr(), nm, dI.data_ptr(), n_seq, ptrs, cap, dc.data_ptr(),
                                  ds.data_ptr())
    assert n == n_rows
    ref.same_rows(_dev_dict(rows, n, dc, ds, nh), want, "dev")
    assert all(float(r[n]) == 7 for r in rows)
    # the two-call pattern: the count with null arrays, then too small by one -- counts valid, no row written
    with pytest.raises(HsError) as e:
        eng.pssm_seq_scan_dev(dS.data_ptr(), dt.data_ptr(), nm, dI.data_ptr(), n_seq, [0] * 7, 0, dc.data_ptr(),
                              ds.data_ptr())
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == n_rows and e.value.n_hits == want["n_hits"]
    assert np.array_equal(dc.cpu().numpy().astype(np.uint64), want["cnt"])
    assert np.array_equal(ds.cpu().numpy().astype(np.uint64), want["seq_cnt"])
    for r in rows:
        r.fill_(9)
    dc.fill_(9), ds.fill_(9)
    torch.cuda.synchronize()
    with pytest.raises(HsError) as e:
        eng.pssm_seq_scan_dev(dS.data_ptr(), dt.data_ptr(), nm, dI.data_ptr(), n_seq, ptrs, n_rows - 1, dc.data_ptr(),
                              ds.data_ptr())
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == n_rows
    assert all(bool((r == 9).all()) for r in rows)
    assert np.array_equal(ds.cpu().numpy().astype(np.uint64), want["seq_cnt"])
    with pytest.raises(HsError) as e:     # the host form
        eng.pssm_seq_scan(prot["S"], prot["t"], prot["id_start"], cap=n_rows - 1)
    assert e.value.needed == n_rows and e.value.n_hits == want["n_hits"]
    assert np.array_equal(e.value.cnt, want["cnt"]) and np.array_equal(e.value.seq_cnt, want["seq_cnt"])
    ref.same_rows(eng.pssm_seq_scan(prot["S"], prot["t"], prot["id_start"], cap=n_rows), want, "exact cap")
    # refusals found on the device, before anything is written
    dc.fill_(9), ds.fill_(9)

    def refused(S=dS, t=dt, I=dI, ns=n_seq, status=capi.HS_ERR_INVALID):
        torch.cuda.synchronize()
        with pytest.raises(HsError) as e:
            eng.pssm_seq_scan_dev(S.data_ptr(), t.data_ptr(), nm, I.data_ptr() if I is not None else 0, ns, ptrs, cap,
                                  dc.data_ptr(), ds.data_ptr())
        assert e.value.status == status
        assert all(bool((r == 9).all()) for r in rows) and bool((dc == 9).all()) and bool((ds == 9).all())

    for where, bad in (("S", float("nan")), ("S", float("inf")), ("S", 2.0 ** 101), ("t", float("nan")),
                       ("t", float("-inf"))):
        S2, t2 = dS.clone(), dt.clone()
        if where == "S":
            S2[20, 13, 7] = bad
        else:
            t2[32] = bad
        refused(S=S2, t=t2)
    for change in ("descends", "starts", "ends"):
        I2 = dI.clone()
        if change == "descends":
            I2[30] = I2[31] + 1
        elif change == "starts":
            I2[0] = 1
        else:
            I2[n_seq] -= 1
        refused(I=I2)
    refused(I=None)
    refused(ns=0)
    refused(ns=(1 << 32) + 1)
    # the host form: the same refusals, with sentinel-filled outputs untouched
    lib, h = eng._lib, eng._h
    out = [np.full(cap, 9, dtype=t) for _, t in capi.PSSM_SEQ_FIELDS]
    cnt, seq_cnt = np.full(nm, 9, np.uint64), np.full(nm, 9, np.uint64)
    n_out, n_hits = C.c_uint64(5), C.c_uint64(5)

    def host(S=prot["S"], t=prot["t"], ids=prot["id_start"], ns=n_seq, nm_=nm):
        st = lib.hs_pssm_seq_scan(h, capi._vp(S), capi._vp(t), C.c_uint64(nm_), None if ids is None else capi._vp(ids),
                                  C.c_uint64(ns), *[capi._vp(a) for a in out], cap, C.byref(n_out), C.byref(n_hits),
                                  capi._vp(cnt), capi._vp(seq_cnt))
        assert n_out.value == 0 and n_hits.value == 0
        assert all(np.all(a == 9) for a in out) and np.all(cnt == 9) and np.all(seq_cnt == 9)
        return st

    S2 = prot["S"].copy()
    S2[1, 2, 3] = np.nan
    ids = prot["id_start"]
    bad = capi.HS_ERR_INVALID
    assert host(S=S2) == bad
    assert host(t=np.where(np.arange(nm) == 4, np.inf, prot["t"])) == bad
    assert host(nm_=1 << 27) == bad
    assert host(ids=None) == bad
    def changed(at, value):
        c = ids.copy()
        c[at] = value
        return c

    assert host(ids=changed(30, int(ids[31]) + 1)) == bad      # does not ascend
    assert host(ids=changed(0, 1)) == bad                      # does not start at 0
    assert host(ids=changed(n_seq, int(ids[-1]) + 1)) == bad   # does not end at n
    assert host(ns=0) == bad
    assert host(ns=(1 << 32) + 1) == bad
    # nm = 0 is an empty, successful call
    empty = eng.pssm_seq_scan(np.zeros((0, K, A)), np.zeros(0), prot["id_start"])
    assert len(empty["m"]) == 0 and empty["n_hits"] == 0
    unbuilt = _engine()
    try:
        with pytest.raises(HsError) as e:
            unbuilt.pssm_seq_scan(prot["S"], prot["t"], prot["id_start"])
        assert e.value.status == capi.HS_ERR_STATE
    finally:
        unbuilt.close()


def test_other_calls_around_it():
    """hs_pssm_scan, hs_pssm_topk and hs_seq_match on the same handle give what they gave, before and after."""
    case = _proteins()
    P = case["P"]
    Q = capi.protein_queries(P["qry"], P["qry_start"], K)
    lsh = seqmatch_ref.LSH
    a, b = synth.make_planes(K, lsh["K"], lsh["L"], lsh["W"])
    eng = Engine(K, lsh["K"], lsh["L"], lsh["W"], a, b)
    try:
        eng.index_build_windows(P["db"], P["db_start"])
        S, t, ids = case["S"][:17], case["t"][:17], case["id_start"]

        def others():
            return (eng.pssm_scan(S, t), eng.pssm_topk(S, 5),
                    eng.seq_match(Q["qcodes"], ids, R=seqmatch_ref.R, codes=True, q_group=Q["q_group"],
                                  n_groups=len(P["qry_start"]) - 1, q_off=Q["q_off"]))

        before = others()
        ref.same_rows(eng.pssm_seq_scan(S, t, ids), _want(case, 17), "between")
        after = others()
        for x, y in zip(before, after):
            assert x.keys() == y.keys()
            for f in x:
                assert np.array_equal(x[f], y[f]), f
        assert len(before[0]["m"]) > 0 and len(before[2]["count"]) > 0
    finally:
        eng.close()
