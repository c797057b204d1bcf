"""hs_pssm_topk on the GPU against the numpy contract of tests/pssm_topk_ref.py: rows, counts and t_used bit for bit;
the filter's survivor count against the count the host tables predict at t_used (which ties the device's thresholds
to the host tables); sample sizes, batches, a forced split and the unfiltered path, none of which may show in a row;
edge profiles, windows and loaded indexes, device pointers, refusals, and the handle's other calls around a call."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import pssm_ref
from tests import pssm_topk_ref as ref

pytestmark = pytest.mark.gpu

NO_ID = 0xffffffff
# (k, alphabet, n): four MFMA steps; every row full of ties (the id order decides); the NS = 0 filter path (19 steps)
SHAPES = [(25, 20, 5000), (3, 4, 200), (75, 32, 300)]
NM = 33   # three profile tiles, the last ragged
DEFAULT_SAMPLE = 262144   # HS_OPT_PSSM_TOPK_SAMPLE as a handle starts


def _coords(A):
    if A == 20:
        return None
    rng = np.random.default_rng(77)
    base = synth.coords()
    if A < 20:
        return np.ascontiguousarray(base[:A])
    return np.ascontiguousarray(np.concatenate([base, rng.normal(0, 3, size=(A - 20, 8))]))


def _engine(k, A, codes=None, hooks=False, options=None):
    a, b = synth.make_planes(k, 2, 1, 200.0, seed=3)
    eng = Engine(k, 2, 1, 200.0, a, b, coords=_coords(A), hooks=hooks, options=options)
    if codes is not None:
        eng.index_build(codes)
    return eng


_CASES = {}


def _case(k, A, n):
    """codes [n][k], 33 profiles and their scores (computed once per shape)."""
    key = (k, A, n)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * k + 10 * A + n)
        codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
        S = rng.normal(0, 2, size=(NM, k, A))
        S[::2] = rng.integers(-16, 17, size=S[::2].shape) / 4.0      # dyadic entries: equal scores are common
        if k == 3:
            S = rng.integers(-1, 2, size=S.shape).astype(np.float64)  # 64 distinct k-mers, 7 distinct scores
        S[3, :, 0] = -1e30                                           # a forbidden residue
        sc = pssm_ref.scores(S, codes)
        sc.setflags(write=False)
        _CASES[key] = dict(codes=codes, S=S, sc=sc)
    return _CASES[key]


def _predicted_survivors(S, t_used, codes):
    T = capi.pssm_tables(S, t_used)
    F = pssm_ref.filter_values(T["code"], codes)
    return int(((F >= T["tau"][:, None]) & (T["dead"] == 0)[:, None]).sum()), int(T["dead"].sum())


def _check(eng, case, topk, sample, nm=NM, t_floor=None, what=""):
    """One call against the reference: rows, counts, t_used, the profile's fields and the exact survivor count."""
    sc, S = case["sc"][:nm], case["S"][:nm]
    n = sc.shape[1]
    got = eng.pssm_topk(S, topk, t_floor=t_floor, want_thresholds=True)
    ref.same_rows(got, ref.rows_from_scores(sc, topk, t_floor), what)
    tu = ref.t_used_from_scores(sc, topk, sample, t_floor)
    assert np.array_equal(got["t_used"].view(np.uint64), tu.view(np.uint64)), what
    p = eng.profile()
    floor = np.full(nm, ref.NO_FLOOR) if t_floor is None else np.asarray(t_floor)
    assert p["pssm_topk_sample"] == min(n, sample) and p["pssm_topk_raised"] == int((tu > floor).sum()), what
    return got, tu, p


@pytest.mark.parametrize("topk", [1, 10, 64])
@pytest.mark.parametrize("k,A,n", SHAPES)
def test_rows_equal_contract(k, A, n, topk):
    case = _case(k, A, n)
    eng = _engine(k, A, case["codes"])
    try:
        got, tu, p = _check(eng, case, topk, DEFAULT_SAMPLE, what=(k, A, n, topk))
        surv, dead = _predicted_survivors(case["S"], tu, case["codes"])
        assert dead == 0 and p["pssm_dead"] == 0 and p["pssm_pairs"] == NM * n
        assert p["pssm_survivors"] == surv, (k, A, n, topk)
        assert p["pssm_mfma_steps"] == -(-k * A // 128) and p["pssm_topk_raised"] == NM
        assert np.all(got["count"] == topk) and p["hits"] == int((case["sc"] >= tu[:, None]).sum())
        if k == 3:   # ties fill every row: equal scores side by side, ids ascending among them
            s, i = got["score"], got["id"].astype(np.int64)
            assert np.all((s[:, 1:] < s[:, :-1]) | ((s[:, 1:] == s[:, :-1]) & (i[:, 1:] > i[:, :-1])))
            if topk > 7:
                assert np.any(s[:, 1:] == s[:, :-1])
    finally:
        eng.close()


def test_index_shorter_than_the_row():
    case = _case(25, 20, 5000)
    small = dict(codes=case["codes"][:7], S=case["S"], sc=case["sc"][:, :7])
    eng = _engine(25, 20, small["codes"])
    try:
        got, tu, p = _check(eng, small, 10, DEFAULT_SAMPLE)
        assert np.all(got["count"] == 7) and np.all(got["id"][:, 7:] == NO_ID) and np.all(np.isneginf(got["score"][:, 7:]))
        assert np.all(tu == ref.NO_FLOOR) and p["pssm_topk_raised"] == 0 and p["hits"] == 7 * NM
    finally:
        eng.close()


@pytest.mark.parametrize("topk", [10, 64])
def test_sample_size_does_not_show_in_the_rows(topk):
    k, A, n = 25, 20, 5000
    case = _case(k, A, n)
    want = ref.rows_from_scores(case["sc"], topk)
    for sample in (1, 63, 64, 65, n, 10 * n):
        eng = _engine(k, A, case["codes"], options={"pssm_topk_sample": sample})
        try:
            got, tu, p = _check(eng, case, topk, sample, what=(topk, sample))
            ref.same_rows(got, want, sample)
            surv, dead = _predicted_survivors(case["S"], tu, case["codes"])
            assert p["pssm_survivors"] == surv and p["pssm_dead"] == dead == 0, (topk, sample)
            assert p["pssm_topk_raised"] == (NM if sample >= topk else 0)
        finally:
            eng.close()
    eng = _engine(k, A)
    try:
        with pytest.raises(HsError):
            eng.set_option("pssm_topk_sample", 0)
    finally:
        eng.close()


def test_the_sample_cuts_the_work():
    """Log-odds profiles over 20 000 25-mers at sample = 4096: every profile is raised, and the filter passes far fewer
    than a quarter of the pairs (the expectation is about topk * n / n_s = 49 hits per profile)."""
    rng = np.random.default_rng(2024)
    n, k, A, nm, topk = 20000, 25, 20, 16, 10
    codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
    counts = np.stack([np.stack([rng.multinomial(30, rng.dirichlet(np.full(A, 0.3))) for _ in range(k)])
                       for _ in range(nm)])
    S = capi.pssm_log_odds(counts, background=np.full(A, 1.0 / A), pseudo=1.0)
    case = dict(codes=codes, S=S, sc=pssm_ref.scores(S, codes))
    tu = ref.t_used_from_scores(case["sc"], topk, 4096)
    surv, dead = _predicted_survivors(S, tu, codes)
    assert dead == 0 and surv < nm * n // 4          # the inputs satisfy it on the host tables
    eng = _engine(k, A, codes, options={"pssm_topk_sample": 4096})
    try:
        got, tu2, p = _check(eng, case, topk, 4096, nm=nm)
        assert p["pssm_survivors"] == surv < nm * n // 4 and p["pssm_topk_raised"] == nm
        assert p["hits"] == int((case["sc"] >= tu[:, None]).sum()) >= nm * topk
    finally:
        eng.close()


def test_edge_profiles():
    k, A, n, topk = 25, 20, 5000, 10
    case = _case(k, A, n)
    S = case["S"][:8].copy()
    S[2] = 1.25                                          # a constant profile: every k-mer ties
    sc = pssm_ref.scores(S, case["codes"])
    srt = np.sort(sc, axis=1)
    floor = np.full(8, ref.NO_FLOOR)
    floor[4] = srt[4, -1] + 1.0                          # above every score
    assert srt[5, -3] > srt[5, -4]
    floor[5] = 0.5 * (srt[5, -3] + srt[5, -4])           # between the 3rd and the 4th best
    floor[6] = srt[6, -1]                                # the best score itself: the tie is in
    local = dict(codes=case["codes"], S=S, sc=sc)
    eng = _engine(k, A, case["codes"])
    try:
        got, tu, p = _check(eng, local, topk, DEFAULT_SAMPLE, nm=8, t_floor=floor)
        assert got["id"][2].tolist() == list(range(topk)) and np.all(got["score"][2] == 1.25 * k)
        assert got["count"].tolist()[4:7] == [0, 3, int((sc[6] >= floor[6]).sum())]
        assert np.all(got["id"][4] == NO_ID) and tu[4] == floor[4]
        assert p["pssm_topk_raised"] == 5 and p["hits"] >= n           # the constant profile costs n hits
        # no floor against an explicit -DBL_MAX
        a = eng.pssm_topk(S, topk, want_thresholds=True)
        b = eng.pssm_topk(S, topk, t_floor=np.full(8, ref.NO_FLOOR), want_thresholds=True)
        ref.same_rows(a, b)
        ref.same_rows(a, ref.rows_from_scores(sc, topk))
        assert np.array_equal(a["t_used"], b["t_used"])
        # nm = 0 is an empty, successful call
        e = eng.pssm_topk(np.zeros((0, k, A)), topk)
        assert e["id"].shape == (0, topk) and len(e["count"]) == 0
    finally:
        eng.close()


def test_batches_splits_and_the_unfiltered_path_do_not_show(monkeypatch):
    k, A, n, topk = 25, 20, 5000, 10
    case = _case(k, A, n)
    want = ref.rows_from_scores(case["sc"][:17], topk)
    eng = _engine(k, A, case["codes"], options={"query_batch": 16})
    try:
        got, tu, p = _check(eng, case, topk, DEFAULT_SAMPLE, nm=17)
        surv, _ = _predicted_survivors(case["S"][:17], tu, case["codes"])
        assert p["pssm_survivors"] == surv and p["verify_launches"] == 2
        eng.set_option("pssm_filter", 0)
        got0, _, p0 = _check(eng, case, topk, DEFAULT_SAMPLE, nm=17)
        ref.same_rows(got0, want, "no filter")
        assert p0["pssm_survivors"] == 17 * n and p0["pssm_mfma_steps"] == 0
    finally:
        eng.close()
    # the library's TEST build reports a survivor overflow for every batch of more than 4 profiles
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "4")
    eng = _engine(k, A, case["codes"], hooks=True)
    try:
        got, tu, p = _check(eng, case, topk, DEFAULT_SAMPLE, nm=17)
        ref.same_rows(got, want, "split")
        assert p["verify_launches"] >= 5 and p["pssm_pairs"] == 17 * n and p["pssm_topk_raised"] == 17
    finally:
        eng.close()


def test_windows_index_and_loaded_index(tmp_path):
    k, A = 25, 20
    rng = np.random.default_rng(9)
    lens = [40, 3, 25, 300, 24, 77]
    residues = rng.integers(0, A, size=sum(lens)).astype(np.uint8)
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    S = rng.integers(-12, 13, size=(5, k, A)) / 4.0
    eng = _engine(k, A)
    try:
        info, pos = eng.index_build_windows(residues, seq_start)
        codes = np.stack([residues[p:p + k] for p in pos])
        case = dict(codes=codes, S=S, sc=pssm_ref.scores(S, codes))
        _check(eng, case, 10, DEFAULT_SAMPLE, nm=5, what="windows")
        path = tmp_path / "w.idx"
        eng.index_save(path)
    finally:
        eng.close()
    eng2 = _engine(k, A)
    try:
        eng2.index_load(path)
        _check(eng2, case, 64, DEFAULT_SAMPLE, nm=5, what="loaded")
    finally:
        eng2.close()


def test_device_pointers_and_refusals():
    import torch
    k, A, n, topk = 25, 20, 5000, 10
    case = _case(k, A, n)
    want = ref.rows_from_scores(case["sc"], topk)
    eng = _engine(k, A, case["codes"])
    try:
        dS = torch.from_numpy(case["S"]).cuda()
        did = torch.full((NM + 1, topk), 7, dtype=torch.int32, device="cuda")
        ds = torch.full((NM + 1, topk), 7.0, dtype=torch.float64, device="cuda")
        dc = torch.full((NM + 1,), 7, dtype=torch.int32, device="cuda")
        dtu = torch.full((NM + 1,), 7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng.pssm_topk_dev(dS.data_ptr(), None, NM, topk, did.data_ptr(), ds.data_ptr(), dc.data_ptr(), dtu.data_ptr())
        got = dict(id=did[:NM].cpu().numpy().astype(np.uint32), score=ds[:NM].cpu().numpy(),
                   count=dc[:NM].cpu().numpy().astype(np.uint32))
        ref.same_rows(got, want, "dev")
        assert np.array_equal(dtu[:NM].cpu().numpy(), ref.t_used_from_scores(case["sc"], topk, DEFAULT_SAMPLE))
        assert bool((did[NM] == 7).all()) and bool((ds[NM] == 7.0).all()) and int(dc[NM]) == 7 and float(dtu[NM]) == 7.0
        # with a floor on the device, and no t_used
        floor = np.sort(case["sc"], axis=1)[:, -4].copy()
        dfl = torch.from_numpy(floor).cuda()
        eng.pssm_topk_dev(dS.data_ptr(), dfl.data_ptr(), NM, topk, did.data_ptr(), ds.data_ptr(), dc.data_ptr())
        got = dict(id=did[:NM].cpu().numpy().astype(np.uint32), score=ds[:NM].cpu().numpy(),
                   count=dc[:NM].cpu().numpy().astype(np.uint32))
        ref.same_rows(got, ref.rows_from_scores(case["sc"], topk, floor), "dev floor")
        # refusals found on the device, before anything is written
        did.fill_(9), ds.fill_(9.0), dc.fill_(9), dtu.fill_(9.0)

        def untouched():
            torch.cuda.synchronize()
            return bool((did == 9).all()) and bool((ds == 9.0).all()) and bool((dc == 9).all()) and bool((dtu == 9.0).all())

        for where, bad in (("S", float("nan")), ("S", float("inf")), ("S", 2.0 ** 101), ("t", float("nan")),
                           ("t", float("-inf"))):
            dS2, dfl2 = dS.clone(), dfl.clone()
            if where == "S":
                dS2[20, 13, 7] = bad
            else:
                dfl2[32] = bad
            torch.cuda.synchronize()
            with pytest.raises(HsError) as e:
                eng.pssm_topk_dev(dS2.data_ptr(), dfl2.data_ptr(), NM, topk, did.data_ptr(), ds.data_ptr(),
                                  dc.data_ptr(), dtu.data_ptr())
            assert e.value.status == capi.HS_ERR_INVALID and untouched()
        for tk in (0, 65):
            with pytest.raises(HsError) as e:
                eng.pssm_topk_dev(dS.data_ptr(), None, NM, tk, did.data_ptr(), ds.data_ptr(), dc.data_ptr(), dtu.data_ptr())
            assert e.value.status == capi.HS_ERR_INVALID and untouched()
        with pytest.raises(HsError) as e:
            eng.pssm_topk_dev(dS.data_ptr(), None, 1 << 27, topk, did.data_ptr(), ds.data_ptr(), dc.data_ptr())
        assert e.value.status == capi.HS_ERR_INVALID and untouched()
        lib, h = eng._lib, eng._h
        assert lib.hs_pssm_topk_dev(h, C.c_void_p(dS.data_ptr()), None, NM, topk, None, C.c_void_p(ds.data_ptr()),
                                    C.c_void_p(dc.data_ptr()), None) == capi.HS_ERR_INVALID and untouched()
        # the host form
        tid, ts = np.full((NM, topk), 7, np.uint32), np.full((NM, topk), 7.0)
        tc, tu = np.full(NM, 7, np.uint32), np.full(NM, 7.0)
        S2 = case["S"].copy()
        S2[1, 2, 3] = np.nan
        fl_bad = np.where(np.arange(NM) == 4, np.inf, floor)
        v = capi._vp
        for Sx, fx, nm, tk, out in ((S2, floor, NM, topk, tid), (case["S"], fl_bad, NM, topk, tid),
                                    (case["S"], floor, 1 << 27, topk, tid), (case["S"], floor, NM, 0, tid),
                                    (case["S"], floor, NM, 65, tid), (case["S"], floor, NM, topk, None)):
            st = lib.hs_pssm_topk(h, v(Sx), v(fx), C.c_uint64(nm), tk, v(out) if out is not None else None, v(ts),
                                  v(tc), v(tu))
            assert st == capi.HS_ERR_INVALID
            assert np.all(tid == 7) and np.all(ts == 7.0) and np.all(tc == 7) and np.all(tu == 7.0)
    finally:
        eng.close()
    unbuilt = _engine(k, A)
    try:
        with pytest.raises(HsError) as e:
            unbuilt.pssm_topk(case["S"], topk)
        assert e.value.status == capi.HS_ERR_STATE
        # no sequence long enough: an empty index, padded rows and zero counts
        info, _ = unbuilt.index_build_windows(np.zeros(10, dtype=np.uint8), np.array([0, 4, 10], dtype=np.uint64))
        assert info["n"] == 0
        floor = np.arange(NM, dtype=np.float64)
        got = unbuilt.pssm_topk(case["S"], topk, t_floor=floor, want_thresholds=True)
        assert np.all(got["id"] == NO_ID) and np.all(np.isneginf(got["score"])) and np.all(got["count"] == 0)
        assert np.array_equal(got["t_used"], floor) and unbuilt.profile()["pssm_topk_raised"] == 0
    finally:
        unbuilt.close()


def test_other_calls_around_a_call():
    """hs_pssm_scan, hs_query_codes and hs_query_topk on the same handle give what they gave, before and after; and the
    scan at t_used, fed through the host rule, gives the same rows."""
    k, topk = 25, 10
    codes = synth.make_db(3000, k, seed=31)
    qcodes = codes[:40].copy()
    a, b = synth.make_planes(k, 4, 3, 120.0, seed=3)
    rng = np.random.default_rng(34)
    S = rng.integers(-12, 13, size=(17, k, 20)) / 4.0
    sc = pssm_ref.scores(S, codes)
    t = np.sort(sc, axis=1)[:, -40].copy()
    eng = Engine(k, 4, 3, 120.0, a, b)
    try:
        eng.index_build(codes)

        def others():
            return eng.pssm_scan(S, t), eng.query_codes(qcodes, 45.0), eng.query_topk(qcodes, 5, R=45.0, codes=True)

        before = others()
        got = eng.pssm_topk(S, topk, want_thresholds=True)
        ref.same_rows(got, ref.rows_from_scores(sc, topk))
        after = others()
        for x, y in zip(before, after):
            assert sorted(x) == sorted(y)
            for f in x:
                assert np.array_equal(x[f], y[f]), f
        assert len(before[0]["m"]) >= 17 * 40 and len(before[1]["q"]) >= 40
        hits = eng.pssm_scan(S, got["t_used"])
        ref.same_rows(capi.pssm_topk_hits(hits["m"], hits["id"], hits["score"], 17, topk), got, "scan at t_used")
        ref.same_rows(eng.pssm_topk(S, topk), got, "again")
    finally:
        eng.close()
