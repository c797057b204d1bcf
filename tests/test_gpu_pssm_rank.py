"""hs_pssm_rank on the GPU against the numpy contract of tests/pssm_rank_ref.py, bit for bit: t_rank, cnt_ge and cnt_gt
at every rank class, the scan at t_rank returning cnt_ge; sample sizes, the filter, batches, a forced split, a loaded
index, device pointers and a changed index, none of which may show; the ladder's retries on a planted sample; the
select's segment edges and every digit of its key; refusals; the handle's other calls around a call; and the
refinement loop with the threshold rule."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import pssm_rank_ref as ref
from tests import pssm_ref

pytestmark = pytest.mark.gpu

# (k, alphabet, n): four MFMA steps; ties at every rank; the NS = 0 filter path (19 steps)
SHAPES = [(25, 20, 5000), (3, 4, 200), (75, 32, 300)]
NM = 33
DEFAULT_SAMPLE = 262144  # HS_OPT_PSSM_RANK_SAMPLE as a handle starts


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
    """codes [n][k], the 33-profile mix of test_gpu_pssm_topk.py and its scores (computed once per shape)."""
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


def _mixed_ranks(n, nm=NM):
    return np.random.default_rng(n).integers(1, n + 1, size=nm).astype(np.uint64)


def _check(eng, case, rank, sample, nm=NM, what=""):
    """One call against the reference: the three outputs, the diagnostics and the profile's fields."""
    sc, S = case["sc"][:nm], case["S"][:nm]
    n = sc.shape[1]
    got = eng.pssm_rank(S, rank, want_diagnostics=True)
    ref.same(got, ref.from_scores(sc, rank), what)
    lad = ref.ladder(sc, rank, sample)
    assert np.array_equal(got["t_scan"].view(np.uint64), lad["t_scan"].view(np.uint64)), what
    assert np.array_equal(got["rounds"], lad["rounds"]), (what, got["rounds"], lad["rounds"])
    p = eng.profile()
    assert p["pssm_rank_sample"] == min(n, sample) and p["pssm_rank_retries"] == lad["retries"], what
    return got, lad, p


@pytest.mark.parametrize("nm", [1, 17, 33])
@pytest.mark.parametrize("k,A,n", SHAPES)
def test_outputs_equal_contract(k, A, n, nm):
    case = _case(k, A, n)
    eng = _engine(k, A, case["codes"])
    try:
        for rank in (1, 2, 64, 65, 100, n - 1, n, _mixed_ranks(n, nm)):
            got, lad, p = _check(eng, case, rank, DEFAULT_SAMPLE, nm=nm, what=(k, A, n, nm, rank))
            r = ref.ranks(rank, nm)
            assert np.all(got["cnt_gt"] < r) and np.all(r <= got["cnt_ge"])
            # n <= the sample: the sample is the index, one round at the answer itself
            assert np.array_equal(got["t_scan"].view(np.uint64), got["t"].view(np.uint64)) and not got["rounds"].any()
            assert p["hits"] == int(got["cnt_ge"].sum())
            if np.ndim(rank) or rank in (1, 65, n):
                hits = eng.pssm_scan(case["S"][:nm], got["t"])
                assert np.array_equal(hits["cnt"], got["cnt_ge"]), (k, A, n, nm, rank)
        if k == 3:   # ties fill every rank
            got = eng.pssm_rank(case["S"][:nm], n // 2)
            assert np.all(got["cnt_ge"] - got["cnt_gt"] > 1)
        e = eng.pssm_rank(np.zeros((0, k, A)), 1, want_diagnostics=True)     # nm = 0 is an empty, successful call
        assert all(len(e[f]) == 0 for f in ("t", "cnt_ge", "cnt_gt", "t_scan", "rounds"))
    finally:
        eng.close()


def test_sample_size_does_not_show():
    k, A, n = 25, 20, 5000
    case = _case(k, A, n)
    ranks = _mixed_ranks(n)
    ranks[:4] = (1, 64, 100, n)
    want = ref.from_scores(case["sc"], ranks)
    eng = _engine(k, A, case["codes"])
    try:
        for sample in (1, 64, 1000, n, 10 * n):
            eng.set_option("pssm_rank_sample", sample)
            got, lad, p = _check(eng, case, ranks, sample, what=sample)
            ref.same(got, want, sample)
            # the scans' fields are summed over every round
            assert p["pssm_pairs"] + p["pssm_dead"] * n == (1 + int(lad["rounds"].max())) * NM * n, sample
        with pytest.raises(HsError):
            eng.set_option("pssm_rank_sample", 0)
    finally:
        eng.close()


def test_filter_batches_and_splits_do_not_show(monkeypatch):
    k, A, n = 25, 20, 5000
    case = _case(k, A, n)
    ranks = _mixed_ranks(n)
    want = ref.from_scores(case["sc"], ranks)
    for options in ({"query_batch": 1}, {"query_batch": 16}, {"pssm_filter": 0},
                    {"query_batch": 16, "pssm_rank_sample": 64}):
        eng = _engine(k, A, case["codes"], options=options)
        try:
            got, _, p = _check(eng, case, ranks, options.get("pssm_rank_sample", DEFAULT_SAMPLE), what=options)
            ref.same(got, want, options)
            if "pssm_filter" in options:
                assert p["pssm_mfma_steps"] == 0 and p["pssm_survivors"] == NM * n
        finally:
            eng.close()
    # the library's TEST build reports a survivor overflow for every batch of more than 4 profiles
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "4")
    eng = _engine(k, A, case["codes"], hooks=True)
    try:
        got, _, p = _check(eng, case, ranks, DEFAULT_SAMPLE, what="split")
        ref.same(got, want, "split")
        assert p["verify_launches"] >= 9
    finally:
        eng.close()


def test_loaded_and_changed_index(tmp_path):
    k, A, n = 25, 20, 5000
    case = _case(k, A, n)
    ranks = np.minimum(_mixed_ranks(n), 3000)
    eng = _engine(k, A, case["codes"][:4000], options={"pssm_rank_sample": 1000})
    try:
        part = dict(codes=case["codes"][:4000], S=case["S"], sc=case["sc"][:, :4000])
        _check(eng, part, ranks, 1000, what="before")
        eng.index_append(case["codes"][4000:])
        _check(eng, case, ranks, 1000, what="appended")
        gone = np.arange(0, n, 7, dtype=np.uint32)
        eng.index_remove(gone)
        keep = np.setdiff1d(np.arange(n), gone)
        left = dict(codes=case["codes"][keep], S=case["S"], sc=np.ascontiguousarray(case["sc"][:, keep]))
        got, _, _ = _check(eng, left, ranks, 1000, what="removed")
        path = tmp_path / "r.idx"
        eng.index_save(path)
    finally:
        eng.close()
    eng2 = _engine(k, A, options={"pssm_rank_sample": 1000})
    try:
        eng2.index_load(path)
        got2, _, _ = _check(eng2, left, ranks, 1000, what="loaded")
        ref.same(got2, got, "loaded against live")
    finally:
        eng2.close()


def test_the_ladder_on_a_planted_sample():
    """Profile 0's best k-mer sits at every one of the 64 sampled positions and nowhere else: the sample proposes the
    maximum, which only 64 k-mers reach, so rank 65 takes two retries (r_s = 13, 49, then beyond the sample), rank 100
    one (18, then beyond) and rank 64 none."""
    k, A, n = 25, 20, 5000
    case = _case(k, A, n)
    codes = case["codes"].copy()
    codes[ref.sample_ids(n, 64)] = np.argmax(case["S"][0], axis=1).astype(np.uint8)
    sc = pssm_ref.scores(case["S"], codes)
    assert int((sc[0] >= sc[0].max()).sum()) == 64                   # the construction is what it says
    local = dict(codes=codes, S=case["S"], sc=sc)
    eng = _engine(k, A, codes, options={"pssm_rank_sample": 64})
    try:
        for rank, retries in ((65, 2), (100, 1), (64, 0)):
            got, lad, p = _check(eng, local, rank, 64, what=rank)
            assert got["rounds"][0] == retries == lad["rounds"][0], (rank, got["rounds"][0])
            if retries:
                assert got["t_scan"][0] == ref.ALL and got["cnt_ge"][0] >= rank
            else:
                assert got["t_scan"][0] == sc[0].max() == got["t"][0] and got["cnt_ge"][0] == 64
            assert p["pssm_rank_retries"] == int(got["rounds"].sum()) >= retries
    finally:
        eng.close()


def _distinct_kmers(n, k, A, seed):
    ids = np.random.default_rng(seed).choice(A ** k, size=n, replace=False)
    return np.stack([(ids // A ** p) % A for p in range(k)], axis=1).astype(np.uint8)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097, 70000])
def test_segment_edges_of_the_select(n):
    """A constant profile (every key equal: one bin takes the whole segment in every pass) and an all-distinct one, over
    segments inside one work item of the select, cut by one item edge (4097) and by many (70 000)."""
    k, A = 5, 20
    codes = _distinct_kmers(n, k, A, n)
    S = np.empty((2, k, A))
    S[0] = 1.25
    S[1] = (np.arange(A)[None, :] * float(A) ** np.arange(k)[:, None]) - 1000.0     # the k-mer's number, less 1000
    sc = pssm_ref.scores(S, codes)
    assert len(np.unique(sc[1])) == n
    case = dict(codes=codes, S=S, sc=sc)
    eng = _engine(k, A, codes)
    try:
        for rank in sorted({1, max(1, n // 2), n}):
            got, _, _ = _check(eng, case, rank, DEFAULT_SAMPLE, nm=2, what=(n, rank))
            assert got["cnt_ge"][0] == n and got["cnt_gt"][0] == 0 and got["t"][0] == 1.25 * k
            assert got["cnt_ge"][1] == rank and got["cnt_gt"][1] == rank - 1
        got, _, _ = _check(eng, case, np.array([n, 1], np.uint64), DEFAULT_SAMPLE, nm=2, what=(n, "mixed"))
        eng.set_option("pssm_rank_sample", 64)       # the segments of the sample's select, and a scan above the rank
        _check(eng, case, max(1, n // 2), 64, nm=2, what=(n, "sample 64"))
    finally:
        eng.close()


def test_sample_sub_batches_and_scan_batches_sized_by_the_hits():
    """More profiles than one sub-batch of the sample pass holds (2^24 / n_s = 239 at n_s = n = 70 000, 256 at n_s =
    2^16), so the pass and its select run at a profile offset above 0; and a largest rank of n, so the default scan
    batch, sized by the hits to expect (2^24 / n = 239 profiles), is smaller than the call."""
    k, A, n, nm = 5, 20, 70000, 260
    codes = _distinct_kmers(n, k, A, 11)
    rng = np.random.default_rng(12)
    S = rng.integers(-8, 9, size=(nm, k, A)) / 2.0
    sc = pssm_ref.scores(S, codes)
    case = dict(codes=codes, S=S, sc=sc)
    ranks = rng.integers(1, n + 1, size=nm).astype(np.uint64)
    ranks[[0, 238, 239, 255, 256, nm - 1]] = (n, 1, n, 7, n // 2, n)
    eng = _engine(k, A, codes)
    try:
        got, _, p = _check(eng, case, ranks, DEFAULT_SAMPLE, nm=nm, what="n_s = n")
        assert p["verify_launches"] >= 2 and not got["rounds"].any()
        eng.set_option("pssm_rank_sample", 65536)
        _check(eng, case, ranks, 65536, nm=nm, what="n_s = 2^16")
        eng.set_option("pssm_rank_sample", 64)       # a real ladder beside it: small ranks above the sample's grain
        _check(eng, case, np.minimum(ranks, 3000), 64, nm=nm, what="n_s = 64")
    finally:
        eng.close()


def test_more_profiles_than_one_batch_of_any_kind():
    """4100 profiles: two default scan batches (4096 + 4) and two sub-batches of the sample pass; and, with
    HS_OPT_QUERY_BATCH = 5000, one batch of more profiles than the LDS-binned count / scatter passes take (4096), which
    goes through the plain ones."""
    k, A, n, nm = 3, 4, 200, 4100
    case0 = _case(k, A, n)
    rng = np.random.default_rng(41)
    S = rng.integers(-1, 2, size=(nm, k, A)).astype(np.float64)
    case = dict(codes=case0["codes"], S=S, sc=pssm_ref.scores(S, case0["codes"]))
    ranks = rng.integers(1, n + 1, size=nm).astype(np.uint64)
    ranks[[0, 4095, 4096, nm - 1]] = (n, 1, n, 100)
    want = ref.from_scores(case["sc"], ranks)
    for options in ({}, {"query_batch": 5000}, {"query_batch": 5000, "pssm_rank_sample": 64}):
        eng = _engine(k, A, case["codes"], options=options)
        try:
            got, _, p = _check(eng, case, ranks, options.get("pssm_rank_sample", DEFAULT_SAMPLE), nm=nm, what=options)
            ref.same(got, want, options)
            if not options:
                assert p["verify_launches"] == 2
        finally:
            eng.close()


def test_every_digit_of_the_key():
    """Entries on three scales (multiples of 2^40, of 1, of 2^-12) over all 4096 6-mers of a 4-letter alphabet: the
    wanted key differs from its neighbours in a high byte, a middle byte or the lowest, and the ranks walk from the
    positive scores through +0.0 into the negative ones."""
    k, A = 6, 4
    n = A ** k
    codes = _distinct_kmers(n, k, A, 6)
    unit = np.array([0.0, 1.0, -1.0, 3.0])
    row = np.stack([unit * 2.0 ** 40, unit * 2.0 ** 40, unit, unit * 5.0, unit * 2.0 ** -12, unit * 2.0 ** -12])
    sc1 = pssm_ref.scores(row[None], codes)[0]
    zero_rank = int((sc1 > 0).sum()) + 1
    assert (sc1 > 0).any() and (sc1 < 0).any() and (sc1 == 0).any() and not np.signbit(sc1[sc1 == 0]).any()
    ranks = np.unique(np.concatenate([np.linspace(1, n, 60).astype(np.int64), [zero_rank - 1, zero_rank,
                                                                                 zero_rank + 1, 2, n - 1]]))
    nm = len(ranks)
    S = np.repeat(row[None], nm, axis=0)
    sc = np.repeat(sc1[None], nm, axis=0)
    case = dict(codes=codes, S=S, sc=sc)
    eng = _engine(k, A, codes)
    try:
        got, _, _ = _check(eng, case, ranks.astype(np.uint64), DEFAULT_SAMPLE, nm=nm)
        assert (got["t"] > 2.0 ** 39).any() and (got["t"] < -2.0 ** 39).any() and (got["t"] == 0).any()
        srt = -np.sort(-np.unique(sc1))
        gaps = np.abs(np.diff(srt))
        assert gaps.min() <= 2.0 ** -11 and gaps.max() >= 2.0 ** 39      # neighbours a low bit and a high byte apart
        eng.set_option("pssm_rank_sample", 512)
        _check(eng, case, ranks.astype(np.uint64), 512, nm=nm, what="sample 512")
    finally:
        eng.close()


def test_device_pointers_and_refusals():
    import torch
    k, A, n = 25, 20, 5000
    case = _case(k, A, n)
    ranks = _mixed_ranks(n)
    want = ref.from_scores(case["sc"], ranks)
    lad = ref.ladder(case["sc"], ranks, DEFAULT_SAMPLE)
    eng = _engine(k, A, case["codes"])
    try:
        dS = torch.from_numpy(case["S"]).cuda()
        dr = torch.from_numpy(ranks.astype(np.int64)).cuda()
        dt = torch.full((NM + 1,), 7.0, dtype=torch.float64, device="cuda")
        dge = torch.full((NM + 1,), 7, dtype=torch.int64, device="cuda")
        dgt = torch.full((NM + 1,), 7, dtype=torch.int64, device="cuda")
        dts = torch.full((NM + 1,), 7.0, dtype=torch.float64, device="cuda")
        dro = torch.full((NM + 1,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        eng.pssm_rank_dev(dS.data_ptr(), dr.data_ptr(), NM, dt.data_ptr(), dge.data_ptr(), dgt.data_ptr(),
                          dts.data_ptr(), dro.data_ptr())
        got = dict(t=dt[:NM].cpu().numpy(), cnt_ge=dge[:NM].cpu().numpy().astype(np.uint64),
                   cnt_gt=dgt[:NM].cpu().numpy().astype(np.uint64))
        ref.same(got, want, "dev")
        assert np.array_equal(dts[:NM].cpu().numpy().view(np.uint64), lad["t_scan"].view(np.uint64))
        assert np.array_equal(dro[:NM].cpu().numpy().astype(np.uint32), lad["rounds"])
        assert float(dt[NM]) == 7.0 and int(dge[NM]) == 7 and int(dgt[NM]) == 7 and float(dts[NM]) == 7.0 and int(dro[NM]) == 7
        # without the diagnostics
        dt.fill_(7.0)
        eng.pssm_rank_dev(dS.data_ptr(), dr.data_ptr(), NM, dt.data_ptr(), dge.data_ptr(), dgt.data_ptr())
        assert np.array_equal(dt[:NM].cpu().numpy().view(np.uint64), want["t"].view(np.uint64))
        # refusals found on the device, before anything is written
        dt.fill_(9.0), dge.fill_(9), dgt.fill_(9), dts.fill_(9.0), dro.fill_(9)

        def untouched():
            torch.cuda.synchronize()
            return (bool((dt == 9.0).all()) and bool((dge == 9).all()) and bool((dgt == 9).all())
                    and bool((dts == 9.0).all()) and bool((dro == 9).all()))

        def dev(S_=dS, r_=dr, nm=NM, t_=dt, ge_=dge, gt_=dgt):
            eng.pssm_rank_dev(S_.data_ptr(), r_.data_ptr() if r_ is not None else None, nm,
                              t_.data_ptr() if t_ is not None else None, ge_.data_ptr() if ge_ is not None else None,
                              gt_.data_ptr() if gt_ is not None else None, dts.data_ptr(), dro.data_ptr())

        for bad in (float("nan"), float("inf"), 2.0 ** 101):
            dS2 = dS.clone()
            dS2[20, 13, 7] = bad
            torch.cuda.synchronize()
            with pytest.raises(HsError) as e:
                dev(S_=dS2)
            assert e.value.status == capi.HS_ERR_INVALID and untouched()
        for bad in (0, n + 1):
            dr2 = dr.clone()
            dr2[32] = bad
            torch.cuda.synchronize()
            with pytest.raises(HsError) as e:
                dev(r_=dr2)
            assert e.value.status == capi.HS_ERR_INVALID and untouched()
        for kw in (dict(nm=1 << 27), dict(r_=None), dict(t_=None), dict(ge_=None), dict(gt_=None)):
            with pytest.raises(HsError) as e:
                dev(**kw)
            assert e.value.status == capi.HS_ERR_INVALID and untouched()
        # the host form
        lib, h, v = eng._lib, eng._h, capi._vp
        t, ge, gt = np.full(NM, 7.0), np.full(NM, 7, np.uint64), np.full(NM, 7, np.uint64)
        ts, ro = np.full(NM, 7.0), np.full(NM, 7, np.uint32)
        S2 = case["S"].copy()
        S2[1, 2, 3] = np.nan
        r0, r1 = ranks.copy(), ranks.copy()
        r0[5], r1[5] = 0, n + 1
        for Sx, rx, nm, outs in ((S2, ranks, NM, (t, ge, gt)), (case["S"], r0, NM, (t, ge, gt)),
                                 (case["S"], r1, NM, (t, ge, gt)), (case["S"], ranks, 1 << 27, (t, ge, gt)),
                                 (case["S"], None, NM, (t, ge, gt)), (case["S"], ranks, NM, (None, ge, gt)),
                                 (case["S"], ranks, NM, (t, None, gt)), (case["S"], ranks, NM, (t, ge, None)),
                                 (None, ranks, NM, (t, ge, gt))):
            st = lib.hs_pssm_rank(h, None if Sx is None else v(Sx), None if rx is None else v(rx), C.c_uint64(nm),
                                  *[None if o is None else v(o) for o in outs], v(ts), v(ro))
            assert st == capi.HS_ERR_INVALID
            assert np.all(t == 7.0) and np.all(ge == 7) and np.all(gt == 7) and np.all(ts == 7.0) and np.all(ro == 7)
    finally:
        eng.close()
    unbuilt = _engine(k, A)
    try:
        with pytest.raises(HsError) as e:
            unbuilt.pssm_rank(case["S"], 1)
        assert e.value.status == capi.HS_ERR_STATE
        # no sequence long enough: an empty index refuses every rank
        info, _ = unbuilt.index_build_windows(np.zeros(10, dtype=np.uint8), np.array([0, 4, 10], dtype=np.uint64))
        assert info["n"] == 0
        with pytest.raises(HsError) as e:
            unbuilt.pssm_rank(case["S"], 1)
        assert e.value.status == capi.HS_ERR_INVALID
        # ... on sentinel-filled outputs, in the host and the _dev form
        lib, h, v = unbuilt._lib, unbuilt._h, capi._vp
        ones = np.ones(NM, np.uint64)
        t, ge, gt = np.full(NM, 7.0), np.full(NM, 7, np.uint64), np.full(NM, 7, np.uint64)
        ts, ro = np.full(NM, 7.0), np.full(NM, 7, np.uint32)
        assert lib.hs_pssm_rank(h, v(case["S"]), v(ones), C.c_uint64(NM), v(t), v(ge), v(gt), v(ts), v(ro)) == capi.HS_ERR_INVALID
        assert np.all(t == 7.0) and np.all(ge == 7) and np.all(gt == 7) and np.all(ts == 7.0) and np.all(ro == 7)
        dS = torch.from_numpy(case["S"]).cuda()
        d1 = torch.ones(NM, dtype=torch.int64, device="cuda")
        dt = torch.full((NM,), 9.0, dtype=torch.float64, device="cuda")
        dge, dgt = (torch.full((NM,), 9, dtype=torch.int64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        with pytest.raises(HsError) as e:
            unbuilt.pssm_rank_dev(dS.data_ptr(), d1.data_ptr(), NM, dt.data_ptr(), dge.data_ptr(), dgt.data_ptr())
        torch.cuda.synchronize()
        assert e.value.status == capi.HS_ERR_INVALID
        assert bool((dt == 9.0).all()) and bool((dge == 9).all()) and bool((dgt == 9).all())
        assert len(unbuilt.pssm_rank(np.zeros((0, k, A)), 1)["t"]) == 0
    finally:
        unbuilt.close()


def test_other_calls_around_a_call():
    """hs_pssm_scan, hs_pssm_topk and hs_query_codes on the same handle give what they gave, before and after."""
    k = 25
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
            return eng.pssm_scan(S, t), eng.pssm_topk(S, 10, want_thresholds=True), eng.query_codes(qcodes, 45.0)

        before = others()
        got = eng.pssm_rank(S, 40)
        ref.same(got, ref.from_scores(sc, 40))
        assert np.array_equal(got["t"], t)
        after = others()
        for x, y in zip(before, after):
            assert sorted(x) == sorted(y)
            for f in x:
                assert np.array_equal(x[f], y[f]), f
        assert len(before[0]["m"]) >= 17 * 40 and len(before[2]["q"]) >= 40
        ref.same(eng.pssm_rank(S, 40), got, "again")
    finally:
        eng.close()


def _same_loop(got, want, what):
    assert got["iters"] == want["iters"] and got["converged"] == want["converged"], (what, got["iters"], want["iters"])
    assert np.array_equal(got["S"].view(np.uint64), want["S"].view(np.uint64)), what
    assert np.array_equal(got["t"].view(np.uint64), want["t"].view(np.uint64)), what
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["used"], want["used"]), what
    assert got["counts"].dtype == np.uint32 and got["used"].dtype == np.uint64


@pytest.mark.parametrize("per_protein", [False, True])
def test_refine_rank_equals_the_reference_loop(per_protein):
    from tests.test_gpu_pssm_counts import A as FA, K as FK, planted
    fam = planted()
    codes = fam["codes"]
    ids = fam["id_start"] if per_protein else None
    eng = _engine(FK, FA)
    try:
        info, _ = eng.index_build_windows(fam["residues"], fam["seq_start"])
        assert info["n"] == len(codes)
        # converges inside n_iter = 8: the hit count is held at 30 k-mers (and their ties) while the matrix moves
        want = ref.refine(codes, FA, fam["loose"], 30, 8, ids)
        assert want["converged"] and 2 <= want["iters"] < 8
        got = eng.pssm_refine_rank(fam["loose"], 30, 8, ids)
        _same_loop(got, want, "converges")
        again = eng.pssm_hit_counts(got["S"], got["t"], ids)    # converged: the counts of (S_out, t_out) are the counts
        assert np.array_equal(again["counts"], got["counts"]) and np.array_equal(again["used"], got["used"])
        if not per_protein:
            assert np.all(got["used"] >= 30)
        # does not converge within n_iter = 3; a rank per profile
        ranks = np.array([20, 25, 10], np.uint64)
        want = ref.refine(codes, FA, fam["strict"], ranks, 3, ids)
        assert not want["converged"] and want["iters"] == 3
        assert not np.array_equal(want["history"][1], want["history"][2])
        _same_loop(eng.pssm_refine_rank(fam["strict"], ranks, 3, ids), want, "does not converge")
        _same_loop(eng.pssm_refine_rank(fam["strict"], ranks, 1, ids), ref.refine(codes, FA, fam["strict"], ranks, 1, ids),
                   "one")
        bg = np.linspace(1.0, 2.0, FA) / np.linspace(1.0, 2.0, FA).sum()
        want = ref.refine(codes, FA, fam["strict"], 20, 4, ids, bg=bg, pseudo=0.5)
        _same_loop(eng.pssm_refine_rank(fam["strict"], 20, 4, ids, background=bg, pseudo=0.5), want, "bg")
        # refusals: nothing is written
        S_out, t_out = np.full(fam["loose"].shape, 7.0), np.full(3, 7.0)
        it, cv = C.c_uint32(5), C.c_uint32(5)
        for rk, n_iter in ((np.array([0, 1, 1], np.uint64), 2), (np.array([1, 1, len(codes) + 1], np.uint64), 2),
                           (ranks, 0), (ranks, 101)):
            st = eng._lib.hs_pssm_refine_rank(eng._h, capi._vp(fam["loose"]), capi._vp(rk), 3, None, 0, None, 1.0,
                                              n_iter, capi._vp(S_out), capi._vp(t_out), None, None, C.byref(it),
                                              C.byref(cv))
            assert st == capi.HS_ERR_INVALID and np.all(S_out == 7.0) and np.all(t_out == 7.0)
    finally:
        eng.close()
