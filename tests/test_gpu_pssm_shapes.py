"""The profile scan's device path at every MFMA step count and at alphabets whose positions straddle lane chunks and
steps (tests/pssm_cases.py: SHAPES), against the numpy contract of tests/pssm_ref.py and the survivor count the host
tables predict -- all five instantiations of hs_pssm_filter_kernel, five profile tiles (a full LDS stage of four and
a stage of one); probe profiles that test the depth axis element by element; the profile families of
tests/test_pssm_cpu.py through the DEVICE's table build, as they are and across a step boundary; and the calls
downstream of the scan at shapes their kernels have not seen.  Every comparison is for equality.
tests/test_pssm_shapes_cpu.py proves the premises on the host."""
import numpy as np
import pytest

from hsearch_amd import capi
from tests import pssm_cases, pssm_counts_ref, pssm_rank_ref, pssm_ref, pssm_seq_ref, pssm_topk_ref
from tests.pssm_cases import ALL64, N, NMS, SHAPES

pytestmark = pytest.mark.gpu

IDS = ["%d-%d" % s for s in SHAPES]
DEFAULT_SAMPLE = 262144   # HS_OPT_PSSM_TOPK_SAMPLE and HS_OPT_PSSM_RANK_SAMPLE as a handle starts


def _same(got, want, what):
    assert np.array_equal(got["m"], want["m"]), what
    assert np.array_equal(got["id"], want["id"]), what
    assert np.array_equal(got["score"].view(np.uint64), want["score"].view(np.uint64)), what
    if "cnt" in got:
        assert np.array_equal(got["cnt"], want["cnt"]), what


def _first_profile_off(eng, S, t, surv):
    """For a failure's message only: the profiles scanned one by one, the first whose survivor count is not surv[m]."""
    for m in range(len(S)):
        eng.pssm_scan(S[m:m + 1], t[m:m + 1])
        p = eng.profile()
        if p["pssm_survivors"] != int(surv[m]):
            return "profile %d alone: %d survivors, the host tables predict %d" % (m, p["pssm_survivors"], int(surv[m]))
    return "every profile alone has the predicted survivors"


@pytest.mark.parametrize("k,A", SHAPES, ids=IDS)
def test_every_step_count_and_alphabet(k, A):
    case = pssm_cases.mixed_case(k, A, N)
    steps = pssm_cases.steps(k, A)
    eng = pssm_cases.engine(k, A, case["codes"])
    try:
        for nm in NMS:
            want = pssm_cases.want(case, nm)
            S, t = case["S"][:nm], case["t"][:nm]
            _same(eng.pssm_scan(S, t), want, (k, A, nm))
            p = eng.profile()
            dead, surv = int(case["dead"][:nm].sum()), int(case["surv"][:nm].sum())
            assert p["pssm_dead"] == dead and p["pssm_pairs"] == (nm - dead) * N, (k, A, nm)
            assert p["pssm_mfma_steps"] == steps and p["hits"] == len(want["m"]), (k, A, nm)
            if p["pssm_survivors"] != surv:
                pytest.fail("(%d, %d) nm %d: %d survivors, the host tables predict %d; %s" % (
                    k, A, nm, p["pssm_survivors"], surv, _first_profile_off(eng, S, t, case["surv"])))
        eng.set_option("query_batch", 16)
        _same(eng.pssm_scan(case["S"], case["t"]), pssm_cases.want(case, 65), (k, A, "batches of 16"))
        p = eng.profile()
        assert p["pssm_survivors"] == int(case["surv"].sum()) and p["pssm_dead"] == int(case["dead"].sum()), (k, A)
        eng.set_option("query_batch", 0)
        eng.set_option("pssm_filter", 0)
        for nm in (1, 65):
            _same(eng.pssm_scan(case["S"][:nm], case["t"][:nm]), pssm_cases.want(case, nm), (k, A, nm, "no filter"))
            p = eng.profile()
            assert p["pssm_survivors"] == nm * N and p["pssm_dead"] == 0 and p["pssm_mfma_steps"] == 0
    finally:
        eng.close()
    one = pssm_cases.mixed_case(k, A, 1)
    eng = pssm_cases.engine(k, A, one["codes"])
    try:
        for nm in NMS:
            _same(eng.pssm_scan(one["S"][:nm], one["t"][:nm]), pssm_cases.want(one, nm), (k, A, nm, "n = 1"))
            assert eng.profile()["pssm_survivors"] == int(one["surv"][:nm].sum()), (k, A, nm, "n = 1")
    finally:
        eng.close()


@pytest.mark.parametrize("k,A", SHAPES, ids=IDS)
def test_every_depth_element(k, A):
    """Profile e = p * A + a (1.0 there, 0.0 elsewhere, t = 1) is hit by the k-mers with x_p == a and by no other, and
    its host tables pass exactly those: a one-hot element or a profile code that sits anywhere but at depth e loses
    hits or lets k-mers through that are none."""
    S, t = pssm_cases.probe_profiles(k, A)
    codes = pssm_cases.probe_codes(k, A)
    want = pssm_ref.scan(S, t, codes)
    have = (codes[:, :, None] == np.arange(A)[None, None, :]).sum(axis=0).reshape(k * A).astype(np.uint64)
    assert np.array_equal(want["cnt"], have) and len(want["m"]) == k * N
    eng = pssm_cases.engine(k, A, codes)
    try:
        got = eng.pssm_scan(S, t)
        p = eng.profile()
        off = np.flatnonzero(got["cnt"] != have)
        if len(off):
            e = int(off[0])
            pytest.fail("(%d, %d): element %d (position %d, residue %d) has %d hits, %d k-mers carry it; %d elements "
                        "differ" % (k, A, e, e // A, e % A, int(got["cnt"][e]), int(have[e]), len(off)))
        _same(got, want, (k, A))
        assert p["pssm_dead"] == 0 and p["pssm_pairs"] == k * A * N and p["pssm_mfma_steps"] == pssm_cases.steps(k, A)
        if p["pssm_survivors"] != len(want["m"]):
            pytest.fail("(%d, %d): %d survivors of %d hits: the filter is exact for the probes on the host tables; %s"
                        % (k, A, p["pssm_survivors"], len(want["m"]), _first_profile_off(eng, S, t, have)))
    finally:
        eng.close()


def _scan_dev(eng, S, t, cap):
    import torch
    nm = len(S)
    dS, dt = torch.from_numpy(np.ascontiguousarray(S)).cuda(), torch.from_numpy(np.ascontiguousarray(t)).cuda()
    dm = torch.full((cap,), 7, dtype=torch.int32, device="cuda")
    did = torch.full((cap,), 7, dtype=torch.int32, device="cuda")
    ds = torch.full((cap,), 7.0, dtype=torch.float64, device="cuda")
    dc = torch.full((nm,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nh = eng.pssm_scan_dev(dS.data_ptr(), dt.data_ptr(), nm, dm.data_ptr(), did.data_ptr(), ds.data_ptr(), cap,
                           dc.data_ptr())
    assert nh <= cap
    return dict(m=dm[:nh].cpu().numpy().astype(np.uint32), id=did[:nh].cpu().numpy().astype(np.uint32),
                score=ds[:nh].cpu().numpy(), cnt=dc.cpu().numpy().astype(np.uint64))


def test_profile_families_on_the_device():
    """The families whose tables tests/test_pssm_cpu.py proves on the host -- scales 2^-20 .. 2^30, constant, zero,
    subnormal and 2^100 entries, thresholds outside the range and up to 1.7e308, the cancellation family whose
    rounded sum hits where the real sum does not -- through the device's own table build (hs_pssm_prep_kernel,
    hs_pssm_prep_tiles_kernel): over all 64 3-mers of 4 residues, and at positions 11 .. 13 of a 25-mer over 20
    residues, where the profile lies on both sides of an MFMA step boundary."""
    forms = (("k = 3", 3, 4, ALL64, lambda S: S), ("embedded", pssm_cases.EMBED_K, pssm_cases.EMBED_A,
                                                   pssm_cases.embedded_codes(), pssm_cases.embed))
    for form, k, A, codes, place in forms:
        eng = pssm_cases.engine(k, A, codes)
        try:
            for name, family in pssm_cases.FAMILIES.items():
                S3, t = family()
                S = place(S3)
                nm, what = len(S), (form, name)
                want = pssm_ref.scan(S, t, codes)
                pred = pssm_cases.predict(S, t, codes)
                dead, surv = int(pred["dead"].sum()), int(pred["surv"].sum())
                assert surv >= len(want["m"]), what
                for how in ("host pointers", "device pointers"):
                    got = eng.pssm_scan(S, t) if how == "host pointers" else _scan_dev(eng, S, t, len(want["m"]) + 5)
                    _same(got, want, what + (how,))
                    p = eng.profile()
                    assert p["pssm_dead"] == dead and p["pssm_pairs"] == (nm - dead) * 64, what + (how,)
                    if p["pssm_survivors"] != surv:
                        pytest.fail("%s, %s, %s: %d survivors, the host tables predict %d; %s" % (
                            form, name, how, p["pssm_survivors"], surv, _first_profile_off(eng, S, t, pred["surv"])))
                if name == "cancellation":   # the family does what it is here for, on the device as well
                    assert len(want["m"]) > 0 and (np.abs(want["score"]) <= 1.0).any(), what
        finally:
            eng.close()


def _predicted_survivors(S, t, codes):
    pred = pssm_cases.predict(S, t, codes)
    return int(pred["surv"].sum()), int(pred["dead"].sum())


@pytest.mark.parametrize("filt", [1, 0], ids=["filter", "no-filter"])
@pytest.mark.parametrize("k,A", [(13, 20), (17, 29)], ids=["13-20", "17-29"])
def test_downstream_calls_at_unrun_shapes(k, A, filt):
    """hs_pssm_topk, hs_pssm_rank, hs_pssm_seq_scan and hs_pssm_hit_counts have kernels of their own sized by k *
    alphabet (the profile in LDS, per-wave [k][alphabet] histograms), run so far at alphabets 4, 20 and 32 only: each
    against its own reference with the assertions of its own test file, at 3 and 4 MFMA steps and an odd alphabet."""
    nm = 17
    case = pssm_cases.mixed_case(k, A, N)
    codes, S, t, sc = case["codes"], case["S"][:nm], case["t"][:nm], case["sc"][:nm]
    hits = pssm_cases.want(case, nm)
    steps = pssm_cases.steps(k, A) if filt else 0
    eng = pssm_cases.engine(k, A, codes, options={"pssm_filter": filt})
    try:
        # hs_pssm_topk (tests/test_gpu_pssm_topk.py: _check and test_rows_equal_contract)
        for topk in (1, 10, 64):
            got = eng.pssm_topk(S, topk, want_thresholds=True)
            pssm_topk_ref.same_rows(got, pssm_topk_ref.rows_from_scores(sc, topk), (k, A, topk))
            tu = pssm_topk_ref.t_used_from_scores(sc, topk, DEFAULT_SAMPLE)
            assert np.array_equal(got["t_used"].view(np.uint64), tu.view(np.uint64)), (k, A, topk)
            p = eng.profile()
            assert p["pssm_topk_sample"] == N and p["pssm_topk_raised"] == nm and np.all(got["count"] == topk)
            assert p["pssm_mfma_steps"] == steps and p["hits"] == int((sc >= tu[:, None]).sum())
            if filt:
                surv, dead = _predicted_survivors(S, tu, codes)
                assert dead == 0 and p["pssm_dead"] == 0 and p["pssm_pairs"] == nm * N
                assert p["pssm_survivors"] == surv, (k, A, topk)
            else:
                assert p["pssm_survivors"] == nm * N
        # hs_pssm_rank (tests/test_gpu_pssm_rank.py: _check and test_outputs_equal_contract)
        mixed = np.random.default_rng(N).integers(1, N + 1, size=nm).astype(np.uint64)
        for rank in (1, 2, 64, 65, N - 1, N, mixed):
            got = eng.pssm_rank(S, rank, want_diagnostics=True)
            pssm_rank_ref.same(got, pssm_rank_ref.from_scores(sc, rank), (k, A, rank))
            lad = pssm_rank_ref.ladder(sc, rank, DEFAULT_SAMPLE)
            assert np.array_equal(got["t_scan"].view(np.uint64), lad["t_scan"].view(np.uint64)), (k, A, rank)
            assert np.array_equal(got["rounds"], lad["rounds"]), (k, A, rank)
            p = eng.profile()
            assert p["pssm_rank_sample"] == N and p["pssm_rank_retries"] == lad["retries"] == 0
            r = pssm_rank_ref.ranks(rank, nm)
            assert np.all(got["cnt_gt"] < r) and np.all(r <= got["cnt_ge"])
            assert np.array_equal(got["t_scan"].view(np.uint64), got["t"].view(np.uint64))
            assert p["hits"] == int(got["cnt_ge"].sum())
            listed = eng.pssm_scan(S, got["t"])
            assert np.array_equal(listed["cnt"], got["cnt_ge"]), (k, A, rank)
        # hs_pssm_seq_scan over a plain index (tests/test_gpu_pssm_seq.py: test_rows_equal_the_rule and
        # test_deep_search_one_sequence_and_a_plain_index): empty sequences, short and long ones, one, one per id
        cuts = np.sort(np.random.default_rng(k * A).integers(0, N + 1, size=40))
        cuts[[3, 4]] = cuts[5]
        some = np.concatenate([[0], cuts, [N]]).astype(np.uint64)
        for ids in (some, np.array([0, N], np.uint64), np.arange(N + 1, dtype=np.uint64)):
            want = pssm_seq_ref.rows(hits, nm, ids)
            got = eng.pssm_seq_scan(S, t, ids)
            pssm_seq_ref.same_rows(got, want, (k, A, len(ids)))
            p = eng.profile()
            assert p["pssm_seq_rows"] == len(want["m"]) and p["hits"] == want["n_hits"] == len(hits["m"])
            assert p["pssm_dead"] == (int(case["dead"][:nm].sum()) if filt else 0)
            assert p["pssm_survivors"] == (int(case["surv"][:nm].sum()) if filt else nm * N)
            pssm_seq_ref.same_rows(capi.pssm_seq_hits(hits["m"], hits["id"], hits["score"], nm, ids), got, "list")
        # hs_pssm_hit_counts, every site and one per protein (tests/test_gpu_pssm_counts.py:
        # test_counts_equal_the_rule and test_shapes)
        for ids in (None, some):
            want = pssm_counts_ref.from_hits(codes, A, hits, nm, ids)
            assert want["used"][7] > 0 and want["used"][5] == 0
            for chunk in (0, 7):
                eng.set_option("pssm_count_chunk", chunk)
                got = eng.pssm_hit_counts(S, t, ids)
                pssm_counts_ref.same_counts(got, want, (k, A, ids is None, chunk))
                p = eng.profile()
                assert p["pssm_count_sites"] == int(want["used"].sum()) and p["hits"] == want["n_hits"]
                assert p["pssm_count_items"] >= int((want["used"] > 0).sum())
                assert p["pssm_survivors"] == (int(case["surv"][:nm].sum()) if filt else nm * N)
            host = capi.pssm_count_hits(codes, A, hits["m"], hits["id"], hits["score"], nm, ids)
            assert np.array_equal(host["counts"], got["counts"]) and np.array_equal(host["used"], got["used"])
            if ids is None:
                assert np.array_equal(got["used"], hits["cnt"])
            else:
                assert np.array_equal(got["used"], pssm_seq_ref.rows(hits, nm, ids)["seq_cnt"])
    finally:
        eng.close()
