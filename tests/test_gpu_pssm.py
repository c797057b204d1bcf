"""hs_pssm_scan on the GPU against the numpy contract of tests/pssm_ref.py: hits, order, scores bit for bit and counts,
with the MFMA filter and without it; the filter's survivor count against the count predicted from the host tables
(which is what proves the one-hot operand and the lane order: a wrong one would only pass more, or lose a rare hit);
dead profiles, the capacity protocol, a forced survivor split, windows and loaded indexes, device pointers, refusals,
and the handle's other calls around a scan."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import pssm_ref

pytestmark = pytest.mark.gpu

# (k, alphabet): 4 steps with a ragged last one; one position; exactly one step; two packed words; the longest
# k-mers (12 steps); the deepest rows there are (19 steps)
SHAPES = [(25, 20), (1, 20), (4, 32), (26, 20), (75, 20), (75, 32)]
NS = [1, 15, 16, 17, 63, 64, 65, 4097]
NMS = [1, 15, 16, 17, 33]


def _coords(A):
    if A == 20:
        return None
    rng = np.random.default_rng(77)
    return np.ascontiguousarray(np.concatenate([synth.coords(), rng.normal(0, 3, size=(A - 20, 8))]))


def _engine(k, A, codes=None, hooks=False, options=None):
    a, b = synth.make_planes(k, 2, 1, 200.0, seed=3)
    eng = Engine(k, 2, 1, 200.0, a, b, coords=_coords(A), hooks=hooks, options=options)
    if codes is not None:
        eng.index_build(codes)
    return eng


_CASES = {}


def _case(k, A, n):
    """codes [n][k], 33 profiles and thresholds, the reference scan of all 33 and the predicted survivors per profile
    (computed once per shape and size)."""
    key = (k, A, n)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * k + 10 * A + n)
        codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
        S = rng.normal(0, 2, size=(33, k, A))
        S[::2] = rng.integers(-16, 17, size=S[::2].shape) / 4.0      # dyadic entries: equal scores are common
        S[3, :, 0] = -1e30                                           # a forbidden residue
        sc = pssm_ref.scores(S, codes)
        # an attained score as the threshold: the tie is a hit.  About a twentieth of the k-mers hit.
        t = np.sort(sc, axis=1)[:, -max(1, n // 20)].copy()
        t[5] = sc[5].max() + 1e3                                     # dead
        t[7] = -1e6                                                  # everything hits
        t[9] = sc[9].max()
        T = capi.pssm_tables(S, t)
        F = pssm_ref.filter_values(T["code"], codes)
        surv = ((F >= T["tau"][:, None]) & (T["dead"] == 0)[:, None]).sum(axis=1)
        assert T["dead"][5] == 1 and surv[7] == n
        _CASES[key] = dict(codes=codes, S=S, t=t, sc=sc, dead=T["dead"], surv=surv)
    return _CASES[key]


def _want(case, nm):
    hit = case["sc"][:nm] >= case["t"][:nm, None]
    m, i = np.nonzero(hit)
    return dict(m=m.astype(np.uint32), id=i.astype(np.uint32), score=case["sc"][m, i], cnt=hit.sum(axis=1).astype(np.uint64))


def _same(got, want, what):
    assert np.array_equal(got["m"], want["m"]), what
    assert np.array_equal(got["id"], want["id"]), what
    assert np.array_equal(got["score"].view(np.uint64), want["score"].view(np.uint64)), what
    if "cnt" in got:
        assert np.array_equal(got["cnt"], want["cnt"]), what


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k,A", SHAPES)
def test_scan_equals_contract(k, A, n):
    case = _case(k, A, n)
    eng = _engine(k, A, case["codes"])
    steps = -(-k * A // 128)
    try:
        for nm in NMS:
            want = _want(case, nm)
            got = eng.pssm_scan(case["S"][:nm], case["t"][:nm])
            _same(got, want, (k, A, n, nm))
            p = eng.profile()
            dead = int(case["dead"][:nm].sum())
            assert p["pssm_dead"] == dead and p["pssm_pairs"] == (nm - dead) * n
            assert p["pssm_survivors"] == int(case["surv"][:nm].sum()), (k, A, n, nm)
            assert p["pssm_mfma_steps"] == steps and p["hits"] == len(want["m"])
        assert len(want["m"]) >= 2
        if n >= 63:   # the filter is no pass-through on these inputs
            assert len(want["m"]) <= int(case["surv"].sum()) < 33 * n // 2
        eng.set_option("pssm_filter", 0)
        for nm in (1, 33):
            got = eng.pssm_scan(case["S"][:nm], case["t"][:nm])
            _same(got, _want(case, nm), (k, A, n, nm, "no filter"))
            p = eng.profile()
            assert p["pssm_survivors"] == nm * n and p["pssm_dead"] == 0 and p["pssm_mfma_steps"] == 0
    finally:
        eng.close()


@pytest.mark.parametrize("k,A", [(25, 20), (6, 20), (75, 20)])
@pytest.mark.parametrize("nm", [64, 65, 130])
def test_many_profile_tiles(k, A, nm):
    """More profile tiles than the filter kernel stages in LDS at once (4 with resident operands): whole stages, a
    ragged last stage, and a single tile behind full ones."""
    n = 1000
    rng = np.random.default_rng(nm * 100 + k)
    codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
    S = rng.integers(-16, 17, size=(nm, k, A)) / 4.0
    t = np.sort(pssm_ref.scores(S, codes), axis=1)[:, -25].copy()
    want = pssm_ref.scan(S, t, codes)
    T = capi.pssm_tables(S, t)
    surv = int((pssm_ref.filter_values(T["code"], codes) >= T["tau"][:, None]).sum())
    eng = _engine(k, A, codes)
    try:
        _same(eng.pssm_scan(S, t), want, (k, A, nm))
        assert eng.profile()["pssm_survivors"] == surv and len(want["m"]) >= 25 * nm
    finally:
        eng.close()


def test_ties_are_hits():
    case = _case(25, 20, 4097)
    want = _want(case, 33)
    on_t = want["score"] == case["t"][want["m"]]
    assert on_t.sum() >= 20   # every profile but the dead and the pass-all one has its threshold attained


def test_batches_do_not_show():
    case = _case(25, 20, 4097)
    want = _want(case, 33)
    for batch in (1, 16, 20):
        eng = _engine(25, 20, case["codes"], options={"query_batch": batch})
        try:
            _same(eng.pssm_scan(case["S"], case["t"]), want, batch)
            assert eng.profile()["pssm_survivors"] == int(case["surv"].sum())
        finally:
            eng.close()


def _all_hit():
    n, nm, k, A = 4097, 17, 25, 20
    rng = np.random.default_rng(5)
    codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
    S = rng.integers(-8, 9, size=(nm, k, A)) / 2.0
    t = pssm_ref.scores(S, codes).min(axis=1)   # the weakest k-mer's score: every k-mer hits
    return codes, S, t, pssm_ref.scan(S, t, codes)


def test_every_kmer_hits_capacity_protocol():
    codes, S, t, want = _all_hit()
    assert len(want["m"]) == 4097 * 17
    eng = _engine(25, 20, codes)
    try:
        lib, h = eng._lib, eng._h
        cap = 1000
        hm, hid = np.full(cap, 7, np.uint32), np.full(cap, 7, np.uint32)
        hs = np.full(cap, 7.0)
        cnt = np.zeros(17, np.uint64)
        n = C.c_uint64(0)
        st = lib.hs_pssm_scan(h, capi._vp(S), capi._vp(t), 17, capi._vp(hm), capi._vp(hid), capi._vp(hs), cap,
                              C.byref(n), capi._vp(cnt))
        assert st == capi.HS_ERR_CAPACITY and n.value == 4097 * 17
        assert np.all(cnt == 4097) and np.all(hm == 7) and np.all(hs == 7.0)
        st = lib.hs_pssm_scan(h, capi._vp(S), capi._vp(t), 17, None, None, None, 0, C.byref(n), None)
        assert st == capi.HS_ERR_CAPACITY and n.value == 4097 * 17
        _same(eng.pssm_scan(S, t), want, "all hit")
        eng.set_option("pssm_filter", 0)
        _same(eng.pssm_scan(S, t, cap=4097 * 17), want, "all hit, no filter")
    finally:
        eng.close()


def test_every_kmer_hits_forced_split(monkeypatch):
    """The library's TEST build reports a survivor-counter overflow for every batch of more than 4 profiles: the
    scan halves its batches down to 4 and nothing shows."""
    codes, S, t, want = _all_hit()
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "4")
    eng = _engine(25, 20, codes, hooks=True)
    try:
        _same(eng.pssm_scan(S, t), want, "split")
        p = eng.profile()
        assert p["verify_launches"] >= 5 and p["pssm_pairs"] == 17 * 4097 and p["pssm_survivors"] == 17 * 4097
    finally:
        eng.close()


def test_windows_index_and_loaded_index(tmp_path):
    k, A = 25, 20
    rng = np.random.default_rng(9)
    lens = [40, 3, 25, 300, 24, 77]
    residues = rng.integers(0, A, size=sum(lens)).astype(np.uint8)
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    eng = _engine(k, A)
    try:
        info, pos = eng.index_build_windows(residues, seq_start)
        codes = np.stack([residues[p:p + k] for p in pos])
        assert len(codes) == sum(max(0, l - k + 1) for l in lens)
        S = rng.integers(-12, 13, size=(5, k, A)) / 4.0
        t = np.sort(pssm_ref.scores(S, codes), axis=1)[:, -10].copy()
        want = pssm_ref.scan(S, t, codes)
        _same(eng.pssm_scan(S, t), want, "windows")
        path = tmp_path / "w.idx"
        eng.index_save(path)
    finally:
        eng.close()
    eng2 = _engine(k, A)
    try:
        eng2.index_load(path)
        _same(eng2.pssm_scan(S, t), want, "loaded")
    finally:
        eng2.close()


def test_euclidean_profiles_equal_bruteforce():
    """S[p][a] = -|coords[a] - c_p|^2, t = -R^2: the scan's hits are the brute-force search's, as SETS -- R^2 sits in
    a gap of the sorted d2 values wider than 10^-6 relative, so the two summation orders cannot disagree."""
    k, n, nq = 25, 4097, 12
    codes = synth.make_db(n, k, seed=21)
    centers, _ = synth.make_queries(codes, nq, max_subst=3, seed=22, jitter=0.05)
    x = synth.embed(codes)
    d2 = np.sort(((x[None, :, :] - centers[:, None, :]) ** 2).sum(axis=2).ravel())
    lo = np.searchsorted(d2, 60.0 ** 2)
    gaps = (d2[lo + 1:lo + 4000] - d2[lo:lo + 3999]) / d2[lo:lo + 3999]
    g = int(np.argmax(gaps > 1e-5))
    assert gaps[g] > 1e-5
    R2 = 0.5 * (d2[lo + g] + d2[lo + g + 1])
    eng = _engine(k, 20, codes)
    try:
        bf = eng.bruteforce(centers, float(np.sqrt(R2)))
        S = pssm_ref.euclid_profiles(centers, synth.coords())
        got = eng.pssm_scan(S, np.full(nq, -R2))
        assert len(bf["q"]) == lo + g + 1 and len(bf["q"]) >= nq
        assert set(zip(bf["q"].tolist(), bf["id"].tolist())) == set(zip(got["m"].tolist(), got["id"].tolist()))
    finally:
        eng.close()


def test_device_pointers_and_refusals():
    import torch
    case = _case(25, 20, 4097)
    want = _want(case, 33)
    eng = _engine(25, 20, case["codes"])
    try:
        dS = torch.from_numpy(case["S"]).cuda()
        dt = torch.from_numpy(case["t"]).cuda()
        cap = len(want["m"]) + 5
        dm = torch.full((cap,), 7, dtype=torch.int32, device="cuda")
        did = torch.full((cap,), 7, dtype=torch.int32, device="cuda")
        ds = torch.full((cap,), 7.0, dtype=torch.float64, device="cuda")
        dc = torch.full((33,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        nh = eng.pssm_scan_dev(dS.data_ptr(), dt.data_ptr(), 33, dm.data_ptr(), did.data_ptr(), ds.data_ptr(), cap,
                               dc.data_ptr())
        assert nh == len(want["m"])
        got = dict(m=dm[:nh].cpu().numpy().astype(np.uint32), id=did[:nh].cpu().numpy().astype(np.uint32),
                   score=ds[:nh].cpu().numpy(), cnt=dc.cpu().numpy().astype(np.uint64))
        _same(got, want, "dev")
        assert int(dm[nh]) == 7 and float(ds[nh]) == 7.0
        # refusals found on the device, before anything is written
        dm.fill_(9), ds.fill_(9.0), dc.fill_(9)
        for where, bad in (("S", float("nan")), ("S", float("inf")), ("S", 2.0 ** 101), ("t", float("nan")),
                           ("t", float("-inf"))):
            dS2, dt2 = dS.clone(), dt.clone()
            if where == "S":
                dS2[20, 13, 7] = bad
            else:
                dt2[32] = bad
            torch.cuda.synchronize()
            with pytest.raises(HsError) as e:
                eng.pssm_scan_dev(dS2.data_ptr(), dt2.data_ptr(), 33, dm.data_ptr(), did.data_ptr(), ds.data_ptr(),
                                  cap, dc.data_ptr())
            assert e.value.status == capi.HS_ERR_INVALID and e.value.n_hits == 0
            assert bool((dm == 9).all()) and bool((ds == 9.0).all()) and bool((dc == 9).all())
        # the host form
        lib, h = eng._lib, eng._h
        hm, hid, hs = np.full(cap, 7, np.uint32), np.full(cap, 7, np.uint32), np.full(cap, 7.0)
        cnt = np.full(33, 7, np.uint64)
        n = C.c_uint64(5)
        S2 = case["S"].copy()
        S2[1, 2, 3] = np.nan
        for Sx, tx, nm in ((S2, case["t"], 33), (case["S"], np.where(np.arange(33) == 4, np.inf, case["t"]), 33),
                           (case["S"], case["t"], 1 << 27)):
            st = lib.hs_pssm_scan(h, capi._vp(Sx), capi._vp(tx), C.c_uint64(nm), capi._vp(hm), capi._vp(hid),
                                  capi._vp(hs), cap, C.byref(n), capi._vp(cnt))
            assert st == capi.HS_ERR_INVALID and n.value == 0
            assert np.all(hm == 7) and np.all(hid == 7) and np.all(hs == 7.0) and np.all(cnt == 7)
        with pytest.raises(HsError):
            eng.set_option("pssm_filter", 2)
        # nm = 0 is an empty, successful scan
        assert len(eng.pssm_scan(np.zeros((0, 25, 20)), np.zeros(0))["m"]) == 0
    finally:
        eng.close()
    unbuilt = _engine(25, 20)
    try:
        with pytest.raises(HsError) as e:
            unbuilt.pssm_scan(case["S"], case["t"])
        assert e.value.status == capi.HS_ERR_STATE
    finally:
        unbuilt.close()


def test_other_calls_around_a_scan():
    """A search and an hs_index_append on the same handle give what they gave, before and after a scan."""
    k = 25
    codes = synth.make_db(3000, k, seed=31)
    more = synth.make_db(500, k, seed=32)
    centers, _ = synth.make_queries(codes, 40, max_subst=2, seed=33)
    a, b = synth.make_planes(k, 4, 3, 120.0, seed=3)
    rng = np.random.default_rng(34)
    S = rng.integers(-12, 13, size=(17, k, 20)) / 4.0
    both = np.concatenate([codes, more])
    t = np.sort(pssm_ref.scores(S, both), axis=1)[:, -40].copy()
    eng = Engine(k, 4, 3, 120.0, a, b)
    ref = Engine(k, 4, 3, 120.0, a, b)
    try:
        eng.index_build(codes)
        ref.index_build(codes)
        q0 = ref.query(centers, 45.0)
        _same(eng.pssm_scan(S, t), pssm_ref.scan(S, t, codes), "before the append")
        q1 = eng.query(centers, 45.0)
        for f in ("q", "id", "table", "dist", "cand"):
            assert np.array_equal(q0[f], q1[f]), f
        assert len(q0["q"]) > 0
        info = eng.index_append(more)
        assert info == {**ref.index_append(more), "device_bytes": info["device_bytes"]}
        _same(eng.pssm_scan(S, t), pssm_ref.scan(S, t, both), "after the append")
        q2, q3 = eng.query(centers, 45.0), ref.query(centers, 45.0)
        for f in ("q", "id", "table", "dist", "cand"):
            assert np.array_equal(q2[f], q3[f]), f
    finally:
        eng.close()
        ref.close()
