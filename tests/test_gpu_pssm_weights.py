"""hs_pssm_weighted_counts and hs_pssm_refine_weighted on the GPU against the host rule (capi.pssm_weight_hits) and the
Python-integer rule of tests/pssm_weights_ref.py, bit for bit, in both site modes: the proteins of
tests/test_gpu_pssm_counts.py; every lane-group size, two positions per lane and the largest histogram; runs inside an
item, cut by one item edge and by many; one k-mer repeated 4097 times; identical outputs across the filter setting,
the profile batch, a forced survivor split, a loaded index, device pointers and a changed index; counts equal to
hs_pssm_hit_counts; every refusal; the handle's other calls around it; and the loop's whole trajectory."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import pssm_ref, pssm_weights_ref as ref, seqmatch_ref
from tests.test_gpu_pssm_counts import _engine, _proteins, _windows, planted

pytestmark = pytest.mark.gpu

K, A = 15, 20
_WANT = {}


def _host(codes, alphabet, hits, nm, ids):
    """the host rule over a reference hit list, checked once against the Python-integer rule's invariants"""
    keep = hits["m"] < nm
    got = capi.pssm_weight_hits(codes, alphabet, hits["m"][keep], hits["id"][keep], hits["score"][keep], nm, ids)
    got.update(cnt=np.bincount(hits["m"][keep].astype(np.int64), minlength=nm).astype(np.uint64),
               n_hits=int(keep.sum()))
    return got


def _want(case, nm, per_protein):
    key = (nm, per_protein)
    if key not in _WANT:
        ids = case["id_start"] if per_protein else None
        _WANT[key] = _host(case["codes"], A, case["hits"], nm, ids)
        if nm == 17:    # the host rule is the Python-integer rule (tests/test_pssm_weights_cpu.py holds it to that too)
            keep = case["hits"]["m"] < nm
            hits = {f: case["hits"][f][keep] for f in ("m", "id", "score")}
            ref.same_weights(_WANT[key], ref.from_hits(case["codes"], A, hits, nm, ids), "host rule")
    return _WANT[key]


@pytest.fixture(scope="module")
def prot():
    case = _proteins()
    eng = _engine()
    info, _ = eng.index_build_windows(case["P"]["db"], case["P"]["db_start"])
    assert info["n"] == case["n"]
    yield dict(case, eng=eng)
    eng.close()


@pytest.mark.parametrize("nm", [1, 17, 33])
@pytest.mark.parametrize("per_protein", [False, True])
def test_weights_equal_the_rule(prot, nm, per_protein):
    eng = prot["eng"]
    ids = prot["id_start"] if per_protein else None
    want = _want(prot, nm, per_protein)
    got = eng.pssm_weighted_counts(prot["S"][:nm], prot["t"][:nm], ids)
    ref.same_weights(got, want, (nm, per_protein))
    p = eng.profile()
    assert p["pssm_weight_sites"] == p["pssm_count_sites"] == int(want["used"].sum()) and p["hits"] == want["n_hits"]
    assert p["pssm_weight_items"] == p["pssm_count_items"] >= int((want["used"] > 0).sum())
    if nm == 33:
        assert want["used"][5] == 0 and not got["wcounts"][5].any() and got["distinct"][5] == 0      # dead
        assert want["used"][9] == 1 and got["wsum"][9] == K << 56                                    # one site
    # counts, cnt and used are hs_pssm_hit_counts' on the same handle, which leaves the weight fields alone
    raw = eng.pssm_hit_counts(prot["S"][:nm], prot["t"][:nm], ids)
    for f in ("counts", "cnt", "used"):
        assert np.array_equal(raw[f], got[f]), f
    q = eng.profile()
    assert q["pssm_weight_sites"] == 0 and q["pssm_weight_items"] == 0 and q["pssm_count_items"] == p["pssm_count_items"]


def test_run_boundaries():
    """Two profiles that hit everything over sequences of 1, 63, 64, 65, 129 and 4097 windows (4419 sites each) at
    chunks of 1, 64, 100 sites and the default: whole runs, runs cut by one item edge and by many."""
    wins = [1, 63, 64, 65, 129, 4097]
    rng = np.random.default_rng(3)
    lens = [w + K - 1 for w in wins]
    residues = rng.integers(0, A, size=sum(lens)).astype(np.uint8)
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    codes, id_start = _windows(residues, seq_start)
    S = np.random.default_rng(17).integers(-2, 3, size=(2, K, A)) / 2.0
    t = np.array([-1e6, -1e6])
    sc = pssm_ref.scores(S, codes)
    t2 = np.sort(sc, axis=1)[:, -300].copy()     # sparse runs: 300-odd sites per profile
    dense, sparse = pssm_ref.scan(S, t, codes), pssm_ref.scan(S, t2, codes)
    eng = _engine()
    try:
        eng.index_build_windows(residues, seq_start)
        for ids in (None, id_start):
            for nm in (1, 2):
                want, want2 = _host(codes, A, dense, nm, ids), _host(codes, A, sparse, nm, ids)
                assert want["used"].tolist() == [6 if ids is not None else 4419] * nm
                for chunk, items in ((1, 4419 * nm), (64, 70 * nm), (100, 45 * nm), (0, 18 * nm)):
                    eng.set_option("pssm_count_chunk", chunk)
                    ref.same_weights(eng.pssm_weighted_counts(S[:nm], t[:nm], ids), want, (nm, chunk))
                    if ids is None:
                        assert eng.profile()["pssm_weight_items"] == items
                    ref.same_weights(eng.pssm_weighted_counts(S[:nm], t2[:nm], ids), want2, (nm, chunk, "sparse"))
    finally:
        eng.close()


@pytest.mark.parametrize("k,alphabet", [(1, 20), (3, 4), (25, 20), (33, 20), (65, 32), (75, 32)])
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_shapes(k, alphabet, n):
    """the lane groups of 1, 4, 32 and 64 lanes, two positions per lane (65, 75) and the largest histogram (75 x 32)"""
    rng = np.random.default_rng(1000 * k + 10 * alphabet + n)
    codes = rng.integers(0, alphabet, size=(n, k)).astype(np.uint8)
    nm = 5
    S = rng.integers(-8, 9, size=(nm, k, alphabet)) / 4.0
    sc = pssm_ref.scores(S, codes)
    t = np.sort(sc, axis=1)[:, -max(1, n // 8)].copy()
    t[1] = -1e6
    t[3] = sc[3].max() + 1.0
    cuts = np.sort(rng.integers(0, n + 1, size=7))
    id_start = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    hits = pssm_ref.scan(S, t, codes)
    a, b = synth.make_planes(k, 2, 1, 200.0, seed=3)
    coords = None if alphabet == 20 else np.ascontiguousarray(np.random.default_rng(77).normal(0, 3, size=(alphabet, 8)))
    eng = Engine(k, 2, 1, 200.0, a, b, coords=coords)
    try:
        eng.index_build(codes)
        for ids in (None, id_start):
            want = _host(codes, alphabet, hits, nm, ids)
            assert want["used"][1] > 0 and want["used"][3] == 0
            if n == 65:
                keep = {f: hits[f] for f in ("m", "id", "score")}
                ref.same_weights(want, ref.from_hits(codes, alphabet, keep, nm, ids), "host rule")
            for filt, chunk in ((1, 0), (0, 0), (1, 7)):
                eng.set_option("pssm_filter", filt)
                eng.set_option("pssm_count_chunk", chunk)
                ref.same_weights(eng.pssm_weighted_counts(S, t, ids), want, (k, alphabet, n, ids is None, filt, chunk))
    finally:
        eng.close()


def test_one_kmer_repeated():
    """4097 copies of one k-mer: every site lands in the same bins, every column holds one residue, and the copies
    share k 2^56 up to the floor: W = k floor(2^56 / 4097)"""
    k = 25
    codes = np.tile(np.random.default_rng(9).integers(0, A, size=k).astype(np.uint8), (4097, 1))
    S = np.zeros((2, k, A))
    t = np.array([-1.0, -1.0])
    eng = _engine(k, A, codes)
    try:
        for chunk in (0, 64):
            eng.set_option("pssm_count_chunk", chunk)
            got = eng.pssm_weighted_counts(S, t)
            ref.same_weights(got, _host(codes, A, pssm_ref.scan(S, t, codes), 2, None), chunk)
            w = k * ((1 << 56) // 4097)
            assert got["wsum"].tolist() == [4097 * w] * 2 and got["distinct"].tolist() == [k] * 2
            assert int(got["wcounts"][1, 3, codes[0, 3]]) == 4097 * w and got["used"].tolist() == [4097] * 2
    finally:
        eng.close()


def test_filter_and_batches_do_not_show(prot):
    eng = prot["eng"]
    try:
        for per_protein in (False, True):
            want = _want(prot, 33, per_protein)
            ids = prot["id_start"] if per_protein else None
            for filt in (1, 0):
                eng.set_option("pssm_filter", filt)
                for batch in (1, 16, 0):
                    eng.set_option("query_batch", batch)
                    ref.same_weights(eng.pssm_weighted_counts(prot["S"], prot["t"], ids), want, (per_protein, filt, batch))
    finally:
        eng.set_option("pssm_filter", 1)
        eng.set_option("query_batch", 0)


def test_forced_split_and_loaded_index(prot, monkeypatch, tmp_path):
    """The TEST build reports a survivor-counter overflow for every batch of more than 4 profiles; the same weights
    from a saved and loaded index."""
    path = tmp_path / "p.idx"
    prot["eng"].index_save(path)
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "4")
    eng = _engine(hooks=True)
    try:
        eng.index_load(path)
        for per_protein in (False, True):
            ids = prot["id_start"] if per_protein else None
            ref.same_weights(eng.pssm_weighted_counts(prot["S"], prot["t"], ids), _want(prot, 33, per_protein),
                             "split, loaded")
            assert eng.profile()["verify_launches"] >= 9
    finally:
        eng.close()


def test_device_pointers_and_refusals(prot):
    import torch
    eng, nm = prot["eng"], 33
    dS, dt = torch.from_numpy(prot["S"]).cuda(), torch.from_numpy(prot["t"]).cuda()
    dI = torch.from_numpy(prot["id_start"].astype(np.int64)).cuda()
    n_seq = len(prot["id_start"]) - 1
    dc = torch.full((nm, K, A), 7, dtype=torch.int32, device="cuda")
    dw = torch.full((nm, K, A), 7, dtype=torch.int64, device="cuda")
    ds, dn, du = (torch.full((nm,), 7, dtype=torch.int64, device="cuda") for _ in range(3))
    dd = torch.full((nm,), 7, dtype=torch.int32, device="cuda")
    outs = (dc, dw, ds, dn, du, dd)

    def dev(S=dS, t=dt, I=None, ns=0, w=dw, nm_=nm, rest=True):
        torch.cuda.synchronize()
        nh = eng.pssm_weighted_counts_dev(S.data_ptr(), t.data_ptr(), nm_, w.data_ptr() if w is not None else 0,
                                          I.data_ptr() if I is not None else None, ns,
                                          *([dc.data_ptr(), ds.data_ptr(), dd.data_ptr(), dn.data_ptr(), du.data_ptr()]
                                            if rest else []))
        torch.cuda.synchronize()
        return nh

    def got(nh):
        return dict(counts=dc.cpu().numpy().astype(np.uint32), wcounts=dw.cpu().numpy().view(np.uint64),
                    wsum=ds.cpu().numpy().view(np.uint64), distinct=dd.cpu().numpy().astype(np.uint32),
                    cnt=dn.cpu().numpy().astype(np.uint64), used=du.cpu().numpy().astype(np.uint64), n_hits=nh)

    ref.same_weights(got(dev()), _want(prot, nm, False), "dev")
    ref.same_weights(got(dev(I=dI, ns=n_seq)), _want(prot, nm, True), "dev, per protein")
    # every optional output left out: counts stay in the handle's scratch
    dw.fill_(7)
    assert dev(rest=False) == _want(prot, nm, False)["n_hits"]
    assert np.array_equal(dw.cpu().numpy().view(np.uint64), _want(prot, nm, False)["wcounts"])
    for o in outs:
        o.fill_(9)

    def refused(status=capi.HS_ERR_INVALID, **kw):
        with pytest.raises(HsError) as e:
            dev(**kw)
        assert e.value.status == status
        assert all(bool((o == 9).all()) for o in outs)

    for where, bad in (("S", float("nan")), ("S", float("inf")), ("S", 2.0 ** 101), ("t", float("nan")),
                       ("t", float("-inf"))):
        S2, t2 = dS.clone(), dt.clone()
        if where == "S":
            S2[20, 13, 7] = bad
        else:
            t2[32] = bad
        refused(S=S2, t=t2)
        refused(S=S2, t=t2, I=dI, ns=n_seq)
    for change in ("descends", "starts", "ends"):
        I2 = dI.clone()
        if change == "descends":
            I2[30] = I2[31] + 1
        elif change == "starts":
            I2[0] = 1
        else:
            I2[n_seq] -= 1
        refused(I=I2, ns=n_seq)
    refused(I=dI, ns=0)
    refused(I=dI, ns=(1 << 32) + 1)
    refused(w=None)
    refused(nm_=1 << 27)
    # the host form: the same refusals, with sentinel-filled outputs untouched
    lib, h = eng._lib, eng._h
    counts, wcounts = np.full((nm, K, A), 9, np.uint32), np.full((nm, K, A), 9, np.uint64)
    wsum, cnt, used = (np.full(nm, 9, np.uint64) for _ in range(3))
    distinct = np.full(nm, 9, np.uint32)
    host_outs = (counts, wcounts, wsum, cnt, used, distinct)
    n_hits = C.c_uint64(5)
    ids = prot["id_start"]

    def host(S=prot["S"], t=prot["t"], I=None, ns=None, nm_=nm, w=wcounts):
        st = lib.hs_pssm_weighted_counts(h, capi._vp(S), capi._vp(t), C.c_uint64(nm_),
                                         None if I is None else capi._vp(I),
                                         C.c_uint64((len(I) - 1 if I is not None else 0) if ns is None else ns),
                                         capi._vp(counts), None if w is None else capi._vp(w), capi._vp(wsum),
                                         capi._vp(distinct), capi._vp(cnt), capi._vp(used), C.byref(n_hits))
        assert n_hits.value == 0 and all(np.all(o == 9) for o in host_outs)
        return st

    def changed(at, value):
        c = ids.copy()
        c[at] = value
        return c

    S2 = prot["S"].copy()
    S2[1, 2, 3] = np.nan
    bad = capi.HS_ERR_INVALID
    for I in (None, ids):
        assert host(S=S2, I=I) == bad
        assert host(t=np.where(np.arange(nm) == 4, np.inf, prot["t"]), I=I) == bad
        assert host(nm_=1 << 27, I=I) == bad
        assert host(w=None, I=I) == bad
    assert host(I=changed(30, int(ids[31]) + 1)) == bad      # does not ascend
    assert host(I=changed(0, 1)) == bad                      # does not start at 0
    assert host(I=changed(n_seq, int(ids[-1]) + 1)) == bad   # does not end at n
    assert host(I=ids, ns=0) == bad
    assert host(I=ids, ns=(1 << 32) + 1) == bad
    # the loop's own refusals
    S_out, t_out = np.full((nm, K, A), 9.0), np.full(nm, 9.0)
    rank = np.full(nm, 100, np.uint64)
    iters, conv = C.c_uint32(7), C.c_uint32(7)

    def loop(S=prot["S"], t=prot["t"], r=None, n_iter=2, bg=None, pseudo=1.0, I=None, out=S_out, rule=0, to=t_out):
        st = lib.hs_pssm_refine_weighted(h, capi._vp(S), None if t is None else capi._vp(t),
                                         None if r is None else capi._vp(r), nm, None if I is None else capi._vp(I),
                                         0 if I is None else len(I) - 1, None if bg is None else capi._vp(bg), pseudo,
                                         rule, n_iter, None if out is None else capi._vp(out),
                                         None if to is None else capi._vp(to), capi._vp(counts), capi._vp(wcounts),
                                         capi._vp(wsum), capi._vp(distinct), capi._vp(used), C.byref(iters),
                                         C.byref(conv))
        assert iters.value == 0 and conv.value == 0
        assert np.all(S_out == 9.0) and np.all(t_out == 9.0) and all(np.all(o == 9) for o in host_outs)
        return st

    assert loop(n_iter=0) == bad and loop(n_iter=101) == bad
    assert loop(rule=2) == bad and loop(rule=0xffffffff) == bad
    assert loop(t=None) == bad and loop(r=rank) == bad                      # neither, both
    assert loop(t=None, r=rank, to=None) == bad                             # the rank rule needs t_out
    assert loop(t=None, r=np.where(np.arange(nm) == 3, 0, rank).astype(np.uint64)) == bad
    for pseudo in (0.0, -1.0, np.inf, np.nan):
        assert loop(pseudo=pseudo) == bad
    for v in (0.0, -0.1, np.inf, np.nan):
        b = np.full(A, 0.05)
        b[3] = v
        assert loop(bg=b) == bad
    assert loop(S=S2) == bad and loop(I=changed(0, 1)) == bad and loop(out=None) == bad
    # nm = 0 is an empty, successful call
    empty = eng.pssm_weighted_counts(np.zeros((0, K, A)), np.zeros(0), ids)
    assert empty["wcounts"].shape == (0, K, A) and empty["n_hits"] == 0
    unbuilt = _engine()
    try:
        with pytest.raises(HsError) as e:
            unbuilt.pssm_weighted_counts(prot["S"], prot["t"])
        assert e.value.status == capi.HS_ERR_STATE
        with pytest.raises(HsError) as e:
            unbuilt.pssm_refine_weighted(prot["S"], 2, t=prot["t"])
        assert e.value.status == capi.HS_ERR_STATE
    finally:
        unbuilt.close()


def test_weights_follow_a_changed_index():
    """After index_append and index_remove the weights are those of the new index."""
    rng = np.random.default_rng(41)
    base = rng.integers(0, A, size=(700, K)).astype(np.uint8)
    more = rng.integers(0, A, size=(333, K)).astype(np.uint8)
    S = rng.integers(-8, 9, size=(4, K, A)) / 4.0
    t = np.sort(pssm_ref.scores(S, np.concatenate([base, more])), axis=1)[:, -100].copy()
    t[2] = -1e6

    def want(codes, ids=None):
        return _host(codes, A, pssm_ref.scan(S, t, codes), 4, ids)

    eng = _engine(codes=base)
    try:
        ref.same_weights(eng.pssm_weighted_counts(S, t), want(base), "built")
        eng.index_append(more)
        both = np.concatenate([base, more])
        ids = np.array([0, 10, 10, 700, 1033], np.uint64)
        ref.same_weights(eng.pssm_weighted_counts(S, t), want(both), "appended")
        ref.same_weights(eng.pssm_weighted_counts(S, t, ids), want(both, ids), "appended, per protein")
        gone = rng.choice(1033, size=200, replace=False)
        new_id = eng.index_remove(gone)
        left = both[new_id != 0xffffffff]
        ids = np.array([0, 400, 833], np.uint64)
        ref.same_weights(eng.pssm_weighted_counts(S, t), want(left), "removed")
        ref.same_weights(eng.pssm_weighted_counts(S, t, ids), want(left, ids), "removed, per protein")
    finally:
        eng.close()


def test_other_calls_around_it():
    """hs_pssm_scan, hs_pssm_seq_scan, hs_pssm_hit_counts and hs_query on the same handle give what they gave."""
    case = _proteins()
    P = case["P"]
    lsh = seqmatch_ref.LSH
    a, b = synth.make_planes(K, lsh["K"], lsh["L"], lsh["W"])
    eng = Engine(K, lsh["K"], lsh["L"], lsh["W"], a, b)
    try:
        eng.index_build_windows(P["db"], P["db_start"])
        S, t, ids = case["S"][:17], case["t"][:17], case["id_start"]
        centers = synth.embed(case["codes"][:40])

        def others():
            return [eng.pssm_scan(S, t), eng.pssm_seq_scan(S, t, ids), eng.pssm_hit_counts(S, t, ids),
                    eng.query(centers, seqmatch_ref.R)]

        before = others()
        ref.same_weights(eng.pssm_weighted_counts(S, t), _want(case, 17, False), "between")
        ref.same_weights(eng.pssm_weighted_counts(S, t, ids), _want(case, 17, True), "between, per protein")
        eng.pssm_refine_weighted(S, 2, t=t, id_start=ids)
        after = others()
        for x, y in zip(before, after):
            assert x.keys() == y.keys()
            for f in x:
                assert np.array_equal(x[f], y[f]), f
        assert len(before[0]["m"]) > 0 and len(before[3]["id"]) > 0
    finally:
        eng.close()


@pytest.fixture(scope="module")
def family():
    fam = planted()
    eng = _engine()
    info, _ = eng.index_build_windows(fam["residues"], fam["seq_start"])
    assert info["n"] == len(fam["codes"])
    yield dict(fam, eng=eng)
    eng.close()


def _same_loop(got, want, what):
    assert got["iters"] == want["iters"] and got["converged"] == want["converged"], (what, got["iters"], want["iters"])
    assert np.array_equal(got["S"].view(np.uint64), want["S"].view(np.uint64)), what
    for f in ("counts", "wcounts", "wsum", "distinct", "used"):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f)
    if "t" in got:
        assert np.array_equal(got["t"].view(np.uint64), np.asarray(want["t"]).view(np.uint64)), what


@pytest.mark.parametrize("neff", ["sites", "columns"])
@pytest.mark.parametrize("by_rank", [False, True])
def test_refine_equals_the_reference_loop(family, neff, by_rank):
    eng, codes = family["eng"], family["codes"]
    how = dict(rank=np.array([40, 25, 10], np.uint64)) if by_rank else dict(t=family["t"])
    for ids in (None, family["id_start"]):
        # a start that converges inside n_iter = 8 (the default background is the index's composition)
        want = ref.refine(codes, A, family["loose"], 8, id_start=ids, neff=neff, **how)
        assert want["converged"] and 2 <= want["iters"] < 8 and want["used"][0] >= 10
        got = eng.pssm_refine_weighted(family["loose"], 8, id_start=ids, neff=neff, **how)
        _same_loop(got, want, ("converges", ids is None))
        if not by_rank:
            assert got["used"][2] == 0       # a profile without hits keeps its S bitwise
            assert np.array_equal(got["S"][2].view(np.uint64), family["loose"][2].view(np.uint64))
        again = eng.pssm_weighted_counts(got["S"], got["t"] if by_rank else family["t"], ids)
        assert np.array_equal(again["wcounts"], got["wcounts"]) and np.array_equal(again["counts"], got["counts"])
        # one that does not within n_iter = 2: the second scan finds something else than the first
        want = ref.refine(codes, A, family["strict"], 2, id_start=ids, neff=neff, **how)
        assert not want["converged"] and want["iters"] == 2
        _same_loop(eng.pssm_refine_weighted(family["strict"], 2, id_start=ids, neff=neff, **how), want,
                   ("does not converge", ids is None))
    bg = np.linspace(1.0, 2.0, A) / np.linspace(1.0, 2.0, A).sum()
    want = ref.refine(codes, A, family["strict"], 5, bg=bg, pseudo=0.5, neff=neff, **how)
    _same_loop(eng.pssm_refine_weighted(family["strict"], 5, background=bg, pseudo=0.5, neff=neff, **how), want, "bg")
