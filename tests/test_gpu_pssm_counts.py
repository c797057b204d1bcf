"""hs_pssm_hit_counts and hs_pssm_refine on the GPU against the numpy rule of tests/pssm_counts_ref.py, bit for bit:
both modes over a windows index of proteins around k with the profile mix of tests/test_gpu_pssm_seq.py; runs inside an
item, cut by one item edge and by many at several chunk sizes; every shape of the histogram; identical counts across
the filter setting, the profile batch, a forced survivor split, a loaded index, device pointers and a changed index;
every refusal; the handle's other calls around it; and the loop's whole trajectory."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import pssm_counts_ref as ref, pssm_ref, pssm_seq_ref, seqmatch_ref

pytestmark = pytest.mark.gpu

K, A = 15, 20


def _coords(alphabet):
    if alphabet == 20:
        return None
    rng = np.random.default_rng(77)
    return np.ascontiguousarray(np.concatenate([synth.coords(), rng.normal(0, 3, size=(alphabet - 20, 8))]))


def _engine(k=K, alphabet=A, codes=None, hooks=False):
    a, b = synth.make_planes(k, 2, 1, 200.0, seed=3)
    eng = Engine(k, 2, 1, 200.0, a, b, coords=_coords(alphabet), hooks=hooks)
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
    33 profiles of tests/test_gpu_pssm_seq.py's mix and their reference hits -- computed once."""
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
        hits = pssm_ref.scan(S, t, codes)
        _CASE.update(P=P, codes=codes, id_start=id_start, S=S, t=t, hits=hits, n=n, want={})
    return _CASE


def _want(case, nm, per_protein):
    key = (nm, per_protein)
    if key not in case["want"]:
        keep = case["hits"]["m"] < nm
        hits = {f: case["hits"][f][keep] for f in ("m", "id", "score")}
        case["want"][key] = ref.from_hits(case["codes"], A, hits, nm, case["id_start"] if per_protein else None)
    return case["want"][key]


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
    every, one = _want(case, 33, False), _want(case, 33, True)
    wins = np.diff(case["id_start"].astype(np.int64))
    assert every["used"][5] == 0 and not every["counts"][5].any()                      # dead
    assert every["used"][7] == case["n"] and one["used"][7] == (wins > 0).sum()        # everything hits
    assert every["used"][9] == 1 and every["counts"][9].sum() == K                     # one hit
    assert not every["counts"][3][:, 0].any() and every["used"][3] > 0                 # the forbidden residue
    assert (one["used"] <= every["used"]).all() and (one["used"] < every["used"]).sum() > 20
    assert np.array_equal(every["cnt"], one["cnt"]) and not np.array_equal(every["counts"], one["counts"])


@pytest.mark.parametrize("nm", [1, 17, 33])
@pytest.mark.parametrize("per_protein", [False, True])
def test_counts_equal_the_rule(prot, nm, per_protein):
    eng = prot["eng"]
    ids = prot["id_start"] if per_protein else None
    want = _want(prot, nm, per_protein)
    got = eng.pssm_hit_counts(prot["S"][:nm], prot["t"][:nm], ids)
    ref.same_counts(got, want, (nm, per_protein))
    p = eng.profile()
    assert p["pssm_count_sites"] == int(want["used"].sum()) and p["hits"] == want["n_hits"]
    assert p["pssm_count_items"] >= int((want["used"] > 0).sum())
    # cnt and used are the list call's cnt and the per-sequence call's seq_cnt on the same handle
    listed = eng.pssm_scan(prot["S"][:nm], prot["t"][:nm])
    assert eng.profile()["pssm_survivors"] == p["pssm_survivors"] and eng.profile()["pssm_dead"] == p["pssm_dead"]
    assert np.array_equal(got["cnt"], listed["cnt"])
    if per_protein:
        assert np.array_equal(got["used"], eng.pssm_seq_scan(prot["S"][:nm], prot["t"][:nm], ids)["seq_cnt"])
    else:
        assert np.array_equal(got["used"], listed["cnt"])
    # the list reduced on the host is the same counts
    host = capi.pssm_count_hits(prot["codes"], A, listed["m"], listed["id"], listed["score"], nm, ids)
    assert np.array_equal(host["counts"], got["counts"]) and np.array_equal(host["used"], got["used"])


def test_run_boundaries():
    """Two profiles that hit everything over sequences of 1, 63, 64, 65, 129 and 4097 windows (4419 sites each) at
    chunks of 1, 64, 100 sites and the default (256 here): runs inside an item, cut by one item edge and by many, and
    the second profile's run starting inside a wave (4419 = 69 x 64 + 3)."""
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
    eng = _engine()
    try:
        info, _ = eng.index_build_windows(residues, seq_start)
        assert info["n"] == sum(wins) == 4419
        for ids in (None, id_start):
            for nm in (1, 2):
                want = ref.hit_counts(codes, A, S[:nm], t[:nm], ids)
                assert want["used"].tolist() == [6 if ids is not None else 4419] * nm
                sparse = ref.hit_counts(codes, A, S[:nm], t2[:nm], ids)
                # (the default: the batch's sites / 4096 within 256 .. 2048 -- 256 here, 18 items per run of 4419)
                for chunk, items in ((1, 4419 * nm), (64, 70 * nm), (100, 45 * nm), (0, 18 * nm)):
                    eng.set_option("pssm_count_chunk", chunk)
                    ref.same_counts(eng.pssm_hit_counts(S[:nm], t[:nm], ids), want, (nm, chunk))
                    if ids is None:
                        assert eng.profile()["pssm_count_items"] == items
                    else:
                        assert eng.profile()["pssm_count_items"] == (6 * nm if chunk == 1 else nm)
                    ref.same_counts(eng.pssm_hit_counts(S[:nm], t2[:nm], ids), sparse, (nm, chunk, "sparse"))
    finally:
        eng.close()


@pytest.mark.parametrize("k,alphabet", [(1, 20), (25, 20), (26, 20), (4, 32), (75, 32)])
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_shapes(k, alphabet, n):
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
    eng = _engine(k, alphabet, codes)
    try:
        for ids in (None, id_start):
            want = ref.from_hits(codes, alphabet, hits, nm, ids)
            assert want["used"][1] > 0 and want["used"][3] == 0
            for filt, chunk in ((1, 0), (0, 0), (1, 7)):
                eng.set_option("pssm_filter", filt)
                eng.set_option("pssm_count_chunk", chunk)
                ref.same_counts(eng.pssm_hit_counts(S, t, ids), want, (k, alphabet, n, ids is None, filt, chunk))
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
                    ref.same_counts(eng.pssm_hit_counts(prot["S"], prot["t"], ids), want, (per_protein, filt, batch))
                    s = eng.profile()["pssm_survivors"]
                    assert s == 33 * prot["n"] if not filt else s < 33 * prot["n"]
    finally:
        eng.set_option("pssm_filter", 1)
        eng.set_option("query_batch", 0)


def test_forced_split_and_loaded_index(prot, monkeypatch, tmp_path):
    """The TEST build reports a survivor-counter overflow for every batch of more than 4 profiles: the same profiles
    run again in smaller batches and nothing shows.  The same counts from a saved and loaded index."""
    path = tmp_path / "p.idx"
    prot["eng"].index_save(path)
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "4")
    eng = _engine(hooks=True)
    try:
        eng.index_load(path)
        for per_protein in (False, True):
            ids = prot["id_start"] if per_protein else None
            ref.same_counts(eng.pssm_hit_counts(prot["S"], prot["t"], ids), _want(prot, 33, per_protein), "split, loaded")
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
    dn = torch.full((nm,), 7, dtype=torch.int64, device="cuda")
    du = torch.full((nm,), 7, dtype=torch.int64, device="cuda")

    def dev(S=dS, t=dt, I=None, ns=0, counts=dc, nm_=nm):
        torch.cuda.synchronize()
        return eng.pssm_hit_counts_dev(S.data_ptr(), t.data_ptr(), nm_, counts.data_ptr() if counts is not None else 0,
                                       I.data_ptr() if I is not None else None, ns, dn.data_ptr(), du.data_ptr())

    def got(nh):
        return dict(counts=dc.cpu().numpy().astype(np.uint32), cnt=dn.cpu().numpy().astype(np.uint64),
                    used=du.cpu().numpy().astype(np.uint64), n_hits=nh)

    ref.same_counts(got(dev()), _want(prot, nm, False), "dev")
    ref.same_counts(got(dev(I=dI, ns=n_seq)), _want(prot, nm, True), "dev, per protein")
    # cnt and used may be null
    torch.cuda.synchronize()
    assert eng.pssm_hit_counts_dev(dS.data_ptr(), dt.data_ptr(), nm, dc.data_ptr()) == _want(prot, nm, False)["n_hits"]
    # refusals found on the device, before anything is written
    dc.fill_(9), dn.fill_(9), du.fill_(9)

    def refused(status=capi.HS_ERR_INVALID, **kw):
        with pytest.raises(HsError) as e:
            dev(**kw)
        assert e.value.status == status
        assert bool((dc == 9).all()) and bool((dn == 9).all()) and bool((du == 9).all())

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
    refused(counts=None)
    refused(nm_=1 << 27)
    # the host form: the same refusals, with sentinel-filled outputs untouched
    lib, h = eng._lib, eng._h
    counts = np.full((nm, K, A), 9, np.uint32)
    cnt, used = np.full(nm, 9, np.uint64), np.full(nm, 9, np.uint64)
    n_hits = C.c_uint64(5)
    ids = prot["id_start"]

    def host(S=prot["S"], t=prot["t"], I=None, ns=None, nm_=nm, c=counts):
        st = lib.hs_pssm_hit_counts(h, capi._vp(S), capi._vp(t), C.c_uint64(nm_), None if I is None else capi._vp(I),
                                    C.c_uint64((len(I) - 1 if I is not None else 0) if ns is None else ns),
                                    None if c is None else capi._vp(c), capi._vp(cnt), capi._vp(used), C.byref(n_hits))
        assert n_hits.value == 0
        assert np.all(counts == 9) and np.all(cnt == 9) and np.all(used == 9)
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
        assert host(c=None, I=I) == bad
    assert host(I=changed(30, int(ids[31]) + 1)) == bad      # does not ascend
    assert host(I=changed(0, 1)) == bad                      # does not start at 0
    assert host(I=changed(n_seq, int(ids[-1]) + 1)) == bad   # does not end at n
    assert host(I=ids, ns=0) == bad
    assert host(I=ids, ns=(1 << 32) + 1) == bad
    # the loop's own refusals
    S_out = np.full((nm, K, A), 9.0)
    iters, conv = C.c_uint32(7), C.c_uint32(7)

    def loop(S=prot["S"], n_iter=2, bg=None, pseudo=1.0, I=None, out=S_out):
        st = lib.hs_pssm_refine(h, capi._vp(S), capi._vp(prot["t"]), nm, None if I is None else capi._vp(I),
                                0 if I is None else len(I) - 1, None if bg is None else capi._vp(bg), pseudo, n_iter,
                                None if out is None else capi._vp(out), capi._vp(counts), capi._vp(used),
                                C.byref(iters), C.byref(conv))
        assert iters.value == 0 and conv.value == 0
        assert np.all(S_out == 9.0) and np.all(counts == 9) and np.all(used == 9)
        return st

    assert loop(n_iter=0) == bad and loop(n_iter=101) == bad
    for pseudo in (0.0, -1.0, np.inf, np.nan):
        assert loop(pseudo=pseudo) == bad
    for v in (0.0, -0.1, np.inf, np.nan):
        b = np.full(A, 0.05)
        b[3] = v
        assert loop(bg=b) == bad
    assert loop(S=S2) == bad and loop(I=changed(0, 1)) == bad and loop(out=None) == bad
    # nm = 0 is an empty, successful call
    empty = eng.pssm_hit_counts(np.zeros((0, K, A)), np.zeros(0), ids)
    assert empty["counts"].shape == (0, K, A) and empty["n_hits"] == 0
    unbuilt = _engine()
    try:
        with pytest.raises(HsError) as e:
            unbuilt.pssm_hit_counts(prot["S"], prot["t"])
        assert e.value.status == capi.HS_ERR_STATE
        with pytest.raises(HsError) as e:
            unbuilt.pssm_refine(prot["S"], prot["t"], 2)
        assert e.value.status == capi.HS_ERR_STATE
    finally:
        unbuilt.close()


def test_counts_follow_a_changed_index():
    """After index_append and index_remove the counts are those of the new index."""
    rng = np.random.default_rng(41)
    base = rng.integers(0, A, size=(700, K)).astype(np.uint8)
    more = rng.integers(0, A, size=(333, K)).astype(np.uint8)
    S = rng.integers(-8, 9, size=(4, K, A)) / 4.0
    t = np.sort(pssm_ref.scores(S, np.concatenate([base, more])), axis=1)[:, -100].copy()
    t[2] = -1e6
    eng = _engine(codes=base)
    try:
        ref.same_counts(eng.pssm_hit_counts(S, t), ref.hit_counts(base, A, S, t), "built")
        eng.index_append(more)
        both = np.concatenate([base, more])
        ids = np.array([0, 10, 10, 700, 1033], np.uint64)
        ref.same_counts(eng.pssm_hit_counts(S, t), ref.hit_counts(both, A, S, t), "appended")
        ref.same_counts(eng.pssm_hit_counts(S, t, ids), ref.hit_counts(both, A, S, t, ids), "appended, per protein")
        gone = rng.choice(1033, size=200, replace=False)
        new_id = eng.index_remove(gone)
        left = both[new_id != 0xffffffff]
        assert len(left) == 833
        ids = np.array([0, 400, 833], np.uint64)
        ref.same_counts(eng.pssm_hit_counts(S, t), ref.hit_counts(left, A, S, t), "removed")
        ref.same_counts(eng.pssm_hit_counts(S, t, ids), ref.hit_counts(left, A, S, t, ids), "removed, per protein")
    finally:
        eng.close()


def test_other_calls_around_it():
    """hs_pssm_scan, hs_pssm_seq_scan and hs_query on the same handle give what they gave, before and after."""
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
            return [eng.pssm_scan(S, t), eng.pssm_seq_scan(S, t, ids), eng.query(centers, seqmatch_ref.R)]

        before = others()
        ref.same_counts(eng.pssm_hit_counts(S, t), _want(case, 17, False), "between")
        ref.same_counts(eng.pssm_hit_counts(S, t, ids), _want(case, 17, True), "between, per protein")
        eng.pssm_refine(S, t, 2, ids)
        after = others()
        assert len(before) == 3
        for x, y in zip(before, after):
            assert x.keys() == y.keys()
            for f in x:
                assert np.array_equal(x[f], y[f]), f
        assert len(before[0]["m"]) > 0 and len(before[2]["id"]) > 0
    finally:
        eng.close()


def planted(seed=5):
    """A planted-family database: 70 proteins of 40 .. 120 residues; proteins 0 .. 29 carry one instance of motif 0,
    proteins 30 .. 49 one of motif 1, every position mutated with probability 0.15.  Profiles: the two consensus
    matrices (match / mismatch scores) and a third whose motif is nowhere, at fixed thresholds."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(40, 121, size=70)
    residues = rng.integers(0, A, size=int(lens.sum())).astype(np.uint8)
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    motifs = rng.integers(0, A, size=(3, K)).astype(np.uint8)
    for s in range(50):
        f = 0 if s < 30 else 1
        inst = motifs[f].copy()
        mut = rng.random(K) < 0.15
        inst[mut] = rng.integers(0, A, size=int(mut.sum()))
        at = int(seq_start[s]) + int(rng.integers(0, lens[s] - K + 1))
        residues[at:at + K] = inst
    codes, id_start = _windows(residues, seq_start)

    def consensus(match, mismatch):
        S = np.full((3, K, A), mismatch)
        for f in range(3):
            S[f, np.arange(K), motifs[f]] = match
        return S

    return dict(residues=residues, seq_start=seq_start, codes=codes, id_start=id_start, t=np.array([25.0, 25.0, 25.0]),
                loose=consensus(3.0, -1.0), strict=consensus(3.0, -6.0))


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
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["used"], want["used"]), what
    assert got["counts"].dtype == np.uint32 and got["used"].dtype == np.uint64


@pytest.mark.parametrize("per_protein", [False, True])
def test_refine_equals_the_reference_loop(family, per_protein):
    eng, codes, t = family["eng"], family["codes"], family["t"]
    ids = family["id_start"] if per_protein else None
    # converges inside n_iter = 8; the default background is the index's composition
    want = ref.refine(codes, A, family["loose"], t, 8, ids)
    assert want["converged"] and 2 <= want["iters"] < 8 and want["used"][0] >= 20 and want["used"][1] >= 12
    got = eng.pssm_refine(family["loose"], t, 8, ids)
    _same_loop(got, want, "converges")
    assert got["used"][2] == 0       # a profile without hits keeps its S bitwise
    assert np.array_equal(got["S"][2].view(np.uint64), family["loose"][2].view(np.uint64))
    assert not np.array_equal(got["S"][0], family["loose"][0])
    again = eng.pssm_hit_counts(got["S"], t, ids)       # converged: the counts of S_out are the counts returned
    assert np.array_equal(again["counts"], got["counts"]) and np.array_equal(again["used"], got["used"])
    # does not converge within n_iter = 2: the second scan finds more than the first
    want = ref.refine(codes, A, family["strict"], t, 2, ids)
    assert not want["converged"] and want["iters"] == 2
    assert not np.array_equal(want["history"][0], want["history"][1])
    _same_loop(eng.pssm_refine(family["strict"], t, 2, ids), want, "does not converge")
    _same_loop(eng.pssm_refine(family["strict"], t, 1, ids), ref.refine(codes, A, family["strict"], t, 1, ids), "one")
    # a given background and pseudo-count
    bg = np.linspace(1.0, 2.0, A) / np.linspace(1.0, 2.0, A).sum()
    want = ref.refine(codes, A, family["strict"], t, 5, ids, bg=bg, pseudo=0.5)
    _same_loop(eng.pssm_refine(family["strict"], t, 5, ids, background=bg, pseudo=0.5), want, "bg")
