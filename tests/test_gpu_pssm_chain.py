"""hs_pssm_family_chain on the GPU against the host rule (capi.pssm_family_chain_hits over the same handle's
pssm_scan) and the contract of tests/pssm_chain_ref.py over tests/pssm_ref.py's scan: every array bit for bit -- over
every group layout, shifts of 0, 3 and 65535, segments of 1 to about 5000 hits across the kernel's tile and LDS edges,
runs longer than a wave, a family of 40 levels; identical rows across the filter setting, the profile batch, a forced
survivor split, a loaded, grown and shrunk index and device pointers; the capacity protocol, every refusal, the family
scan around it, and the chain compare -> layout -> family chain over the gapped planted motif."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import pssm_chain_ref as ref, pssm_family_ref as fam, pssm_ref, seqmatch_ref

pytestmark = pytest.mark.gpu

K, A = 25, 20
ALL = -1e300      # a threshold every window passes
PEN = dict(gap_open=4.0, gap_ext=1.0)


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
    """The proteins of seqmatch_ref.make_proteins (0, fewer than k, exactly k, 300 residues), 33 profiles with dyadic and
    real entries, thresholds that a thirtieth of the windows reach (profile 7: a quarter; profile 5: none), their
    reference hits, and the reference chains per configuration -- each computed once."""
    if not _CASE:
        P = seqmatch_ref.make_proteins(K)
        codes, id_start = _windows(P["db"], P["db_start"])
        n = len(codes)
        rng = np.random.default_rng(1000 * K + n)
        S = rng.normal(0, 2, size=(33, K, A))
        S[::2] = rng.integers(-16, 17, size=S[::2].shape) / 4.0      # dyadic entries: equal scores are common
        S[3, :, 0] = -1e30                                           # a forbidden residue
        S[12] = S[11] = rng.integers(-1, 2, size=S[11].shape) / 2.0  # coarse and twice: ties between two profiles
        sc = pssm_ref.scores(S, codes)
        t = np.sort(sc, axis=1)[:, -max(1, n // 30)].copy()
        t[5] = sc[5].max() + 1e3                                     # dead
        t[7] = np.sort(sc[7])[-n // 4]
        t[11] = t[12] = np.sort(sc[11])[-n // 4]
        hit = sc >= t[:, None]
        m, i = np.nonzero(hit)
        hits = dict(m=m.astype(np.uint32), id=i.astype(np.uint32), score=sc[m, i])
        _CASE.update(P=P, codes=codes, id_start=id_start, S=S, t=t, hits=hits, n=n, want={})
    return _CASE


def _layout(nm, groups):
    m_group = fam.group_layouts(nm)[groups]
    return m_group, ref.sorted_offsets(m_group, nm, K)


def _want(case, nm, groups, max_shift, **kw):
    key = (nm, groups, max_shift, tuple(sorted((k, np.asarray(v).tobytes()) for k, v in kw.items())))
    if key not in case["want"]:
        keep = case["hits"]["m"] < nm
        m_group, m_off = _layout(nm, groups)
        h = case["hits"]
        case["want"][key] = ref.chains_from_hits(h["m"][keep], h["id"][keep], h["score"][keep], nm, case["id_start"],
                                                 m_group, m_off, max_shift, **kw)
    return case["want"][key]


@pytest.fixture(scope="module")
def prot():
    case = _proteins()
    eng = _engine()
    info, _ = eng.index_build_windows(case["P"]["db"], case["P"]["db_start"])
    assert info["n"] == case["n"] == int(case["id_start"][-1]) and 1500 < case["n"] < 5000
    yield dict(case, eng=eng)
    eng.close()


def _chain(eng, case, nm, groups, max_shift, **kw):
    m_group, m_off = _layout(nm, groups)
    return eng.pssm_family_chain(case["S"][:nm], case["t"][:nm], case["id_start"], m_group, m_off, max_shift, **kw)


@pytest.mark.parametrize("nm", [1, 17, 33])
@pytest.mark.parametrize("groups", ["singletons", "one", "mixed"])
def test_chains_equal_the_rule(prot, nm, groups):
    eng = prot["eng"]
    listed = eng.pssm_scan(prot["S"][:nm], prot["t"][:nm])
    m_group, m_off = _layout(nm, groups)
    for max_shift in (0, 3, 65535):
        want = _want(prot, nm, groups, max_shift, **PEN)
        got = _chain(eng, prot, nm, groups, max_shift, **PEN)
        ref.same_chains(got, want, (nm, groups, max_shift))
        p = eng.profile()
        assert p["pssm_chain_segs"] == want["all_segs"] == p["pssm_chain_kept"] == len(want["group"])
        assert p["hits"] == want["n_hits"] and p["pssm_fam_rows"] == 0
        # the list call on the same handle, reduced by the host rule, is the same rows
        host = capi.pssm_family_chain_hits(listed["m"], listed["id"], listed["score"], nm, prot["id_start"], m_group,
                                           m_off, max_shift, **PEN)
        ref.same_chains(host, got, "list")
        if groups == "one" and nm > 1 and max_shift:
            assert (got["gaps"] > 0).any() and (got["count"] > 2).any() and (got["shift"] != 0).any()
        if max_shift == 0:
            assert np.all(got["gaps"] == 0) and np.all(got["shift"] == 0)


def test_segment_sizes_cross_the_tile_and_lds_edges():
    """Everything hits.  Group 0 is one profile: its segments hold as many hits as the protein has windows -- 1, 63, 64,
    65, 85, 129, 256, 257 and 1700, one run each, the last ones longer than a wave.  Group 1 is three profiles: three
    times as many -- 255 and 768 on either side of the LDS limit, about 5000 in the largest."""
    wins = [1, 63, 64, 65, 85, 129, 256, 257, 1700]
    rng = np.random.default_rng(21)
    lens = np.array([w + K - 1 for w in wins])
    residues = rng.integers(0, A, size=int(lens.sum())).astype(np.uint8)
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    codes, id_start = _windows(residues, seq_start)
    assert np.diff(id_start.astype(np.int64)).tolist() == wins
    S = rng.integers(-8, 9, size=(4, K, A)) / 4.0
    S[2] = rng.normal(0, 1, size=(K, A))
    t = np.full(4, ALL)
    m_group = np.array([0, 1, 1, 1], np.uint32)
    m_off = np.array([0, 0, 2, 5], np.uint32)
    hits = pssm_ref.scan(S, t, codes)
    eng = _engine()
    try:
        eng.index_build_windows(residues, seq_start)
        for max_shift, pen in ((3, PEN), (0, PEN), (40, dict(gap_open=0.5, gap_ext=2.0 ** -20))):
            want = ref.chains(hits, 4, id_start, m_group, m_off, max_shift, **pen)
            got = eng.pssm_family_chain(S, t, id_start, m_group, m_off, max_shift, **pen)
            ref.same_chains(got, want, ("sizes", max_shift))
            assert len(got["group"]) == 2 * len(wins) and eng.profile()["pssm_chain_segs"] == 2 * len(wins)
            assert got["cnt"].tolist() == [sum(wins)] * 4 and got["grp_rows"].tolist() == [len(wins)] * 2
            assert np.all(got["count"][got["group"] == 0] == 1)
        assert (got["count"] == 3).sum() >= 5 and (got["gaps"] > 0).any()
    finally:
        eng.close()


def test_a_family_of_40_levels():
    """40 profiles in one family at offsets 0, 2, 4, ..., everything hits, proteins of 50 and 7 windows: 40 runs in a
    segment of 2000 hits, and chains longer than any one tile of lanes sees at once."""
    rng = np.random.default_rng(23)
    lens = np.array([50 + K - 1, 7 + K - 1])
    residues = rng.integers(0, A, size=int(lens.sum())).astype(np.uint8)
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    codes, id_start = _windows(residues, seq_start)
    nm = 40
    S = rng.integers(-8, 9, size=(nm, K, A)) / 4.0 + 0.25            # a positive drift: long chains pay
    t = np.full(nm, ALL)
    m_group = np.zeros(nm, np.uint32)
    m_off = (2 * np.arange(nm)).astype(np.uint32)
    hits = pssm_ref.scan(S, t, codes)
    eng = _engine()
    try:
        eng.index_build_windows(residues, seq_start)
        for max_shift in (0, 2, 65535):
            want = ref.chains(hits, nm, id_start, m_group, m_off, max_shift, gap_open=1.0, gap_ext=0.5, min_count=2)
            got = eng.pssm_family_chain(S, t, id_start, m_group, m_off, max_shift, gap_open=1.0, gap_ext=0.5, min_count=2)
            ref.same_chains(got, want, ("levels", max_shift))
            assert len(got["seq"]) == 2
        assert got["count"].max() >= 20
    finally:
        eng.close()


def test_filters(prot):
    eng, nm = prot["eng"], 33
    base = _want(prot, nm, "mixed", 3, **PEN)
    n_groups = int(fam.group_layouts(nm)["mixed"].max()) + 1
    for min_count in (1, 2, 3):
        want = _want(prot, nm, "mixed", 3, min_count=min_count, **PEN)
        got = _chain(eng, prot, nm, "mixed", 3, min_count=min_count, **PEN)
        ref.same_chains(got, want, min_count)
        p = eng.profile()
        assert p["pssm_chain_segs"] == base["all_segs"] and p["pssm_chain_kept"] == len(want["group"]) == got["grp_rows"].sum()
        assert np.all(got["count"] >= min_count)
    assert 0 < len(_want(prot, nm, "mixed", 3, min_count=3, **PEN)["group"]) < len(base["group"])
    # a threshold per group: exactly at a chain's score the row stays, at the next double above it goes
    g = int(np.bincount(base["group"]).argmax())
    s = float(np.sort(base["score"][base["group"] == g])[-3])
    t_group = np.full(n_groups, -1e300)
    t_group[g] = s
    at = _chain(eng, prot, nm, "mixed", 3, t_group=t_group, **PEN)
    ref.same_chains(at, _want(prot, nm, "mixed", 3, t_group=t_group, **PEN), "at the score")
    assert (at["score"][at["group"] == g] == s).any()
    t_group[g] = np.nextafter(s, np.inf)
    above = _chain(eng, prot, nm, "mixed", 3, t_group=t_group, **PEN)
    ref.same_chains(above, _want(prot, nm, "mixed", 3, t_group=t_group, **PEN), "above the score")
    assert not (above["score"][above["group"] == g] == s).any() and above["grp_rows"][g] < at["grp_rows"][g]
    assert np.array_equal(above["cnt"], base["cnt"]) and above["n_hits"] == base["n_hits"]     # the scan's, unfiltered


def test_filter_and_batches_do_not_show(prot):
    eng = prot["eng"]
    want = _want(prot, 33, "mixed", 3, min_count=2, **PEN)
    try:
        for filt in (1, 0):
            eng.set_option("pssm_filter", filt)
            for batch in (1, 16, 0):
                eng.set_option("query_batch", batch)
                ref.same_chains(_chain(eng, prot, 33, "mixed", 3, min_count=2, **PEN), want, (filt, batch))
                p = eng.profile()
                if batch == 1:      # groups of 1, 2, 3, 5 are each a batch: no group is cut
                    assert p["verify_launches"] >= len(np.unique(fam.group_layouts(33)["mixed"]))
                assert (p["pssm_survivors"] == 33 * prot["n"]) == (filt == 0)
    finally:
        eng.set_option("pssm_filter", 1)
        eng.set_option("query_batch", 0)


def test_forced_split_and_changed_indexes(prot, monkeypatch, tmp_path):
    """The TEST build reports a survivor-counter overflow for every batch of more than 4 profiles: with groups of at
    most 4 the rows are the same (from a saved and loaded index); a group of 6 cannot be cut: HS_ERR_CAPACITY, nothing
    written.  Then the same rows after the index grew by appended k-mers and shrank again."""
    nm = 33
    m_group = np.repeat(np.arange(nm), np.resize([1, 2, 3, 4], nm))[:nm].astype(np.uint32)
    m_off = ref.sorted_offsets(m_group, nm, K)
    h = prot["hits"]
    kw = dict(min_count=2, **PEN)
    want = ref.chains(h, nm, prot["id_start"], m_group, m_off, 3, **kw)
    path = tmp_path / "p.idx"
    prot["eng"].index_save(path)
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "4")
    eng = _engine(hooks=True)
    try:
        eng.index_load(path)
        ref.same_chains(eng.pssm_family_chain(prot["S"], prot["t"], prot["id_start"], m_group, m_off, 3, **kw), want,
                        "split, loaded")
        assert eng.profile()["verify_launches"] >= 9
        # a group of 6
        six = np.array([0, 1, 1, 1, 1, 1, 1, 2], dtype=np.uint32)
        out = [np.full(50, 9, dtype=t) for _, t in capi.PSSM_CHAIN_FIELDS]
        cnt, grp = np.full(8, 9, np.uint64), np.full(3, 9, np.uint64)
        n_out, n_hits = C.c_uint64(5), C.c_uint64(5)
        zeros = np.zeros(8, np.uint32)
        st = eng._lib.hs_pssm_family_chain(eng._h, capi._vp(prot["S"][:8]), capi._vp(prot["t"][:8]), 8, capi._vp(six), 3,
                                           capi._vp(zeros), capi._vp(prot["id_start"]), len(prot["id_start"]) - 1, 3,
                                           4.0, 1.0, 1, None, *[capi._vp(a) for a in out], 50, C.byref(n_out),
                                           C.byref(n_hits), capi._vp(cnt), capi._vp(grp))
        assert st == capi.HS_ERR_CAPACITY and n_out.value == 0
        assert b"one group" in eng._lib.hs_last_error(eng._h)
        assert all(np.all(a == 9) for a in out) and np.all(cnt == 9) and np.all(grp == 9)
        # the index grown by 100 k-mers (a further sequence) and shrunk by the first sequence that has windows
        extra = np.random.default_rng(8).integers(0, A, size=(100, K)).astype(np.uint8)
        eng.index_append(extra)
        ids2 = np.concatenate([prot["id_start"], [prot["n"] + 100]]).astype(np.uint64)
        codes2 = np.concatenate([prot["codes"], extra])
        hits2 = pssm_ref.scan(prot["S"], prot["t"], codes2)
        ref.same_chains(eng.pssm_family_chain(prot["S"], prot["t"], ids2, m_group, m_off, 3, **kw),
                        ref.chains(hits2, nm, ids2, m_group, m_off, 3, **kw), "appended")
        s0 = int(np.flatnonzero(np.diff(ids2.astype(np.int64)) > 5)[0])
        gone = np.arange(int(ids2[s0]), int(ids2[s0 + 1]), dtype=np.uint32)
        eng.index_remove(gone)
        ids3 = ids2.copy()
        ids3[s0 + 1:] -= np.uint64(len(gone))
        codes3 = np.delete(codes2, gone, axis=0)
        hits3 = pssm_ref.scan(prot["S"], prot["t"], codes3)
        ref.same_chains(eng.pssm_family_chain(prot["S"], prot["t"], ids3, m_group, m_off, 3, **kw),
                        ref.chains(hits3, nm, ids3, m_group, m_off, 3, **kw), "removed")
    finally:
        eng.close()


def _dev_rows(torch, cap, fill=7):
    return [torch.full((cap,), fill, dtype=torch.float64 if t == np.float64 else torch.int32, device="cuda")
            for _, t in capi.PSSM_CHAIN_FIELDS]


def _dev_dict(rows, n, dc, dg, nh):
    got = {name: r[:n].cpu().numpy().astype(t) for (name, t), r in zip(capi.PSSM_CHAIN_FIELDS, rows)}
    got["n_hits"] = nh
    if dc is not None:
        got.update(cnt=dc.cpu().numpy().astype(np.uint64), grp_rows=dg.cpu().numpy().astype(np.uint64))
    return got


def test_device_pointers_capacity_and_refusals(prot):
    import torch
    eng, nm = prot["eng"], 33
    m_group, m_off = _layout(nm, "mixed")
    n_groups = int(m_group.max()) + 1
    loose = _want(prot, nm, "mixed", 3, min_count=2, **PEN)
    t_group = np.full(n_groups, float(np.median(loose["score"])))
    want = _want(prot, nm, "mixed", 3, min_count=2, t_group=t_group, **PEN)
    n_rows = len(want["group"])
    assert 0 < n_rows < len(loose["group"])
    dS, dt = torch.from_numpy(prot["S"]).cuda(), torch.from_numpy(prot["t"]).cuda()
    dI = torch.from_numpy(prot["id_start"].astype(np.int64)).cuda()
    dG = torch.from_numpy(m_group.astype(np.int32)).cuda()
    dO = torch.from_numpy(m_off.astype(np.int32)).cuda()
    dT = torch.from_numpy(t_group).cuda()
    n_seq = len(prot["id_start"]) - 1
    cap = n_rows + 5
    rows = _dev_rows(torch, cap)
    dc = torch.full((nm,), 7, dtype=torch.int64, device="cuda")
    dg = torch.full((n_groups,), 7, dtype=torch.int64, device="cuda")
    ptrs = [r.data_ptr() for r in rows]

    def call(S=dS, t=dt, G=dG, ng=n_groups, O=dO, I=dI, ns=n_seq, ms=3, go=4.0, ge=1.0, mc=2, T=dT, p=ptrs, c=cap,
             counts=True):
        torch.cuda.synchronize()
        return eng.pssm_family_chain_dev(S.data_ptr(), t.data_ptr(), nm, G.data_ptr() if G is not None else 0, ng,
                                         O.data_ptr() if O is not None else 0, I.data_ptr() if I is not None else 0, ns,
                                         ms, go, ge, mc, T.data_ptr() if T is not None else 0, p, c,
                                         dc.data_ptr() if counts else 0, dg.data_ptr() if counts else 0)

    n, nh = call()
    assert n == n_rows
    ref.same_chains(_dev_dict(rows, n, dc, dg, nh), want, "dev")
    assert all(float(r[n]) == 7 for r in rows)
    p = eng.profile()
    assert p["pssm_chain_kept"] == n_rows and p["pssm_chain_segs"] == loose["all_segs"]
    # cnt and grp_rows NULL: the same rows
    for r in rows:
        r.fill_(7)
    dc.fill_(9), dg.fill_(9)
    n, nh = call(counts=False)
    ref.same_chains(_dev_dict(rows, n, None, None, nh), want, "dev, no counts")
    assert bool((dc == 9).all()) and bool((dg == 9).all())
    host = eng.pssm_family_chain(prot["S"], prot["t"], prot["id_start"], m_group, m_off, 3, min_count=2, t_group=t_group,
                                 want_counts=False, **PEN)
    ref.same_chains(host, want, "host, no counts")
    assert "cnt" not in host
    # the two-call pattern: the count with null arrays, then too small by one -- counts valid, no row written
    with pytest.raises(HsError) as e:
        call(p=[0] * 10, c=0)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == n_rows and e.value.n_hits == want["n_hits"]
    assert np.array_equal(dc.cpu().numpy().astype(np.uint64), want["cnt"])
    assert np.array_equal(dg.cpu().numpy().astype(np.uint64), want["grp_rows"])
    for r in rows:
        r.fill_(9)
    dc.fill_(9), dg.fill_(9)
    with pytest.raises(HsError) as e:
        call(c=n_rows - 1)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == n_rows
    assert all(bool((r == 9).all()) for r in rows)
    assert np.array_equal(dg.cpu().numpy().astype(np.uint64), want["grp_rows"])
    kw = dict(min_count=2, t_group=t_group, **PEN)
    with pytest.raises(HsError) as e:     # the host form
        eng.pssm_family_chain(prot["S"], prot["t"], prot["id_start"], m_group, m_off, 3, cap=n_rows - 1, **kw)
    assert e.value.needed == n_rows and e.value.n_hits == want["n_hits"]
    assert np.array_equal(e.value.cnt, want["cnt"]) and np.array_equal(e.value.grp_rows, want["grp_rows"])
    ref.same_chains(eng.pssm_family_chain(prot["S"], prot["t"], prot["id_start"], m_group, m_off, 3, cap=n_rows, **kw),
                    want, "exact cap")
    # refusals found on the device, before anything is written
    dc.fill_(9), dg.fill_(9)

    def refused(status=capi.HS_ERR_INVALID, **kw):
        with pytest.raises(HsError) as e:
            call(**kw)
        assert e.value.status == status, kw
        assert all(bool((r == 9).all()) for r in rows) and bool((dc == 9).all()) and bool((dg == 9).all())
        return str(e.value)

    refused(O=None)                                                       # m_off is required
    inside = int(np.flatnonzero(m_group[1:] == m_group[:-1])[0]) + 1      # a profile that is not its group's first
    O2 = dO.clone()
    O2[inside - 1], O2[inside] = 5, 4
    assert "decreases" in refused(O=O2)                                   # m_off decreases inside a group
    O2 = dO.clone()
    first = int(np.flatnonzero(m_group[1:] != m_group[:-1])[-1]) + 1      # across a group boundary it may fall
    O2[first - 1] = 100
    assert call(O=O2)[1] == want["n_hits"]
    for r in rows:
        r.fill_(9)
    dc.fill_(9), dg.fill_(9)
    refused(ms=65536)
    for bad in (float("nan"), float("inf"), -1.0):
        refused(go=bad)
        refused(ge=bad)
    for where, bad in (("S", float("nan")), ("S", 2.0 ** 101), ("t", float("nan")), ("t", float("-inf"))):
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
    G2 = dG.clone()
    G2[5], G2[6] = 3, 2                                                   # m_group decreases
    refused(G=G2)
    G2 = dG.clone()
    G2[nm - 1] = n_groups                                                 # a value >= n_groups
    refused(G=G2)
    refused(G=None)                                                       # n_groups != nm without m_group
    refused(mc=0)
    refused(ng=(1 << 32) + 1)
    for bad in (float("nan"), float("inf"), float("-inf")):
        T2 = dT.clone()
        T2[n_groups - 1] = bad
        refused(T=T2)
    O2 = dO.clone()
    O2[nm - 1] = -(1 << 31)                                               # the bits of 2^31: above 2^31 - 1
    refused(O=O2)
    refused(p=[0] + ptrs[1:])                                             # a null output with cap > 0
    # the host form: the same refusals, with sentinel-filled outputs untouched
    lib, h = eng._lib, eng._h
    out = [np.full(cap, 9, dtype=t) for _, t in capi.PSSM_CHAIN_FIELDS]
    cnt, grp = np.full(nm, 9, np.uint64), np.full(n_groups, 9, np.uint64)
    n_out, n_hits = C.c_uint64(5), C.c_uint64(5)

    def host(S=prot["S"], t=prot["t"], ids=prot["id_start"], ns=n_seq, nm_=nm, G=m_group, ng=n_groups, O=m_off, ms=3,
             go=4.0, ge=1.0, mc=2, T=t_group, outs=out):
        vp = lambda a: None if a is None else capi._vp(np.ascontiguousarray(a))
        keep = [np.ascontiguousarray(a) if a is not None else None for a in (S, t, G, O, ids, T)]
        st = lib.hs_pssm_family_chain(h, capi._vp(keep[0]), capi._vp(keep[1]), C.c_uint64(nm_), vp(keep[2]), ng,
                                      vp(keep[3]), vp(keep[4]), C.c_uint64(ns), ms, go, ge, mc, vp(keep[5]),
                                      *[vp(a) for a in outs], cap, C.byref(n_out), C.byref(n_hits), capi._vp(cnt),
                                      capi._vp(grp))
        assert n_out.value == 0 and n_hits.value == 0
        assert all(np.all(a == 9) for a in out) and np.all(cnt == 9) and np.all(grp == 9)
        return st

    def changed(a, at, value):
        c = a.copy()
        c[at] = value
        return c

    S2 = prot["S"].copy()
    S2[1, 2, 3] = np.nan
    ids = prot["id_start"]
    bad = capi.HS_ERR_INVALID
    assert host(O=None) == bad
    assert host(O=changed(changed(m_off, inside - 1, 5), inside, 4)) == bad          # decreases inside a group
    assert b"decreases" in lib.hs_last_error(h)
    assert host(ms=65536) == bad
    for x in (np.nan, np.inf, -np.inf, -1.0):
        assert host(go=x) == bad and host(ge=x) == bad
    assert host(S=S2) == bad
    assert host(t=np.where(np.arange(nm) == 4, np.inf, prot["t"])) == bad
    assert host(nm_=1 << 27) == bad
    assert host(ids=None) == bad
    assert host(ids=changed(ids, 30, int(ids[31]) + 1)) == bad           # does not ascend
    assert host(ids=changed(ids, 0, 1)) == bad                           # does not start at 0
    assert host(ids=changed(ids, n_seq, int(ids[-1]) + 1)) == bad        # does not end at n
    assert host(ns=0) == bad
    assert host(G=changed(m_group, 5, m_group[4] + 2)) == bad            # m_group decreases behind it
    assert host(G=changed(m_group, nm - 1, n_groups)) == bad
    assert host(G=None) == bad
    assert host(mc=0) == bad
    assert host(T=changed(t_group, 0, np.nan)) == bad and host(T=changed(t_group, 1, -np.inf)) == bad
    assert host(O=changed(m_off, nm - 1, 1 << 31)) == bad
    assert host(outs=out[:4] + [None] + out[5:]) == bad
    # nm = 0 is an empty, successful call
    empty = eng.pssm_family_chain(np.zeros((0, K, A)), np.zeros(0), prot["id_start"], None, np.zeros(0, np.uint32), 3)
    assert len(empty["group"]) == 0 and empty["n_hits"] == 0
    unbuilt = _engine()
    try:
        with pytest.raises(HsError) as e:
            unbuilt.pssm_family_chain(prot["S"], prot["t"], prot["id_start"], m_group, m_off, 3)
        assert e.value.status == capi.HS_ERR_STATE
    finally:
        unbuilt.close()


def test_a_family_of_4097_is_refused():
    """A group of 4097 profiles through the device-pointer form (whose value checks run on the device) and the host
    form, on sentinel-filled outputs; 4096 profiles pass."""
    import torch
    codes = np.random.default_rng(2).integers(0, A, size=(64, K)).astype(np.uint8)
    eng = _engine(codes=codes)
    try:
        nm = 4097
        S, t = np.zeros((nm, K, A)), np.full(nm, 1.0)           # (no window reaches 1: the passing calls find nothing)
        ids = np.array([0, 40, 64], dtype=np.uint64)
        zeros = np.zeros(nm, np.uint32)
        dS, dt = torch.from_numpy(S).cuda(), torch.from_numpy(t).cuda()
        dI = torch.from_numpy(ids.astype(np.int64)).cuda()
        dG = torch.zeros(nm, dtype=torch.int32, device="cuda")
        rows = _dev_rows(torch, 8, fill=9)
        ptrs = [r.data_ptr() for r in rows]
        dc = torch.full((nm,), 9, dtype=torch.int64, device="cuda")
        dg = torch.full((1,), 9, dtype=torch.int64, device="cuda")

        def dev(nm_):
            torch.cuda.synchronize()
            return eng.pssm_family_chain_dev(dS.data_ptr(), dt.data_ptr(), nm_, dG.data_ptr(), 1, dG.data_ptr(),
                                             dI.data_ptr(), 2, 3, 4.0, 1.0, 1, 0, ptrs, 8, dc.data_ptr(), dg.data_ptr())

        with pytest.raises(HsError) as e:
            dev(4097)
        assert e.value.status == capi.HS_ERR_INVALID and "4096" in str(e.value)
        assert all(bool((r == 9).all()) for r in rows) and bool((dc == 9).all()) and bool((dg == 9).all())
        assert dev(4096) == (0, 0) and bool((dc[:4096] == 0).all()) and int(dc[4096]) == 9 and int(dg[0]) == 0
        with pytest.raises(HsError) as e:
            eng.pssm_family_chain(S, t, ids, zeros, zeros, 3)
        assert e.value.status == capi.HS_ERR_INVALID and "4096" in str(e.value)
        got = eng.pssm_family_chain(S[:4096], t[:4096], ids, zeros[:4096], zeros[:4096], 3)
        assert len(got["group"]) == 0 and got["n_hits"] == 0
    finally:
        eng.close()


def test_the_family_scan_around_it(prot):
    """hs_pssm_family_scan, hs_pssm_scan and hs_pssm_seq_scan on the same handle give what they gave."""
    eng = prot["eng"]
    S, t, ids = prot["S"][:17], prot["t"][:17], prot["id_start"]
    m_group, m_off = _layout(17, "mixed")

    def others():
        return (eng.pssm_family_scan(S, t, ids, m_group=m_group, m_off=m_off, min_count=2), eng.pssm_scan(S, t),
                eng.pssm_seq_scan(S, t, ids))

    before = others()
    assert eng.profile()["pssm_chain_segs"] == 0
    ref.same_chains(_chain(eng, prot, 17, "mixed", 3, **PEN), _want(prot, 17, "mixed", 3, **PEN), "between")
    after = others()
    for x, y in zip(before, after):
        assert x.keys() == y.keys()
        for f in x:
            assert np.array_equal(x[f], y[f]), f
    assert len(before[0]["group"]) > 0 and len(before[1]["m"]) > 0


@pytest.mark.parametrize("ins", [1, 3])
def test_gapped_planted_motif_end_to_end(ins):
    """compare -> layout -> family chain over the gapped planted motif of tests/pssm_chain_ref.py (seed 20261; the
    construction is checked on the reference by tests/test_pssm_chain_cpu.py): the family rows with min_count = 3 lose
    the four proteins with an insertion, the chain at max_shift = 3 reports all nine at the planted offset."""
    c = ref.planted_gapped(ins=ins)
    eng = _engine()
    try:
        info, _ = eng.index_build_windows(c["residues"], c["seq_start"])
        assert info["n"] == len(c["codes"])
        h = eng.pssm_compare(capi.pssm_compare_columns(c["S"], "pearson"), 10.0, None, 13)
        lay = capi.pssm_family_layout(h["x"], h["y"], h["d"], 3)
        assert lay["n_groups"] == 1 and lay["n_conflicts"] == 0 and lay["off"].tolist() == c["shifts"].tolist()
        order = lay["order"]
        args = (c["S"][order], c["t"][order], c["id_start"])
        g, off = lay["group"][order], lay["off"][order]
        rows = eng.pssm_family_scan(*args, m_group=g, m_off=off, min_count=3)
        assert rows["seq"].tolist() == list(ref.PLANTED_UNGAPPED)
        got = eng.pssm_family_chain(*args, g, off, 3, min_count=3, **PEN)
        hits = pssm_ref.scan(c["S"], c["t"], c["codes"])
        ref.same_chains(got, ref.chains(hits, 3, c["id_start"], g, off, 3, min_count=3, **PEN), "planted")
        assert got["seq"].tolist() == sorted(c["planted"]) and np.all(got["count"] == 3)
        assert (got["first_id"] - c["id_start"][got["seq"]]).tolist() == [c["planted"][s] for s in got["seq"].tolist()]
        gapped = np.isin(got["seq"], ref.PLANTED_GAPPED)
        assert np.all(got["shift"][gapped] == ins) and np.all(got["gaps"][gapped] == 1)
        assert np.all(got["shift"][~gapped] == 0) and np.all(got["gaps"][~gapped] == 0)
        less = eng.pssm_family_chain(*args, g, off, ins - 1, min_count=3, **PEN)
        assert less["seq"].tolist() == list(ref.PLANTED_UNGAPPED)
        zero = eng.pssm_family_chain(*args, g, off, 0, min_count=3, **PEN)
        assert np.array_equal(zero["score"].view(np.uint64), rows["sum"].view(np.uint64))
    finally:
        eng.close()
