"""hs_pssm_family_scan on the GPU against the host rule (capi.pssm_family_hits over the same handle's pssm_scan) and
the numpy contract of tests/pssm_family_ref.py over tests/pssm_ref.py's scan: every array bit for bit -- over every
group layout with and without offsets, rows of 70, 300 and 1000 hits, an order of the sum that shows, ties, sequence
boundaries, the filters at their edge; identical rows across the filter setting, the profile batch, a forced survivor
split, a loaded, grown and shrunk index and device pointers; the capacity protocol, every refusal, the handle's other
calls around it, and the chain compare -> layout -> family scan over a planted motif."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import pssm_family_ref as ref, pssm_ref, pssm_seq_ref, seqmatch_ref

pytestmark = pytest.mark.gpu

K, A = 25, 20
ALL = -1e300      # a threshold every window passes


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
    """The proteins of seqmatch_ref.make_proteins (0, fewer than k, exactly k, 300 residues), 33 profiles of mixed
    kinds, their reference hits, and the reference rows per (nm, layout, offsets) -- each computed once."""
    if not _CASE:
        P = seqmatch_ref.make_proteins(K)
        codes, id_start = _windows(P["db"], P["db_start"])
        n = len(codes)
        rng = np.random.default_rng(1000 * K + n)
        S = rng.normal(0, 2, size=(33, K, A))
        S[::2] = rng.integers(-16, 17, size=S[::2].shape) / 4.0      # dyadic entries: equal scores are common
        S[3, :, 0] = -1e30                                           # a forbidden residue
        S[11] = rng.integers(-1, 2, size=S[11].shape) / 2.0          # very coarse: the best of a row is often tied
        S[12] = S[11]                                                # ... and tied between two profiles
        sc = pssm_ref.scores(S, codes)
        t = np.sort(sc, axis=1)[:, -max(1, n // 30)].copy()          # an attained score: about a thirtieth hit
        t[5] = sc[5].max() + 1e3                                     # dead
        t[7] = -1e6                                                  # everything hits
        t[9] = sc[9].max()                                           # attained by (almost surely) one window
        t[11] = t[12] = np.sort(sc[11])[-n // 4]
        hit = sc >= t[:, None]
        m, i = np.nonzero(hit)
        hits = dict(m=m.astype(np.uint32), id=i.astype(np.uint32), score=sc[m, i])
        _CASE.update(P=P, codes=codes, id_start=id_start, S=S, t=t, hits=hits, n=n, want={})
    return _CASE


def _layout(nm, groups, with_off):
    m_group = ref.group_layouts(nm)[groups]
    return m_group, (ref.offsets_in_groups(m_group, nm, K) if with_off else None)


def _want(case, nm, groups="singletons", with_off=False, **kw):
    key = (nm, groups, with_off, tuple(sorted((k, np.asarray(v).tobytes()) for k, v in kw.items())))
    if key not in case["want"]:
        keep = case["hits"]["m"] < nm
        m_group, m_off = _layout(nm, groups, with_off)
        h = case["hits"]
        case["want"][key] = ref.rows_from_hits(h["m"][keep], h["id"][keep], h["score"][keep], nm, case["id_start"],
                                               m_group=m_group, m_off=m_off, **kw)
    return case["want"][key]


@pytest.fixture(scope="module")
def prot():
    case = _proteins()
    eng = _engine()
    info, _ = eng.index_build_windows(case["P"]["db"], case["P"]["db_start"])
    assert info["n"] == case["n"] == int(case["id_start"][-1]) and 1500 < case["n"] < 5000
    yield dict(case, eng=eng)
    eng.close()


def _scan(eng, case, nm, groups="singletons", with_off=False, **kw):
    m_group, m_off = _layout(nm, groups, with_off)
    return eng.pssm_family_scan(case["S"][:nm], case["t"][:nm], case["id_start"], m_group=m_group, m_off=m_off, **kw)


@pytest.mark.parametrize("nm", [1, 17, 33])
@pytest.mark.parametrize("groups", ["singletons", "one", "mixed"])
def test_rows_equal_the_rule(prot, nm, groups):
    eng = prot["eng"]
    listed = eng.pssm_scan(prot["S"][:nm], prot["t"][:nm])
    for with_off in (False, True):
        want = _want(prot, nm, groups, with_off)
        got = _scan(eng, prot, nm, groups, with_off)
        ref.same_rows(got, want, (nm, groups, with_off))
        p = eng.profile()
        assert p["pssm_fam_rows"] == p["pssm_fam_kept"] == len(want["group"]) == want["all_rows"]
        assert p["hits"] == want["n_hits"] == int(got["count"].sum())
        # the list call on the same handle, reduced by the host rule, is the same rows
        m_group, m_off = _layout(nm, groups, with_off)
        host = capi.pssm_family_hits(listed["m"], listed["id"], listed["score"], nm, prot["id_start"], m_group=m_group,
                                     m_off=m_off)
        ref.same_rows(host, got, "list")
        if with_off and nm > 1:
            assert (got["diag"] < 0).any() and (got["diag"] > 0).any()
        if groups != "singletons" and nm > 1 and with_off is False:
            assert (np.diff(got["best_m"].astype(np.int64)) < 0).any()      # rows are not in profile order


def test_without_groups_it_is_the_sequence_scan(prot):
    eng = prot["eng"]
    got = eng.pssm_family_scan(prot["S"], prot["t"], prot["id_start"])
    seq = eng.pssm_seq_scan(prot["S"], prot["t"], prot["id_start"])
    for mine, theirs in (("group", "m"), ("seq", "seq"), ("count", "count"), ("best_id", "best_id"), ("lo", "lo"),
                         ("hi", "hi")):
        assert np.array_equal(got[mine], seq[theirs]), mine
    assert np.array_equal(got["best_score"].view(np.uint64), seq["best_score"].view(np.uint64))
    assert np.array_equal(got["best_m"], seq["m"]) and np.all(got["diag"] == 0)
    assert np.array_equal(got["cnt"], seq["cnt"]) and np.array_equal(got["grp_rows"], seq["seq_cnt"])
    assert np.array_equal(got["sum"].view(np.uint64), _want(prot, 33)["sum"].view(np.uint64)) and got["n_hits"] == seq["n_hits"]


def test_long_rows():
    """Rows of 70 and of 300 hits (two groups at a common offset, everything hits, one sequence), and one row of 1000
    hits (one profile without diagonals over one sequence of 1000 windows)."""
    rng = np.random.default_rng(11)
    residues = rng.integers(0, A, size=1000 + K - 1).astype(np.uint8)
    seq_start = np.array([0, len(residues)], dtype=np.uint64)
    codes, id_start = _windows(residues, seq_start)
    S = rng.integers(-8, 9, size=(370, K, A)) / 4.0
    S[100:200] = rng.normal(0, 1, size=(100, K, A))                   # full mantissas inside the group of 300
    m_group = np.repeat([0, 1], [70, 300]).astype(np.uint32)
    eng = _engine()
    try:
        eng.index_build_windows(residues, seq_start)
        want = ref.rows(pssm_ref.scan(S[:1], np.full(1, ALL), codes), 1, id_start)
        assert want["count"].tolist() == [1000] and want["lo"].tolist() == [0] and want["hi"].tolist() == [999]
        ref.same_rows(eng.pssm_family_scan(S[:1], np.full(1, ALL), id_start), want, "1000")
    finally:
        eng.close()
    eng = _engine(codes=codes[:40])     # 40 windows: rows of 70 and of 300 on every diagonal
    try:
        ids = np.array([0, 40], dtype=np.uint64)
        t = np.full(370, ALL)
        m_off = np.full(370, 7, dtype=np.uint32)
        want = ref.rows(pssm_ref.scan(S, t, codes[:40]), 370, ids, m_group=m_group, m_off=m_off)
        assert want["count"].tolist() == [70] * 40 + [300] * 40 and want["diag"].min() == -7
        got = eng.pssm_family_scan(S, t, ids, m_group=m_group, m_off=m_off)
        ref.same_rows(got, want, "70 and 300")
        assert got["grp_rows"].tolist() == [40, 40]
    finally:
        eng.close()


def test_the_order_of_the_sum():
    """Profiles scaled by 2^40, 1 and 2^-12 inside one group (tests/test_pssm_family_cpu.py shows that the reversed order
    changes the bits): the device's sums are those of the ascending (m, id) order."""
    rng = np.random.default_rng(3)
    codes = rng.integers(0, A, size=(300, K)).astype(np.uint8)
    S = ref.order_sensitive_profiles(K, A)
    t = np.full(3, ALL)
    id_start = np.array([0, 300], dtype=np.uint64)
    kw = dict(m_group=np.zeros(3, np.uint32), m_off=np.zeros(3, np.uint32))
    hits = pssm_ref.scan(S, t, codes)
    want = ref.rows(hits, 3, id_start, **kw)
    back = ref.rows(hits, 3, id_start, reverse_sum=True, **kw)
    assert (want["sum"].view(np.uint64) != back["sum"].view(np.uint64)).sum() >= 10
    eng = _engine(codes=codes)
    try:
        for batch in (0, 1):                   # (a batch below the group's size is raised to the group)
            eng.set_option("query_batch", batch)
            ref.same_rows(eng.pssm_family_scan(S, t, id_start, **kw), want, batch)
        # without diagonals: one row of 900 hits, summed over 300 ids of each profile in turn
        want = ref.rows(hits, 3, id_start, m_group=kw["m_group"])
        assert want["count"].tolist() == [900]
        ref.same_rows(eng.pssm_family_scan(S, t, id_start, m_group=kw["m_group"]), want, "900")
    finally:
        eng.close()


def test_ties(prot):
    """Profiles 11 and 12 are one coarse matrix: in one group the best of a row is tied between them (the smaller m
    wins) and, without diagonals, between ids of one profile (the smaller id wins)."""
    eng = prot["eng"]
    S, t = prot["S"][11:13], prot["t"][11:13]
    keep = (prot["hits"]["m"] == 11) | (prot["hits"]["m"] == 12)
    h = {f: v[keep] for f, v in prot["hits"].items()}
    for m_off in (None, np.zeros(2, np.uint32)):
        kw = dict(m_group=np.zeros(2, np.uint32), m_off=m_off)
        want = ref.rows_from_hits(h["m"] - 11, h["id"], h["score"], 2, prot["id_start"], **kw)
        ref.same_rows(eng.pssm_family_scan(S, t, prot["id_start"], **kw), want, "ties")
        assert np.all(want["best_m"] == 0) and np.all(want["count"] % 2 == 0)
        if m_off is None:
            tied = 0
            for r in range(len(want["seq"])):
                s = int(want["seq"][r])
                sel = (h["m"] == 11) & (h["score"] == want["best_score"][r])
                sel &= (h["id"] >= prot["id_start"][s]) & (h["id"] < prot["id_start"][s + 1])
                tied += int(sel.sum() > 1)
                assert want["best_id"][r] == h["id"][sel].min()
            assert tied >= 3


def test_sequence_boundaries(prot):
    """The everything-hits profile with an offset: sequences without ids have no row, every sequence with windows has
    a hit at its first and at its last window, and one diagonal in neighbouring sequences stays two rows.  n = 1."""
    eng = prot["eng"]
    S, t = prot["S"][7:8], prot["t"][7:8]
    wins = np.diff(prot["id_start"].astype(np.int64))
    assert (wins == 0).sum() >= 4 and (wins == 1).sum() >= 2
    m_off = np.array([2], dtype=np.uint32)
    keep = prot["hits"]["m"] == 7
    h = {f: v[keep] for f, v in prot["hits"].items()}
    want = ref.rows_from_hits(h["m"] * 0, h["id"], h["score"], 1, prot["id_start"], m_off=m_off)
    got = eng.pssm_family_scan(S, t, prot["id_start"], m_off=m_off)
    ref.same_rows(got, want, "boundaries")
    assert len(got["seq"]) == wins.sum() and np.all(got["count"] == 1)
    assert np.array_equal(np.unique(got["seq"]), np.flatnonzero(wins > 0))
    first = got["diag"] == -2
    assert first.sum() == (wins > 0).sum() and np.all(got["lo"][first] == 0)        # one row per sequence: not merged
    last = np.array([got["hi"][got["seq"] == s].max() for s in np.flatnonzero(wins > 0)])
    assert np.array_equal(last, wins[wins > 0] - 1)
    one = _engine(codes=prot["codes"][:1])
    try:
        ids = np.array([0, 0, 1, 1], dtype=np.uint64)
        got = one.pssm_family_scan(prot["S"][:4], np.full(4, ALL), ids, m_group=[0, 0, 1, 1], m_off=[0, 1, 0, 0])
        want = ref.rows(pssm_ref.scan(prot["S"][:4], np.full(4, ALL), prot["codes"][:1]), 4, ids, m_group=[0, 0, 1, 1],
                        m_off=[0, 1, 0, 0])
        ref.same_rows(got, want, "n = 1")
        assert got["seq"].tolist() == [1, 1, 1] and got["diag"].tolist() == [-1, 0, 0] and got["count"].tolist() == [1, 1, 2]
    finally:
        one.close()


def test_filters(prot):
    eng, nm = prot["eng"], 33
    base = _want(prot, nm, "mixed", True)
    sizes = np.bincount(ref.group_layouts(nm)["mixed"])
    for min_count in (1, 2, 3, 5):
        want = _want(prot, nm, "mixed", True, min_count=min_count)
        got = _scan(eng, prot, nm, "mixed", True, min_count=min_count)
        ref.same_rows(got, want, min_count)
        p = eng.profile()
        assert p["pssm_fam_rows"] == base["all_rows"] and p["pssm_fam_kept"] == len(want["group"]) == got["grp_rows"].sum()
        assert np.all(got["count"] >= min_count) and np.all(got["count"] <= sizes[got["group"]])
    assert 0 < len(_want(prot, nm, "mixed", True, min_count=3)["group"]) < len(base["group"])
    # a threshold per group: exactly at a row's sum the row stays, at the next double above it goes
    n_groups = len(sizes)
    g = int(np.bincount(base["group"]).argmax())
    rows_g = np.flatnonzero(base["group"] == g)
    s = float(np.sort(base["sum"][rows_g])[len(rows_g) // 2])
    t_group = np.full(n_groups, -1e300)
    t_group[g] = s
    at = _scan(eng, prot, nm, "mixed", True, t_group=t_group)
    ref.same_rows(at, _want(prot, nm, "mixed", True, t_group=t_group), "at the sum")
    assert (at["sum"][at["group"] == g] == s).any() and at["grp_rows"][g] == (base["sum"][rows_g] >= s).sum()
    t_group[g] = np.nextafter(s, np.inf)
    above = _scan(eng, prot, nm, "mixed", True, t_group=t_group)
    ref.same_rows(above, _want(prot, nm, "mixed", True, t_group=t_group), "above the sum")
    assert not (above["sum"][above["group"] == g] == s).any() and above["grp_rows"][g] == (base["sum"][rows_g] > s).sum()
    assert above["grp_rows"][g] < at["grp_rows"][g]
    other = np.arange(n_groups) != g
    assert np.array_equal(above["grp_rows"][other], base["grp_rows"][other])
    assert np.array_equal(above["cnt"], base["cnt"]) and above["n_hits"] == base["n_hits"]     # the scan's, unfiltered


def test_filter_and_batches_do_not_show(prot):
    eng = prot["eng"]
    want = _want(prot, 33, "mixed", True, min_count=2)
    surv = None
    try:
        for filt in (1, 0):
            eng.set_option("pssm_filter", filt)
            for batch in (1, 4, 0):
                eng.set_option("query_batch", batch)
                ref.same_rows(_scan(eng, prot, 33, "mixed", True, min_count=2), want, (filt, batch))
                p = eng.profile()
                if batch == 1:      # groups of 1, 2, 3, 5 are each a batch: no group is cut
                    assert p["verify_launches"] >= len(np.unique(ref.group_layouts(33)["mixed"]))
                s = p["pssm_survivors"]
                if filt:
                    surv = s if surv is None else surv
                    assert s == surv < 33 * prot["n"]
                else:
                    assert s == 33 * prot["n"]
    finally:
        eng.set_option("pssm_filter", 1)
        eng.set_option("query_batch", 0)


def test_forced_split_and_changed_indexes(prot, monkeypatch, tmp_path):
    """The TEST build reports a survivor-counter overflow for every batch of more than 4 profiles: with groups of at
    most 4 the rows are the same (from a saved and loaded index); a group of 6 cannot be cut: HS_ERR_CAPACITY, nothing
    written.  Then the same rows after the index grew by appended k-mers and shrank again."""
    nm = 33
    m_group = np.repeat(np.arange(nm), np.resize([1, 2, 3, 4], nm))[:nm].astype(np.uint32)
    m_off = ref.offsets_in_groups(m_group, nm, K)
    h = prot["hits"]
    want = ref.rows(h, nm, prot["id_start"], m_group=m_group, m_off=m_off, min_count=2)
    path = tmp_path / "p.idx"
    prot["eng"].index_save(path)
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "4")
    eng = _engine(hooks=True)
    try:
        eng.index_load(path)
        kw = dict(m_group=m_group, m_off=m_off, min_count=2)
        ref.same_rows(eng.pssm_family_scan(prot["S"], prot["t"], prot["id_start"], **kw), want, "split, loaded")
        assert eng.profile()["verify_launches"] >= 9
        # a group of 6
        six = np.array([0, 1, 1, 1, 1, 1, 1, 2], dtype=np.uint32)
        out = [np.full(50, 9, dtype=t) for _, t in capi.PSSM_FAMILY_FIELDS]
        cnt, grp = np.full(8, 9, np.uint64), np.full(3, 9, np.uint64)
        n_out, n_hits = C.c_uint64(5), C.c_uint64(5)
        st = eng._lib.hs_pssm_family_scan(eng._h, capi._vp(prot["S"][:8]), capi._vp(prot["t"][:8]), 8, capi._vp(six), 3,
                                          None, capi._vp(prot["id_start"]), len(prot["id_start"]) - 1, 1, None,
                                          *[capi._vp(a) for a in out], 50, C.byref(n_out), C.byref(n_hits),
                                          capi._vp(cnt), capi._vp(grp))
        assert st == capi.HS_ERR_CAPACITY and n_out.value == 0
        assert b"one group" in eng._lib.hs_last_error(eng._h)
        assert all(np.all(a == 9) for a in out) and np.all(cnt == 9) and np.all(grp == 9)
        # the index grown by 100 k-mers (a further sequence) and shrunk by the first sequence that has windows
        extra = np.random.default_rng(8).integers(0, A, size=(100, K)).astype(np.uint8)
        eng.index_append(extra)
        ids2 = np.concatenate([prot["id_start"], [prot["n"] + 100]]).astype(np.uint64)
        codes2 = np.concatenate([prot["codes"], extra])
        hits2 = pssm_ref.scan(prot["S"], prot["t"], codes2)
        ref.same_rows(eng.pssm_family_scan(prot["S"], prot["t"], ids2, **kw), ref.rows(hits2, nm, ids2, **kw), "appended")
        s0 = int(np.flatnonzero(np.diff(ids2.astype(np.int64)) > 5)[0])
        gone = np.arange(int(ids2[s0]), int(ids2[s0 + 1]), dtype=np.uint32)
        eng.index_remove(gone)
        ids3 = ids2.copy()
        ids3[s0 + 1:] -= np.uint64(len(gone))
        codes3 = np.delete(codes2, gone, axis=0)
        hits3 = pssm_ref.scan(prot["S"], prot["t"], codes3)
        ref.same_rows(eng.pssm_family_scan(prot["S"], prot["t"], ids3, **kw), ref.rows(hits3, nm, ids3, **kw), "removed")
    finally:
        eng.close()


def _dev_rows(torch, cap, fill=7):
    return [torch.full((cap,), fill, dtype=torch.float64 if t == np.float64 else torch.int32, device="cuda")
            for _, t in capi.PSSM_FAMILY_FIELDS]


def _dev_dict(rows, n, dc, dg, nh):
    got = {name: r[:n].cpu().numpy().astype(t) for (name, t), r in zip(capi.PSSM_FAMILY_FIELDS, rows)}
    got.update(n_hits=nh, cnt=dc.cpu().numpy().astype(np.uint64), grp_rows=dg.cpu().numpy().astype(np.uint64))
    return got


def test_device_pointers_capacity_and_refusals(prot):
    import torch
    eng, nm = prot["eng"], 33
    m_group, m_off = _layout(nm, "mixed", True)
    n_groups = int(m_group.max()) + 1
    t_group = np.full(n_groups, float(np.median(_want(prot, nm, "mixed", True, min_count=2)["sum"])))
    want = _want(prot, nm, "mixed", True, min_count=2, t_group=t_group)
    n_rows = len(want["group"])
    assert 0 < n_rows < _want(prot, nm, "mixed", True, min_count=2)["grp_rows"].sum()
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

    def call(S=dS, t=dt, G=dG, ng=n_groups, O=dO, I=dI, ns=n_seq, mc=2, T=dT, p=ptrs, c=cap):
        torch.cuda.synchronize()
        return eng.pssm_family_scan_dev(S.data_ptr(), t.data_ptr(), nm, G.data_ptr() if G is not None else 0, ng,
                                        O.data_ptr() if O is not None else 0, I.data_ptr() if I is not None else 0, ns,
                                        mc, T.data_ptr() if T is not None else 0, p, c, dc.data_ptr(), dg.data_ptr())

    n, nh = call()
    assert n == n_rows
    ref.same_rows(_dev_dict(rows, n, dc, dg, nh), want, "dev")
    assert all(float(r[n]) == 7 for r in rows)
    p = eng.profile()
    assert p["pssm_fam_kept"] == n_rows and p["pssm_fam_rows"] == _want(prot, nm, "mixed", True)["all_rows"]
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
    kw = dict(m_group=m_group, m_off=m_off, min_count=2, t_group=t_group)
    with pytest.raises(HsError) as e:     # the host form
        eng.pssm_family_scan(prot["S"], prot["t"], prot["id_start"], cap=n_rows - 1, **kw)
    assert e.value.needed == n_rows and e.value.n_hits == want["n_hits"]
    assert np.array_equal(e.value.cnt, want["cnt"]) and np.array_equal(e.value.grp_rows, want["grp_rows"])
    ref.same_rows(eng.pssm_family_scan(prot["S"], prot["t"], prot["id_start"], cap=n_rows, **kw), want, "exact cap")
    # refusals found on the device, before anything is written
    dc.fill_(9), dg.fill_(9)

    def refused(status=capi.HS_ERR_INVALID, **kw):
        with pytest.raises(HsError) as e:
            call(**kw)
        assert e.value.status == status, kw
        assert all(bool((r == 9).all()) for r in rows) and bool((dc == 9).all()) and bool((dg == 9).all())

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
    O2[3] = -(1 << 31)                                                    # the bits of 2^31: above 2^31 - 1
    refused(O=O2)
    refused(p=[0] + ptrs[1:])                                             # a null output with cap > 0
    # the host form: the same refusals, with sentinel-filled outputs untouched
    lib, h = eng._lib, eng._h
    out = [np.full(cap, 9, dtype=t) for _, t in capi.PSSM_FAMILY_FIELDS]
    cnt, grp = np.full(nm, 9, np.uint64), np.full(n_groups, 9, np.uint64)
    n_out, n_hits = C.c_uint64(5), C.c_uint64(5)

    def host(S=prot["S"], t=prot["t"], ids=prot["id_start"], ns=n_seq, nm_=nm, G=m_group, ng=n_groups, O=m_off, mc=2,
             T=t_group, outs=out):
        vp = lambda a: None if a is None else capi._vp(np.ascontiguousarray(a))
        keep = [np.ascontiguousarray(a) if a is not None else None for a in (S, t, G, O, ids, T)]
        st = lib.hs_pssm_family_scan(h, capi._vp(keep[0]), capi._vp(keep[1]), C.c_uint64(nm_), vp(keep[2]), ng,
                                     vp(keep[3]), vp(keep[4]), C.c_uint64(ns), mc, vp(keep[5]),
                                     *[vp(a) for a in outs], cap, C.byref(n_out), C.byref(n_hits), capi._vp(cnt),
                                     capi._vp(grp))
        assert n_out.value == 0 and n_hits.value == 0
        assert all(np.all(a == 9) for a in out) and np.all(cnt == 9) and np.all(grp == 9)
        return st

    S2 = prot["S"].copy()
    S2[1, 2, 3] = np.nan
    ids = prot["id_start"]
    bad = capi.HS_ERR_INVALID
    assert host(S=S2) == bad
    assert host(t=np.where(np.arange(nm) == 4, np.inf, prot["t"])) == bad
    assert host(nm_=1 << 27) == bad
    assert host(ids=None) == bad

    def changed(a, at, value):
        c = a.copy()
        c[at] = value
        return c

    assert host(ids=changed(ids, 30, int(ids[31]) + 1)) == bad           # does not ascend
    assert host(ids=changed(ids, 0, 1)) == bad                           # does not start at 0
    assert host(ids=changed(ids, n_seq, int(ids[-1]) + 1)) == bad        # does not end at n
    assert host(ns=0) == bad
    assert host(G=changed(m_group, 5, m_group[4] + 2)) == bad            # m_group decreases behind it
    assert host(G=changed(m_group, nm - 1, n_groups)) == bad
    assert host(G=None) == bad
    assert host(mc=0) == bad
    assert host(T=changed(t_group, 0, np.nan)) == bad and host(T=changed(t_group, 1, -np.inf)) == bad
    assert host(O=changed(m_off, 3, 1 << 31)) == bad
    assert host(outs=out[:4] + [None] + out[5:]) == bad
    # nm = 0 is an empty, successful call
    empty = eng.pssm_family_scan(np.zeros((0, K, A)), np.zeros(0), prot["id_start"])
    assert len(empty["group"]) == 0 and empty["n_hits"] == 0
    unbuilt = _engine()
    try:
        with pytest.raises(HsError) as e:
            unbuilt.pssm_family_scan(prot["S"], prot["t"], prot["id_start"])
        assert e.value.status == capi.HS_ERR_STATE
    finally:
        unbuilt.close()


def test_a_group_above_the_batch_and_the_width_rule_are_refused():
    """A group of 4097 profiles and a key of 65 bits, through the device-pointer form (whose value checks run on the
    device), the host form and the host rule, on sentinel-filled outputs; 4096 profiles and 64 bits pass."""
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

        def dev(nm_, G=dG, ng=1, O=None, grp=dg):
            torch.cuda.synchronize()
            return eng.pssm_family_scan_dev(dS.data_ptr(), dt.data_ptr(), nm_, G.data_ptr(), ng,
                                            O.data_ptr() if O is not None else 0, dI.data_ptr(), 2, 1, 0, ptrs, 8,
                                            dc.data_ptr(), grp.data_ptr() if grp is not None else 0)

        def dev_untouched():
            return all(bool((r == 9).all()) for r in rows) and bool((dc == 9).all()) and bool((dg == 9).all())

        # (1) the group size, found by the device's check: m_group[m] == m_group[m - 4096]
        with pytest.raises(HsError) as e:
            dev(4097)
        assert e.value.status == capi.HS_ERR_INVALID and "4096" in str(e.value) and dev_untouched()
        G2 = dG.clone()
        G2[4096] = 1                                            # 4096 profiles and one: two groups, both allowed
        dg2 = torch.full((2,), 9, dtype=torch.int64, device="cuda")
        assert dev(4097, G=G2, ng=2, grp=dg2) == (0, 0) and bool((dg2 == 0).all()) and bool((dc == 0).all())
        dc.fill_(9)
        assert dev(4096) == (0, 0) and bool((dc[:4096] == 0).all()) and int(dc[4096]) == 9 and int(dg[0]) == 0
        dc.fill_(9), dg.fill_(9)
        with pytest.raises(HsError) as e:                       # the host form, through the wrapper ...
            eng.pssm_family_scan(S, t, ids, m_group=zeros)
        assert e.value.status == capi.HS_ERR_INVALID and "4096" in str(e.value)
        got = eng.pssm_family_scan(S[:4096], t[:4096], ids, m_group=zeros[:4096])
        assert len(got["group"]) == 0 and got["n_hits"] == 0
        # (2) the width rule: 2^32 groups (32 bits), 2 sequences (1 bit), 40 ids + an offset of 2^31 - 1 (32 bits)
        big = 1 << 32
        off = np.zeros(4, np.uint32)
        off[2] = (1 << 31) - 1
        dO = torch.from_numpy(off.astype(np.int32)).cuda()
        with pytest.raises(HsError) as e:
            dev(4, ng=big, O=dO, grp=None)
        assert e.value.status == capi.HS_ERR_INVALID and "64-bit key" in str(e.value) and dev_untouched()
        dO[2] = 1 << 30                                         # 31 bits for the diagonal: 64 in all, accepted
        assert dev(4, ng=big, O=dO, grp=None) == (0, 0)
        dc.fill_(9)
        # ... the host form and the host rule, called directly: sentinel-filled outputs stay
        out = [np.full(8, 9, dtype=ty) for _, ty in capi.PSSM_FAMILY_FIELDS]
        cnt = np.full(4, 9, np.uint64)
        n_out, n_hits = C.c_uint64(5), C.c_uint64(5)
        vp = capi._vp

        def host(nm_, G, ng, O, grp):
            st = eng._lib.hs_pssm_family_scan(eng._h, vp(S), vp(t), nm_, vp(G), ng, None if O is None else vp(O), vp(ids),
                                              2, 1, None, *[vp(a) for a in out], 8, C.byref(n_out), C.byref(n_hits),
                                              vp(cnt), None if grp is None else vp(grp))
            return st

        def host_untouched():
            return all(np.all(a == 9) for a in out) and np.all(cnt == 9) and n_out.value == 0 and n_hits.value == 0

        assert host(4, zeros, big, off, None) == capi.HS_ERR_INVALID and host_untouched()
        assert b"64-bit key" in eng._lib.hs_last_error(eng._h)
        grp1 = np.full(1, 9, np.uint64)
        cnt = np.full(nm, 9, np.uint64)
        assert host(4097, zeros, 1, None, grp1) == capi.HS_ERR_INVALID and host_untouched() and grp1[0] == 9
        off_ok = off.copy()
        off_ok[2] = 1 << 30
        cnt = np.full(4, 9, np.uint64)
        assert host(4, zeros, big, off_ok, None) == capi.HS_OK and np.all(cnt == 0)
        m, i, sc = np.array([0, 1], np.uint32), np.array([3, 50], np.uint32), np.array([1.0, 2.0])

        def rule(O):
            st = eng._lib.hs_pssm_family_hits(vp(m), vp(i), vp(sc), 2, 4, vp(zeros), big, vp(O), vp(ids), 2, 1, None,
                                              *[vp(a) for a in out], 8, C.byref(n_out))
            return st

        n_out.value = 5
        assert rule(off) == capi.HS_ERR_INVALID and all(np.all(a == 9) for a in out) and n_out.value == 0
        with pytest.raises(HsError):
            capi.pssm_family_hits(m, i, sc, 4, ids, m_group=zeros[:4], n_groups=big, m_off=off)
        assert rule(off_ok) == capi.HS_OK and n_out.value == 2 and out[1][:2].tolist() == [0, 1]
    finally:
        eng.close()


def test_other_calls_around_it():
    """hs_pssm_scan, hs_pssm_seq_scan, hs_pssm_topk and hs_seq_match on the same handle give what they gave."""
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
            return (eng.pssm_scan(S, t), eng.pssm_seq_scan(S, t, ids), eng.pssm_topk(S, 5),
                    eng.seq_match(Q["qcodes"], ids, R=seqmatch_ref.R, codes=True, q_group=Q["q_group"],
                                  n_groups=len(P["qry_start"]) - 1, q_off=Q["q_off"]))

        before = others()
        ref.same_rows(_scan(eng, case, 17, "mixed", True), _want(case, 17, "mixed", True), "between")
        after = others()
        for x, y in zip(before, after):
            assert x.keys() == y.keys()
            for f in x:
                assert np.array_equal(x[f], y[f]), f
        assert len(before[0]["m"]) > 0 and len(before[3]["count"]) > 0
    finally:
        eng.close()


def test_planted_motif_end_to_end():
    """compare -> layout -> family scan over the planted motif of tests/pssm_family_ref.py (seed 20261; the construction
    is checked on the reference by tests/test_pssm_family_cpu.py): with min_count = 3 the reported proteins are exactly
    the planted ones, on the diagonal of the planted position; every profile alone also hits decoys."""
    c = ref.planted_case()
    eng = _engine()
    try:
        info, _ = eng.index_build_windows(c["residues"], c["seq_start"])
        assert info["n"] == len(c["codes"])
        h = eng.pssm_compare(capi.pssm_compare_columns(c["S"], "pearson"), 10.0, None, 13)
        lay = capi.pssm_family_layout(h["x"], h["y"], h["d"], 3)
        assert lay["n_groups"] == 1 and lay["n_conflicts"] == 0 and lay["off"].tolist() == c["shifts"].tolist()
        order = lay["order"]
        got = eng.pssm_family_scan(c["S"][order], c["t"][order], c["id_start"], m_group=lay["group"][order],
                                   m_off=lay["off"][order], min_count=3)
        assert dict(zip(got["seq"].tolist(), got["diag"].tolist())) == c["planted"] and len(got["seq"]) == 9
        assert np.all(got["count"] == 3) and np.all(got["hi"] - got["lo"] == 6)
        hits = pssm_ref.scan(c["S"], c["t"], c["codes"])
        ref.same_rows(got, ref.rows(hits, 3, c["id_start"], m_group=lay["group"], m_off=lay["off"], min_count=3), "rows")
        alone = eng.pssm_family_scan(c["S"], c["t"], c["id_start"])
        for m in range(3):
            assert len(set(alone["seq"][alone["group"] == m].tolist()) - set(c["planted"])) >= 5
    finally:
        eng.close()
