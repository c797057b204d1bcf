"""The profile calls on the random worlds of tests/pssm_fuzz_cases.py against the Python references of tests/*_ref.py:
per world one engine and one index, every call, every array bit for bit, and the counters of the profile where the
reference predicts them.  The seed's residues decide how the world runs -- the filter off, the profile batch, the grid
of the null model, the test build that splits batches above 4 profiles, the way the index came about (built from
windows or codes, grown, shrunk, loaded), the device-pointer forms -- so a failure's name reproduces it.
tests/test_pssm_fuzz_cpu.py holds the same worlds to the edges they must reach."""
import os

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import (pssm_chain_ref, pssm_compare_ref, pssm_counts_ref, pssm_family_ref, pssm_fuzz_cases as cases,
                   pssm_null_ref, pssm_rank_ref, pssm_seq_ref, pssm_topk_ref, pssm_weights_ref)

pytestmark = pytest.mark.gpu

EVERYTHING = -1e300       # a threshold every k-mer reaches
# what the device-pointer forms' outputs are filled with: no call writes either -- ids, counts and profile numbers stay
# below 2^31, a diagonal or a shift is a difference of offsets of at most a few million, and no score is a NaN
SENTINEL = -(1 << 31) + 9


def _engine(w, hooks=False):
    a, b = synth.make_planes(w["k"], 2, 1, 200.0, seed=3)
    return Engine(w["k"], 2, 1, 200.0, a, b, coords=w["coords"], hooks=hooks,
                  options=dict(pssm_filter=w["pssm_filter"], query_batch=w["query_batch"], pssm_null_bins=w["bins"]))


def _build(eng, w, tmp_path):
    """the world's index by the world's route; every route ends at the same n k-mers in the same order"""
    route, n, k = w["route"], w["n"], w["k"]
    if route == "windows":
        info, _ = eng.index_build_windows(w["residues"], w["seq_start"])
    elif route == "codes":
        info = eng.index_build(w["codes"])
    elif route == "append":
        eng.index_build(w["codes"][:n // 2])
        info = eng.index_append(w["codes"][n // 2:])
    elif route == "remove":          # a leading sequence of three windows more, taken away again
        extra = np.random.default_rng(w["seed"]).integers(0, w["A"], size=k + 2).astype(np.uint8)
        eng.index_build_windows(np.concatenate([extra, w["residues"]]),
                                np.concatenate([[0], w["seq_start"] + np.uint64(k + 2)]).astype(np.uint64))
        new_id = eng.index_remove(np.arange(3, dtype=np.uint32))
        assert new_id[:3].tolist() == [capi.NO_ID] * 3 and np.array_equal(new_id[3:], np.arange(n, dtype=np.uint32))
        info = eng.index_info()
    else:
        other = _engine(w)
        try:
            other.index_build_windows(w["residues"], w["seq_start"])
            other.index_save(tmp_path / "world.idx")
        finally:
            other.close()
        info = eng.index_load(tmp_path / "world.idx")
    assert info["n"] == n


def _same_compare(got, want, what):
    for f in ("x", "y", "d", "cnt"):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f)
    assert pssm_compare_ref.same_bits(got["score"], want["score"]), what


def _host_forms(eng, w, want, what):
    nm, ids, S, t, n = w["nm"], w["id_start"], w["S"], w["t"], w["n"]
    hits = eng.pssm_scan(S, t)
    for f in ("m", "id", "cnt"):
        assert np.array_equal(hits[f], w["hits"][f]), (what, f)
    assert pssm_compare_ref.same_bits(hits["score"], w["hits"]["score"]), what
    p = eng.profile()
    assert p["hits"] == len(w["hits"]["m"]), what
    if not w["pssm_filter"]:
        assert p["pssm_survivors"] == nm * n, what

    seq = eng.pssm_seq_scan(S, t, ids)
    pssm_seq_ref.same_rows(seq, want["seq"], what)
    p = eng.profile()
    assert p["pssm_seq_rows"] == len(want["seq"]["m"]) and p["hits"] == want["seq"]["n_hits"], what

    fam = eng.pssm_family_scan(S, t, ids, **cases.family_args(w))
    pssm_family_ref.same_rows(fam, want["fam"], what)
    p = eng.profile()
    assert p["pssm_fam_rows"] == want["fam"]["all_rows"] and p["pssm_fam_kept"] == len(want["fam"]["group"]), what
    assert p["hits"] == want["fam"]["n_hits"], what
    plain = eng.pssm_family_scan(S, t, ids)
    pssm_family_ref.same_rows(plain, want["fam_plain"], what)
    # (1) without m_group and m_off the family scan is the sequence scan's rows -- the device's against the device's
    for mine, theirs in (("group", "m"), ("seq", "seq"), ("count", "count"), ("best_id", "best_id"), ("lo", "lo"),
                         ("hi", "hi"), ("best_m", "m"), ("cnt", "cnt"), ("grp_rows", "seq_cnt")):
        assert np.array_equal(plain[mine], seq[theirs]), (what, mine)
    assert pssm_compare_ref.same_bits(plain["best_score"], seq["best_score"]) and np.all(plain["diag"] == 0), what
    assert plain["n_hits"] == seq["n_hits"], what

    args, kw = cases.chain_args(w)
    chain = eng.pssm_family_chain(S, t, ids, *args, **kw)
    pssm_chain_ref.same_chains(chain, want["chain"], what)
    p = eng.profile()
    assert p["pssm_chain_segs"] == want["chain"]["all_segs"] and p["pssm_chain_kept"] == len(want["chain"]["group"]), what
    assert p["hits"] == want["chain"]["n_hits"], what

    top = eng.pssm_topk(S, w["topk"])
    pssm_topk_ref.same_rows(top, want["topk"], what)
    # (2) pssm_topk(N) is the N best of an everything-hits scan under (score descending, id ascending)
    every = eng.pssm_scan(S, np.full(nm, EVERYTHING))
    assert len(every["m"]) == nm * n, what
    sc = every["score"].reshape(nm, n)
    assert np.array_equal(every["id"].reshape(nm, n), np.broadcast_to(np.arange(n, dtype=np.uint32), (nm, n))), what
    take = min(w["topk"], n)
    for m in range(nm):
        best = np.lexsort((np.arange(n), -sc[m]))[:take]
        assert np.array_equal(top["id"][m, :take], best.astype(np.uint32)), (what, m)
        assert pssm_compare_ref.same_bits(top["score"][m, :take], sc[m, best]), (what, m)

    rank = eng.pssm_rank(S, w["rank"])
    pssm_rank_ref.same(rank, want["rank"], what)
    # (3) a scan at the thresholds pssm_rank returns gives counts that bracket the ranks
    at = eng.pssm_scan(S, rank["t"])
    assert np.array_equal(at["cnt"], rank["cnt_ge"]), what
    above = np.bincount(at["m"][at["score"] > rank["t"][at["m"]]].astype(np.int64), minlength=nm).astype(np.uint64)
    assert np.array_equal(above, rank["cnt_gt"]) and np.all(above < w["rank"]) and np.all(w["rank"] <= at["cnt"]), what

    for name, start in (("counts", None), ("counts_seq", ids)):
        got = eng.pssm_hit_counts(S, t, start)
        pssm_counts_ref.same_counts(got, want[name], (what, name))
        p = eng.profile()
        assert p["pssm_count_sites"] == int(want[name]["used"].sum()) and p["hits"] == want[name]["n_hits"], (what, name)
    for name, start in (("weights", None), ("weights_seq", ids)):
        got = eng.pssm_weighted_counts(S, t, start)
        pssm_weights_ref.same_weights(got, want[name], (what, name))
        p = eng.profile()
        assert p["pssm_weight_sites"] == int(want[name]["used"].sum()) and p["hits"] == want[name]["n_hits"], (what, name)

    pv = eng.pssm_pvalue(S, want["pv_m"], want["pv_score"], bg=w["bg"], t_lo=w["t_lo"])
    assert pssm_null_ref.same_bits(pv["p_hi"], want["p_hi"]) and pssm_null_ref.same_bits(pv["p_lo"], want["p_lo"]), what
    p = eng.profile()
    assert p["pssm_null_bins"] == w["bins"] and p["pssm_null_profiles"] == nm, what
    th = eng.pssm_pvalue_threshold(S, w["p"], bg=w["bg"], t_lo=w["t_lo"])
    for f in ("t", "p_hi", "p_lo"):
        assert pssm_null_ref.same_bits(th[f], want["thr"][f]), (what, f)
    assert np.array_equal(th["flag"], want["thr"]["flag"]), what

    X, Y = cases.compare_args(w)
    _same_compare(eng.pssm_compare(S, w["cmp_t"], None, w["min_overlap"]), want["cmp_self"], (what, "self"))
    p = eng.profile()
    assert p["pssm_cmp_pairs"] == nm * (nm - 1) // 2 and p["hits"] == len(want["cmp_self"]["x"]), what
    if want["reached"]["compare_unfiltered"]:
        assert p["pssm_cmp_steps"] == 0 and p["pssm_cmp_survivors"] == p["pssm_cmp_pairs"], what
    _same_compare(eng.pssm_compare(X, w["cmp_t"], Y, w["min_overlap"]), want["cmp_xy"], (what, "xy"))
    p = eng.profile()
    assert p["pssm_cmp_pairs"] == len(X) * len(Y) and p["hits"] == len(want["cmp_xy"]["x"]), what


def _fill(r):
    return r.fill_(float("nan") if r.is_floating_point() else SENTINEL)


def _rows(torch, fields, cap):
    return [_fill(torch.empty((max(cap, 1),), dtype=torch.float64 if t == np.float64 else torch.int32, device="cuda"))
            for _, t in fields]


def _read(fields, rows, n):
    return {name: r[:n].cpu().numpy().astype(t) for (name, t), r in zip(fields, rows)}


def _sentinel(r):
    """bool tensor: the entries of r that still hold what _fill wrote"""
    return r.isnan() if r.is_floating_point() else r == SENTINEL


def _untouched(rows):
    return all(bool(_sentinel(r).all()) for r in rows)


def _u64(x):
    return x.cpu().numpy().astype(np.uint64)


def _device_forms(eng, w, want, what):
    """The device-pointer forms on sentinel-filled outputs of exactly the needed size; then one row short: the
    capacity status, the needed count and the counts.  The contract (include/hsearch.h) lets a _dev form write the rows
    of the profile batches that still fitted, so under the world's batch size every entry is either the sentinel or the
    row that belongs there, and the last one is the sentinel; then again as ONE batch (query_batch = 0, where the test
    build does not split it): no row written."""
    import torch
    nm, n_seq, ng = w["nm"], w["n_seq"], w["n_groups"]
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).astype(t)).cuda()
    dS, dt, dI = dev(w["S"], np.float64), dev(w["t"], np.float64), dev(w["id_start"], np.int64)
    dG, dO, dC = dev(w["m_group"], np.int32), dev(w["m_off"], np.int32), dev(w["chain_off"], np.int32)
    dT = dev(w["t_group"], np.float64) if w["t_group"] is not None else None
    tg = dT.data_ptr() if dT is not None else 0
    dc = torch.full((nm,), 9, dtype=torch.int64, device="cuda")
    dg = torch.full((ng,), 9, dtype=torch.int64, device="cuda")
    ds = torch.full((nm,), 9, dtype=torch.int64, device="cuda")

    def short(call, fields, rows, ref, needed, n_hits=None):
        if needed == 0:
            return
        try:
            for one_batch in (False, True):
                if one_batch:
                    if w["hooks"] and nm > cases.SPLIT_ABOVE:
                        break
                    eng.set_option("query_batch", 0)
                for r in rows:
                    _fill(r)
                torch.cuda.synchronize()
                with pytest.raises(HsError) as e:
                    call(needed - 1)
                assert e.value.status == capi.HS_ERR_CAPACITY, what
                assert (e.value.needed if hasattr(e.value, "needed") else e.value.n_hits) == needed, what
                assert n_hits is None or e.value.n_hits == n_hits, what
                torch.cuda.synchronize()
                if one_batch:
                    assert _untouched(rows), what
                    continue
                for (name, ty), r in zip(fields, rows):
                    raw = r[:needed].cpu().numpy()
                    written = ~_sentinel(r[:needed]).cpu().numpy()
                    assert not written[needed - 1], (what, name)
                    a, b = raw.astype(ty)[written], np.asarray(ref[name])[written]
                    if ty == np.float64:
                        a, b = a.view(np.uint64), b.view(np.uint64)
                    assert np.array_equal(a, b), (what, name)
        finally:
            eng.set_option("query_batch", w["query_batch"])

    # the scan, and the p-values of its hits without a copy to the host
    h = w["hits"]
    scan_fields = (("m", np.uint32), ("id", np.uint32), ("score", np.float64))
    rows = _rows(torch, scan_fields, len(h["m"]))
    call = lambda cap: eng.pssm_scan_dev(dS.data_ptr(), dt.data_ptr(), nm, *[r.data_ptr() for r in rows], cap,
                                         dc.data_ptr())
    torch.cuda.synchronize()
    assert call(len(h["m"])) == len(h["m"]), what
    got = _read(scan_fields, rows, len(h["m"]))
    assert np.array_equal(got["m"], h["m"]) and np.array_equal(got["id"], h["id"]), what
    assert pssm_compare_ref.same_bits(got["score"], h["score"]) and np.array_equal(_u64(dc), h["cnt"]), what
    if len(h["m"]):
        dbg = dev(w["bg"], np.float64)
        dtl = dev(np.full(nm, w["t_lo"]), np.float64) if w["t_lo"] is not None else None
        dhi, dlo = (torch.full((len(h["m"]) + 1,), 9.0, dtype=torch.float64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        eng.pssm_pvalue_dev(dS.data_ptr(), nm, rows[0].data_ptr(), rows[2].data_ptr(), len(h["m"]), dhi.data_ptr(),
                            dlo.data_ptr(), d_bg=dbg.data_ptr(), d_t_lo=dtl.data_ptr() if dtl is not None else None)
        k = len(h["m"])
        assert pssm_null_ref.same_bits(dhi[:k].cpu().numpy(), want["p_hi"][:k]), what
        assert pssm_null_ref.same_bits(dlo[:k].cpu().numpy(), want["p_lo"][:k]), what
        assert float(dhi[k]) == 9.0 and float(dlo[k]) == 9.0, what
    dc.fill_(9)
    short(call, scan_fields, rows, h, len(h["m"]))
    assert np.array_equal(_u64(dc), h["cnt"]) or len(h["m"]) == 0, what

    # the sequence scan
    need = len(want["seq"]["m"])
    rows = _rows(torch, capi.PSSM_SEQ_FIELDS, need)
    call = lambda cap: eng.pssm_seq_scan_dev(dS.data_ptr(), dt.data_ptr(), nm, dI.data_ptr(), n_seq,
                                             [r.data_ptr() for r in rows], cap, dc.data_ptr(), ds.data_ptr())
    torch.cuda.synchronize()
    assert call(need) == (need, want["seq"]["n_hits"]), what
    got = _read(capi.PSSM_SEQ_FIELDS, rows, need)
    got.update(cnt=_u64(dc), seq_cnt=_u64(ds))
    pssm_seq_ref.same_rows(got, want["seq"], (what, "dev"))
    short(call, capi.PSSM_SEQ_FIELDS, rows, want["seq"], need, want["seq"]["n_hits"])

    # the family scan
    need = len(want["fam"]["group"])
    rows = _rows(torch, capi.PSSM_FAMILY_FIELDS, need)
    call = lambda cap: eng.pssm_family_scan_dev(dS.data_ptr(), dt.data_ptr(), nm, dG.data_ptr(), ng, dO.data_ptr(),
                                                dI.data_ptr(), n_seq, w["min_count"], tg, [r.data_ptr() for r in rows],
                                                cap, dc.data_ptr(), dg.data_ptr())
    torch.cuda.synchronize()
    assert call(need) == (need, want["fam"]["n_hits"]), what
    got = _read(capi.PSSM_FAMILY_FIELDS, rows, need)
    got.update(cnt=_u64(dc), grp_rows=_u64(dg))
    pssm_family_ref.same_rows(got, want["fam"], (what, "dev"))
    dg.fill_(9)
    short(call, capi.PSSM_FAMILY_FIELDS, rows, want["fam"], need, want["fam"]["n_hits"])
    assert need == 0 or np.array_equal(_u64(dg), want["fam"]["grp_rows"]), what

    # the chain
    need = len(want["chain"]["group"])
    rows = _rows(torch, capi.PSSM_CHAIN_FIELDS, need)
    call = lambda cap: eng.pssm_family_chain_dev(dS.data_ptr(), dt.data_ptr(), nm, dG.data_ptr(), ng, dC.data_ptr(),
                                                 dI.data_ptr(), n_seq, w["max_shift"], w["gap_open"], w["gap_ext"],
                                                 w["min_count"], tg, [r.data_ptr() for r in rows], cap, dc.data_ptr(),
                                                 dg.data_ptr())
    torch.cuda.synchronize()
    assert call(need) == (need, want["chain"]["n_hits"]), what
    got = _read(capi.PSSM_CHAIN_FIELDS, rows, need)
    got.update(cnt=_u64(dc), grp_rows=_u64(dg))
    pssm_chain_ref.same_chains(got, want["chain"], (what, "dev"))
    short(call, capi.PSSM_CHAIN_FIELDS, rows, want["chain"], need, want["chain"]["n_hits"])

    # the comparison, X against itself
    cmp_fields = (("x", np.uint32), ("y", np.uint32), ("d", np.int32), ("score", np.float64))
    need = len(want["cmp_self"]["x"])
    rows = _rows(torch, cmp_fields, need)
    dct = dev(np.full(nm, w["cmp_t"]), np.float64)
    call = lambda cap: eng.pssm_compare_dev(dS.data_ptr(), nm, 0, 0, dct.data_ptr(), w["min_overlap"],
                                            *[r.data_ptr() for r in rows], cap, dc.data_ptr())
    torch.cuda.synchronize()
    assert call(need) == need, what
    got = _read(cmp_fields, rows, need)
    got["cnt"] = _u64(dc)
    _same_compare(got, want["cmp_self"], (what, "dev"))
    short(call, cmp_fields, rows, want["cmp_self"], need)


@pytest.mark.parametrize("seed", range(int(os.environ.get("HS_PSSM_FUZZ_CASES", str(cases.DEFAULT_CASES)))))
def test_random_world_matches_the_references(seed, monkeypatch, tmp_path):
    w = cases.world(seed)
    want = cases.references(w)
    what = (seed, w["style"], w["k"], w["A"], w["nm"], w["n"], w["route"])
    if w["hooks"]:          # the test build reports a survivor-counter overflow for every batch of more than 4 profiles
        monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", str(cases.SPLIT_ABOVE))
    eng = _engine(w, hooks=w["hooks"])
    try:
        _build(eng, w, tmp_path)
        _host_forms(eng, w, want, what)
        if w["dev"]:
            _device_forms(eng, w, want, what)
    finally:
        eng.close()
