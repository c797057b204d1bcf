"""hs_seq_match_hits / hs_seq_match_merge / hs_window_id_start (host only, no GPU): the rule of include/hsearch.h
against tests/seqmatch_ref.py on random tuple lists -- empty sequences at the start, in the middle and at the end, ids
on both ends of a sequence, diagonals of both signs, with and without q_group and q_off --, invariance under a
permutation, duplicates, -0.0, the merge of query blocks against the whole, and every error of the contract with the
outputs left unwritten."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hsearch_amd
from hsearch_amd import capi
from tests import seqmatch_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NEW = ["hs_seq_match", "hs_seq_match_dev", "hs_window_id_start", "hs_seq_match_hits", "hs_seq_match_merge"]
# sequences without ids at the start, twice in the middle and at the end
_LENS = (0, 0, 5, 1, 0, 0, 40, 17, 0, 300, 2, 0)


def _id_start(lens=_LENS):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _case(seed, nq=23, m=900, n_groups=5, lens=_LENS):
    """m distinct (q, id) with heavily tied distances; every sequence's first and last id is hit"""
    rng = np.random.default_rng(seed)
    id_start = _id_start(lens)
    n = int(id_start[-1])
    pairs = rng.choice(nq * n, size=m, replace=False)
    ends = np.unique(np.concatenate([id_start[:-1][np.diff(id_start) > 0], id_start[1:][np.diff(id_start) > 0] - 1]))
    pairs = np.unique(np.concatenate([pairs, rng.integers(0, nq, len(ends)) * n + ends.astype(np.int64)]))
    rng.shuffle(pairs)
    q, id = (pairs // n).astype(np.uint32), (pairs % n).astype(np.uint32)
    dist = rng.choice(np.array([0.0, 1.0, 1.5, 7.25]), len(q))
    q_group = rng.integers(0, n_groups, nq).astype(np.uint32)
    q_off = rng.integers(0, 120, nq).astype(np.uint32)
    return dict(q=q, id=id, dist=dist), nq, id_start, q_group, n_groups, q_off


def test_library_exports_the_seq_match_symbols():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    declared = re.findall(r"HS_API\s+[\w\s\*]+?\b(hs_\w+)\s*\(", header)
    lib = hsearch_amd.load()
    for name in _NEW:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("use_group,use_off", [(True, True), (False, True), (True, False), (False, False)])
def test_hits_match_the_reference(seed, use_group, use_off):
    hits, nq, id_start, q_group, n_groups, q_off = _case(seed)
    g, o = q_group if use_group else None, q_off if use_off else None
    want = sr.seq_match(hits, id_start, g, o)
    got = capi.seq_match_hits(hits["q"], hits["id"], hits["dist"], nq, id_start, q_group=g,
                              n_groups=n_groups if use_group else None, q_off=o)
    sr.assert_same(got, want, (seed, use_group, use_off))
    assert int(got["count"].sum()) == len(hits["q"])
    assert (got["lo"] <= got["hi"]).all()
    if use_off:
        assert (want["diag"] < 0).any() and (want["diag"] > 0).any()
    else:
        assert (want["diag"] == 0).all()
    # both ends of a sequence are hit, and no row names a sequence without ids
    lens = np.diff(id_start.astype(np.int64))
    assert (lens[got["seq"]] > 0).all()
    assert (got["lo"] == 0).any() and (got["hi"] == lens[got["seq"]] - 1).any()
    # rows strictly ascending in (group, seq, diag)
    key = np.stack([got["group"].astype(np.int64), got["seq"].astype(np.int64), got["diag"].astype(np.int64)], 1)
    assert all(tuple(key[i]) < tuple(key[i + 1]) for i in range(len(key) - 1))


def test_permutation_duplicates_and_negative_zero():
    hits, nq, id_start, q_group, n_groups, q_off = _case(7)
    args = dict(q_group=q_group, n_groups=n_groups, q_off=q_off)
    want = capi.seq_match_hits(hits["q"], hits["id"], hits["dist"], nq, id_start, **args)
    rng = np.random.default_rng(5)
    for _ in range(3):
        p = rng.permutation(len(hits["q"]))
        sr.assert_same(capi.seq_match_hits(hits["q"][p], hits["id"][p], hits["dist"][p], nq, id_start, **args), want,
                       "permuted")
    # every third tuple once more: counts once
    dup = np.concatenate([np.arange(len(hits["q"])), np.arange(0, len(hits["q"]), 3)])
    rng.shuffle(dup)
    sr.assert_same(capi.seq_match_hits(hits["q"][dup], hits["id"][dup], hits["dist"][dup], nq, id_start, **args), want,
                   "duplicates")
    # ... but not with two distances
    q2, id2 = np.append(hits["q"], hits["q"][0]), np.append(hits["id"], hits["id"][0])
    with pytest.raises(capi.HsError) as e:
        capi.seq_match_hits(q2, id2, np.append(hits["dist"], hits["dist"][0] + 1.0), nq, id_start, **args)
    assert e.value.status == capi.HS_ERR_INVALID
    # -0.0 is +0.0: the same bits out, and it ties with +0.0 on (q, id)
    neg = hits["dist"].copy()
    neg[neg == 0.0] = -0.0
    assert np.signbit(neg).any()
    got = capi.seq_match_hits(hits["q"], hits["id"], neg, nq, id_start, **args)
    sr.assert_same(got, want, "-0.0")
    assert not np.signbit(got["best_dist"]).any()


@pytest.mark.parametrize("blocks", [1, 2, 3, 4, 5])
def test_merge_of_query_blocks_is_the_whole(blocks):
    hits, nq, id_start, q_group, n_groups, q_off = _case(11, nq=41, m=2500)
    args = dict(q_group=q_group, n_groups=n_groups, q_off=q_off)
    whole = capi.seq_match_hits(hits["q"], hits["id"], hits["dist"], nq, id_start, **args)
    cuts = np.linspace(0, nq, blocks + 1).astype(int)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        m = (hits["q"] >= lo) & (hits["q"] < hi)
        parts.append(capi.seq_match_hits(hits["q"][m], hits["id"][m], hits["dist"][m], nq, id_start, **args))
    sr.assert_same(capi.seq_match_merge(parts), whole, blocks)
    sr.assert_same(capi.seq_match_merge(parts[::-1]), whole, (blocks, "reversed"))
    # the capacity protocol of both host forms
    need = len(whole["group"])
    for call in (lambda cap: capi.seq_match_merge(parts, cap=cap),
                 lambda cap: capi.seq_match_hits(hits["q"], hits["id"], hits["dist"], nq, id_start, cap=cap, **args)):
        with pytest.raises(capi.HsError) as e:
            call(need - 1)
        assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == need
        sr.assert_same(call(need), whole, "cap = need")


def test_merge_refuses_a_count_past_32_bits():
    row = dict(group=[1], seq=[2], diag=[-3], count=[0x80000000], best_dist=[1.0], best_q=[4], best_id=[5], lo=[6],
               hi=[7])
    with pytest.raises(capi.HsError) as e:
        capi.seq_match_merge([row, row])
    assert e.value.status == capi.HS_ERR_INVALID
    small = dict(row, count=[0x7fffffff])
    got = capi.seq_match_merge([row, small])
    assert got["count"].tolist() == [0xffffffff] and got["diag"].tolist() == [-3]


def test_window_id_start_against_a_direct_count():
    rng = np.random.default_rng(3)
    for k in (1, 4, 15, 25):
        lens = np.concatenate([[0, k - 1, k, k + 1], rng.integers(0, 3 * k + 2, 40), [0]])
        seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        want = [0]
        for n in lens:
            want.append(want[-1] + sum(1 for _ in range(0, int(n) - k + 1)))
        got = capi.window_id_start(seq_start, k)
        assert got.dtype == np.uint64 and got.tolist() == want
    with pytest.raises(capi.HsError) as e:
        capi.window_id_start([0, 5, 4], 3)
    assert e.value.status == capi.HS_ERR_INVALID
    with pytest.raises(capi.HsError):
        capi.window_id_start([0, 5], 0)


def test_protein_queries_cut_windows_like_the_database():
    rng = np.random.default_rng(9)
    k = 6
    lens = [0, 5, 6, 7, 30, 2]
    res = rng.integers(0, 20, sum(lens)).astype(np.uint8)
    seq_start = np.concatenate([[0], np.cumsum(lens)])
    got = capi.protein_queries(res, seq_start, k)
    rows, grp, off = [], [], []
    for p, (a, b) in enumerate(zip(seq_start[:-1], seq_start[1:])):
        for o in range(0, b - a - k + 1):
            rows.append(res[a + o:a + o + k])
            grp.append(p)
            off.append(o)
    assert np.array_equal(got["qcodes"], np.array(rows)) and got["qcodes"].dtype == np.uint8
    assert got["q_group"].tolist() == grp and got["q_off"].tolist() == off


def _raw_hits(hits, nq, q_group, n_groups, q_off, id_start, cap=64):
    """the C call itself with filled outputs: (status, n_out, outputs untouched)"""
    q = np.ascontiguousarray(hits["q"], dtype=np.uint32)
    id = np.ascontiguousarray(hits["id"], dtype=np.uint32)
    dist = np.ascontiguousarray(hits["dist"], dtype=np.float64)
    outs = [np.full(cap, 0x5A, dtype=t) for _, t in capi.SEQ_MATCH_FIELDS]
    keep = [np.ascontiguousarray(x) for x in (q_group, q_off, id_start) if x is not None]
    n_out = C.c_uint64(99)
    st = hsearch_amd.load().hs_seq_match_hits(
        capi._vp(q), capi._vp(id), capi._vp(dist), len(q), nq, None if q_group is None else capi._vp(q_group), n_groups,
        None if q_off is None else capi._vp(q_off), capi._vp(id_start), len(id_start) - 1, *[capi._vp(o) for o in outs],
        cap, C.byref(n_out))
    del keep
    return st, n_out.value, all((o == 0x5A).all() for o in outs)


def test_every_error_of_the_contract_leaves_the_outputs_untouched():
    u32, u64 = np.uint32, np.uint64
    hits = dict(q=np.array([0, 1], dtype=u32), id=np.array([0, 9], dtype=u32), dist=np.array([1.0, 2.0]))
    good = np.array([0, 4, 4, 10], dtype=u64)
    grp, off = np.array([0, 2], dtype=u32), np.array([3, 0], dtype=u32)
    assert _raw_hits(hits, 2, grp, 3, off, good) == (capi.HS_OK, 2, False)
    bad = [
        ("id_start descends", dict(id_start=np.array([0, 5, 4, 10], dtype=u64))),
        ("id_start does not start at 0", dict(id_start=np.array([1, 4, 4, 10], dtype=u64))),
        ("an id at id_start's end", dict(id_start=np.array([0, 4, 4, 9], dtype=u64))),
        ("a group out of range", dict(q_group=np.array([0, 3], dtype=u32))),
        ("no q_group, n_groups != nq", dict(q_group=None, n_groups=3)),
        ("q >= nq", dict(nq=1, q_group=None, n_groups=1, q_off=None)),
        ("a NaN distance", dict(dist=np.array([1.0, np.nan]))),
        ("a negative distance", dict(dist=np.array([-1.0, 2.0]))),
    ]
    for what, change in bad:
        a = dict(nq=2, q_group=grp, n_groups=3, q_off=off, id_start=good, dist=hits["dist"])
        a.update(change)
        st, n_out, untouched = _raw_hits(dict(hits, dist=a["dist"]), a["nq"], a["q_group"], a["n_groups"], a["q_off"],
                                         a["id_start"])
        assert (st, n_out, untouched) == (capi.HS_ERR_INVALID, 0, True), what
    # the width rule: 32 bits of groups + 0 of sequences + 32 / 33 of diagonals; then 1 of sequences on top of 64
    one_seq = np.array([0, 10], dtype=u64)
    wide = 1 << 32
    for max_qoff, id_start, status in ((wide - 10, one_seq, capi.HS_OK),          # 10 + 2^32 - 10 - 1 = 2^32 - 1: 32 bits
                                       (wide - 9, one_seq, capi.HS_ERR_INVALID),  # 2^32: 33 bits, 65 in all
                                       (wide - 10, np.array([0, 10, 10], dtype=u64), capi.HS_ERR_INVALID)):
        st, n_out, untouched = _raw_hits(hits, 2, grp, wide, np.array([max_qoff, 0], dtype=u32), id_start)
        assert st == status and untouched == (status != capi.HS_OK), (max_qoff, len(id_start))
    st, _, untouched = _raw_hits(hits, 2, grp, wide + 1, off, one_seq)
    assert st == capi.HS_ERR_INVALID and untouched
    # at exactly 64 bits the rows are right
    off64 = np.array([wide - 10, 0], dtype=u32)
    got = capi.seq_match_hits(hits["q"], hits["id"], hits["dist"], 2, one_seq, q_group=grp, n_groups=wide, q_off=off64)
    want = sr.seq_match(hits, one_seq, grp, off64)
    for f in sr.FIELDS:
        if f != "diag":  # (its low 32 bits)
            assert np.array_equal(got[f], want[f]), f
    assert got["diag"].tolist() == [np.int32(np.uint32((0 - (wide - 10)) & 0xffffffff).astype(np.int64) - wide), 9]
    # merge: zero count, lo > hi, NaN
    row = dict(group=[1], seq=[2], diag=[0], count=[1], best_dist=[1.0], best_q=[4], best_id=[5], lo=[6], hi=[7])
    for change in (dict(count=[0]), dict(lo=[8]), dict(best_dist=[np.nan])):
        outs = [np.full(4, 0x5A, dtype=t) for _, t in capi.SEQ_MATCH_FIELDS]
        with pytest.raises(capi.HsError) as e:
            capi.seq_match_merge([dict(row, **change)], out=outs)
        assert e.value.status == capi.HS_ERR_INVALID and all((o == 0x5A).all() for o in outs)
