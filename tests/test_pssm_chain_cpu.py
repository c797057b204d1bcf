"""hs_pssm_family_chain without a GPU: the host rule (capi.pssm_family_chain_hits) against the contract of
tests/pssm_chain_ref.py, bit for bit, on the hits of tests/pssm_ref.py's scan -- three shapes, every group layout,
shifts from 0 to 65535, three penalty pairs, the filters, shuffled and repeated tuples; the gapped planted proteins that
the family rows lose and the chain keeps; agreement with the family rows at max_shift = 0; ties in every choice and a
tie order that shows; extreme scores; the capacity protocol for rows and paths; every refused input on sentinel-filled
outputs; exports; and the header under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hsearch_amd import HsError, capi

import pssm_chain_ref as ref
import pssm_family_ref as fam
import pssm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(25, 20, 3500), (3, 4, 200), (75, 32, 300)]
PENALTIES = [(0.0, 0.0), (4.0, 1.0), (0.1, 2.0 ** -20)]
SHIFTS = [0, 1, 3, 65535]

_CASES = {}


def _case(k, A, n):
    """codes in sequences of mixed lengths (empty ones among them), 33 profiles with dyadic and real entries, thresholds
    that about a fortieth of the windows reach (one profile: a fifth), and the reference scan's hits"""
    if (k, A, n) not in _CASES:
        rng = np.random.default_rng(100 * k + A)
        codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
        lens = []
        while sum(lens) < n:
            lens.append(int(rng.choice([0, 1, 7, 40, 90, 260])))
        id_start = np.minimum(np.concatenate([[0], np.cumsum(lens)]), n).astype(np.uint64)
        S = rng.normal(0, 2, size=(33, k, A))
        S[::2] = rng.integers(-16, 17, size=S[::2].shape) / 4.0
        sc = pssm_ref.scores(S, codes)
        t = np.sort(sc, axis=1)[:, -max(1, n // 40)].copy()
        t[7] = np.sort(sc[7])[-max(1, n // 5)]
        _CASES[(k, A, n)] = dict(codes=codes, id_start=id_start, S=S, t=t, hits=pssm_ref.scan(S, t, codes), k=k)
    return _CASES[(k, A, n)]


def _hits(case, nm):
    h = case["hits"]
    keep = h["m"] < nm
    return h["m"][keep], h["id"][keep], h["score"][keep]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d" % s[0])
@pytest.mark.parametrize("groups", ["singletons", "one", "mixed"])
def test_hits_rule_equals_reference(shape, groups):
    case = _case(*shape)
    rng = np.random.default_rng(17)
    seen_gap = seen_multi = False
    for nm in (1, 17, 33):
        m_group = fam.group_layouts(nm)[groups]
        m_off = ref.sorted_offsets(m_group, nm, case["k"])
        m, i, sc = _hits(case, nm)
        n_groups = nm if m_group is None else int(m_group.max()) + 1
        t_group = np.sort(sc)[len(sc) // 2] * np.ones(n_groups)           # about the median hit score
        # the tuples shuffled, a fifth of them twice
        p = rng.permutation(np.concatenate([np.arange(len(m)), rng.integers(0, len(m), size=len(m) // 5)]))
        for max_shift in SHIFTS:
            for gap_open, gap_ext in PENALTIES:
                # (the full cross only at the smallest shape; elsewhere every value of every argument, not every pair)
                if shape[0] != 3 and (SHIFTS.index(max_shift) + PENALTIES.index((gap_open, gap_ext))) % 2:
                    continue
                for min_count, tg in ((1, None), (2, t_group), (3, None), (2, None), (1, t_group)):
                    kw = dict(gap_open=gap_open, gap_ext=gap_ext, min_count=min_count, t_group=tg)
                    want = ref.chains_from_hits(m, i, sc, nm, case["id_start"], m_group, m_off, max_shift, **kw)
                    got = capi.pssm_family_chain_hits(m[p], i[p], sc[p], nm, case["id_start"], m_group, m_off, max_shift,
                                                      want_path=True, **kw)
                    ref.same_chains(got, want, (shape, groups, nm, max_shift, gap_open, min_count))
                    assert not np.isnan(got["score"]).any()
                    assert np.all(got["count"] >= min_count) and np.all(got["gaps"] < got["count"])
                    assert len(set(zip(got["group"].tolist(), got["seq"].tolist()))) == len(got["group"])
                    seen_gap |= bool((got["gaps"] > 0).any())
                    seen_multi |= bool((got["count"] > 2).any())
                    if max_shift == 0:
                        assert np.all(got["gaps"] == 0) and np.all(got["shift"] == 0)
                    if groups == "singletons" or nm == 1:
                        assert np.all(got["count"] == 1)
    if groups != "singletons":
        assert seen_gap and seen_multi, (seen_gap, seen_multi)


@pytest.mark.parametrize("ins", [1, 2, 3])
def test_the_gapped_planted_proteins(ins):
    """Seed 20261 with `ins` residues inserted behind motif column 10 in proteins 1, 6, 8, 9: the family rows keep the
    five ungapped proteins, the chain at max_shift = 3 keeps all nine and no decoy."""
    c = ref.planted_gapped(ins=ins)
    assert c["gapped"] == ref.PLANTED_GAPPED and sorted(c["planted"]) == sorted(ref.PLANTED_GAPPED + ref.PLANTED_UNGAPPED)
    hits = pssm_ref.scan(c["S"], c["t"], c["codes"])
    g, off = np.zeros(3, np.uint32), np.array([0, 3, 6], np.uint32)
    args = (hits["m"], hits["id"], hits["score"], 3, c["id_start"])
    rows = capi.pssm_family_hits(*args, m_group=g, m_off=off, min_count=3)
    assert rows["seq"].tolist() == list(ref.PLANTED_UNGAPPED)
    got = capi.pssm_family_chain_hits(*args, g, off, 3, 4.0, 1.0, min_count=3, want_path=True)
    ref.same_chains(got, ref.chains(hits, 3, c["id_start"], g, off, 3, gap_open=4.0, gap_ext=1.0, min_count=3), ins)
    assert got["seq"].tolist() == sorted(c["planted"])
    assert (got["first_id"] - c["id_start"][got["seq"]]).tolist() == [c["planted"][s] for s in got["seq"].tolist()]
    gapped = np.isin(got["seq"], ref.PLANTED_GAPPED)
    assert np.all(got["shift"][gapped] == ins) and np.all(got["gaps"][gapped] == 1)
    assert np.all(got["shift"][~gapped] == 0) and np.all(got["gaps"][~gapped] == 0) and np.all(got["count"] == 3)
    assert 205.25 <= got["score"][gapped].min() and got["score"][gapped].max() <= 209.25
    assert 229.5 <= got["score"][~gapped].min() and got["score"][~gapped].max() <= 244.5
    less = capi.pssm_family_chain_hits(*args, g, off, ins - 1, 4.0, 1.0, min_count=3)
    assert less["seq"].tolist() == list(ref.PLANTED_UNGAPPED)
    # the paths: strictly increasing m and off, `count` hits, and their rescored value is the score, bit for bit
    score_of = dict(zip(zip(hits["m"].tolist(), hits["id"].tolist()), hits["score"].tolist()))
    for r in range(len(got["seq"])):
        a, b = int(got["path_start"][r]), int(got["path_start"][r + 1])
        pm, pid = got["path_m"][a:b].astype(np.int64), got["path_id"][a:b].astype(np.int64)
        assert b - a == got["count"][r] and np.all(np.diff(pm) > 0) and np.all(np.diff(pid) > 0)
        assert (pm[0], pid[0], pm[-1], pid[-1]) == (got["first_m"][r], got["first_id"][r], got["last_m"][r], got["last_id"][r])
        again = ref.rescore(list(zip(pm.tolist(), pid.tolist())), score_of, off, c["id_start"], 4.0, 1.0)
        assert np.float64(again).view(np.uint64) == got["score"][r:r + 1].view(np.uint64)[0]
    # at max_shift = 0 the chain is the family row: the same proteins, the rows' sum bit for bit
    zero = capi.pssm_family_chain_hits(*args, g, off, 0, 4.0, 1.0, min_count=3)
    assert zero["seq"].tolist() == rows["seq"].tolist()
    assert np.array_equal(zero["score"].view(np.uint64), rows["sum"].view(np.uint64))


@pytest.mark.parametrize("groups", ["one", "mixed"])
def test_zero_shift_agrees_with_the_family_rows(groups):
    """max_shift = 0, every hit score positive, offsets strictly increasing inside groups: a (g, s) row's score is the
    largest sum among the family rows of that (g, s) with count >= min_count."""
    k, A, n = SHAPES[0]
    case = _case(k, A, n)
    nm = 17
    m_group = fam.group_layouts(nm)[groups]
    m_off = np.zeros(nm, np.uint32)
    for x in range(1, nm):
        m_off[x] = m_off[x - 1] + 1 + x % 3 if m_group[x] == m_group[x - 1] else 0
    sc_all = pssm_ref.scores(case["S"][:nm], case["codes"])
    t = np.maximum(np.sort(sc_all, axis=1)[:, -n // 12], 0.25)            # thresholds above 0: every hit is positive
    hits = pssm_ref.scan(case["S"][:nm], t, case["codes"])
    assert hits["score"].min() > 0
    args = (hits["m"], hits["id"], hits["score"], nm, case["id_start"])
    for min_count in (1, 2, 3):
        got = capi.pssm_family_chain_hits(*args, m_group, m_off, 0, 4.0, 1.0, min_count=min_count)
        rows = capi.pssm_family_hits(*args, m_group=m_group, m_off=m_off, min_count=min_count)
        best = {}
        for g, s, v in zip(rows["group"].tolist(), rows["seq"].tolist(), rows["sum"].tolist()):
            best[(g, s)] = max(best.get((g, s), -np.inf), v)
        assert list(zip(got["group"].tolist(), got["seq"].tolist())) == sorted(best)
        want = np.array([best[key] for key in sorted(best)])
        assert np.array_equal(got["score"].view(np.uint64), want.view(np.uint64)) and len(want) > 10
        assert (got["count"] >= 2).any()


def test_ties_fill_every_choice():
    """Constant profiles over a 4-letter alphabet at k = 3: every hit scores the same, so predecessors tie in v, then in
    n, and ends tie in C and n.  The rule's orders decide, and another order gives other rows."""
    k, A, n = 3, 4, 200
    rng = np.random.default_rng(2)
    codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
    nm = 6
    S = np.full((nm, k, A), 0.5)
    hits = pssm_ref.scan(S, np.full(nm, 1.0), codes)                      # every window, every profile: 1.5
    assert len(hits["m"]) == nm * n
    id_start = np.array([0, 50, 50, 120, 200], dtype=np.uint64)
    m_group = np.array([0, 0, 0, 0, 1, 1], np.uint32)
    m_off = np.array([0, 0, 1, 1, 0, 2], np.uint32)                       # equal offsets: the same diagonal twice
    args = (hits["m"], hits["id"], hits["score"], nm, id_start)
    differ = 0
    for max_shift, pen in ((0, (0.0, 0.0)), (2, (0.0, 0.0)), (2, (0.5, 0.25))):
        kw = dict(gap_open=pen[0], gap_ext=pen[1], min_count=2)
        got = capi.pssm_family_chain_hits(*args, m_group, m_off, max_shift, want_path=True, **kw)
        want = ref.chains(hits, nm, id_start, m_group, m_off, max_shift, **kw)
        ref.same_chains(got, want, ("ties", max_shift, pen))
        # (two profiles at one offset cannot both lie on one diagonal at increasing off: two blocks at max_shift = 0)
        assert got["count"].max() == (2 if max_shift == 0 else 4)
        other = ref.chains(hits, nm, id_start, m_group, m_off, max_shift, pred_m_ascending=True, **kw)
        differ += sum(a != b for a, b in zip(want["path"], other["path"]))
    assert differ > 0                                                     # the predecessor tie order shows


def test_extreme_scores_give_no_nan():
    k, A = 25, 20
    rng = np.random.default_rng(3)
    codes = rng.integers(0, A, size=(300, k)).astype(np.uint8)
    id_start = np.array([0, 100, 300], dtype=np.uint64)
    S3 = fam.order_sensitive_profiles(k, A)                               # scores of the order 2^40, 1 and 2^-12
    S = np.concatenate([S3, rng.normal(0, 1, size=(3, k, A))])
    S[3, :, 0] = -1e30
    S[4, 0, :] = 2.0 ** 100
    S[5, 1, :] = -(2.0 ** 100)
    S[5, 2, :] = 2.0 ** 100
    hits = pssm_ref.scan(S, np.full(6, -1e300), codes)
    g = np.array([0, 0, 0, 1, 1, 1], np.uint32)
    off = np.array([0, 1, 2, 0, 0, 3], np.uint32)
    for max_shift, pen in ((0, (0.0, 0.0)), (3, (4.0, 1.0)), (65535, (1e300, 1e300))):
        kw = dict(gap_open=pen[0], gap_ext=pen[1])
        got = capi.pssm_family_chain_hits(hits["m"], hits["id"], hits["score"], 6, id_start, g, off, max_shift, **kw)
        ref.same_chains(got, ref.chains(hits, 6, id_start, g, off, max_shift, **kw), ("extreme", max_shift))
        assert not np.isnan(got["score"]).any() and np.isfinite(got["score"]).all() and len(got["score"]) == 4


def test_a_large_penalty_takes_no_gapped_link():
    case = _case(*SHAPES[1])
    nm = 17
    m_group = fam.group_layouts(nm)["one"]
    m_off = ref.sorted_offsets(m_group, nm, 3)
    m, i, sc = _hits(case, nm)
    free = capi.pssm_family_chain_hits(m, i, sc, nm, case["id_start"], m_group, m_off, 3)
    assert (free["gaps"] > 0).any()
    dear = capi.pssm_family_chain_hits(m, i, sc, nm, case["id_start"], m_group, m_off, 3, gap_open=1e6)
    assert np.all(dear["gaps"] == 0) and np.all(dear["shift"] == 0)
    # ... and with a penalty on every link there is none: shift the offsets so that no two hits share a diagonal
    far = (np.arange(nm) * 1000).astype(np.uint32)
    alone = capi.pssm_family_chain_hits(m, i, sc, nm, case["id_start"], m_group, far, 65535, gap_open=1e6)
    assert np.all(alone["count"] == 1) and len(alone["count"]) == len(free["count"])
    ref.same_chains(alone, ref.chains_from_hits(m, i, sc, nm, case["id_start"], m_group, far, 65535, gap_open=1e6), "alone")


def _raw(lib, m, i, sc, nm, m_group, n_groups, m_off, id_start, max_shift, gap_open, gap_ext, min_count, t_group, outs,
         cap, n_out, path=(None, None, None), path_cap=0, n_path=None):
    a = [None if x is None else np.ascontiguousarray(x, dtype=t)
         for x, t in ((m, np.uint32), (i, np.uint32), (sc, np.float64), (m_group, np.uint32), (m_off, np.uint32),
                      (id_start, np.uint64), (t_group, np.float64))]
    vp = [None if x is None else capi._vp(x) for x in a]
    return lib.hs_pssm_family_chain_hits(vp[0], vp[1], vp[2], len(a[0]), nm, vp[3], n_groups, vp[4], vp[5],
                                         0 if a[5] is None else len(a[5]) - 1, max_shift, gap_open, gap_ext, min_count,
                                         vp[6], *[None if o is None else capi._vp(o) for o in outs], cap,
                                         None if n_out is None else C.byref(n_out),
                                         *[None if x is None else capi._vp(x) for x in path], path_cap,
                                         None if n_path is None else C.byref(n_path))


def test_capacity_protocol_for_rows_and_paths():
    case = _case(*SHAPES[1])
    nm = 17
    m_group = fam.group_layouts(nm)["mixed"]
    m_off = ref.sorted_offsets(m_group, nm, 3)
    m, i, sc = _hits(case, nm)
    full = capi.pssm_family_chain_hits(m, i, sc, nm, case["id_start"], m_group, m_off, 3, want_path=True)
    n_rows, n_path = len(full["group"]), len(full["path_m"])
    assert n_rows > 10 and n_path == int(full["count"].sum()) > n_rows
    lib = capi.load()
    ng = int(m_group.max()) + 1
    n_out, npth = C.c_uint64(0), C.c_uint64(0)
    st = _raw(lib, m, i, sc, nm, m_group, ng, m_off, case["id_start"], 3, 0.0, 0.0, 1, None, [None] * 10, 0, n_out)
    assert st == capi.HS_ERR_CAPACITY and n_out.value == n_rows
    out = [np.full(n_rows - 1, 9, dtype=t) for _, t in capi.PSSM_CHAIN_FIELDS]
    with pytest.raises(HsError) as e:
        capi.pssm_family_chain_hits(m, i, sc, nm, case["id_start"], m_group, m_off, 3, cap=n_rows - 1, out=out)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == n_rows and all(np.all(a == 9) for a in out)
    out = [np.full(n_rows + 1, 9, dtype=t) for _, t in capi.PSSM_CHAIN_FIELDS]
    ref.same_chains(capi.pssm_family_chain_hits(m, i, sc, nm, case["id_start"], m_group, m_off, 3, cap=n_rows + 1,
                                                out=out), full, "exact cap")
    assert all(a[n_rows] == 9 for a in out)
    # the path: too small a path_cap writes nothing, rows included
    out = [np.full(n_rows, 9, dtype=t) for _, t in capi.PSSM_CHAIN_FIELDS]
    ps, pm, pid = np.full(n_rows + 1, 9, np.uint64), np.full(n_path, 9, np.uint32), np.full(n_path, 9, np.uint32)
    st = _raw(lib, m, i, sc, nm, m_group, ng, m_off, case["id_start"], 3, 0.0, 0.0, 1, None, out, n_rows, n_out,
              (ps, pm, pid), n_path - 1, npth)
    assert st == capi.HS_ERR_CAPACITY and n_out.value == n_rows and npth.value == n_path
    assert all(np.all(a == 9) for a in out + [ps, pm, pid])
    st = _raw(lib, m, i, sc, nm, m_group, ng, m_off, case["id_start"], 3, 0.0, 0.0, 1, None, out, n_rows, n_out,
              (ps, pm, pid), n_path, npth)
    assert st == capi.HS_OK and np.array_equal(ps, full["path_start"]) and np.array_equal(pm, full["path_m"])
    assert np.array_equal(pid, full["path_id"])
    with pytest.raises(HsError) as e:
        capi.pssm_family_chain_hits(m, i, sc, nm, case["id_start"], m_group, m_off, 3, want_path=True, path_cap=3)
    assert e.value.needed_path == n_path


def test_refused_inputs_write_nothing():
    lib = capi.load()
    m = np.array([0, 0, 1], np.uint32)
    i = np.array([4, 4, 6], np.uint32)
    good = np.array([0, 3, 10], np.uint64)
    out = [np.full(4, 9, dtype=t) for _, t in capi.PSSM_CHAIN_FIELDS]
    n_out = C.c_uint64(5)

    def call(ss=(1.0, 1.0, 0.5), nm=2, id_start=good, m_group=(0, 0), n_groups=1, m_off=(0, 1), max_shift=2,
             gap_open=1.0, gap_ext=0.5, min_count=1, t_group=None, outs=out, n=n_out, **kw):
        return _raw(lib, m, i, ss, nm, m_group, n_groups, m_off, id_start, max_shift, gap_open, gap_ext, min_count,
                    t_group, outs, 4, n, **kw)

    bad = capi.HS_ERR_INVALID
    assert call(m_off=None) == bad and n_out.value == 0                  # m_off is required
    assert call(m_off=[1, 0]) == bad                                     # decreases inside a group
    assert call(m_off=[1, 0], m_group=[0, 1], n_groups=2) == capi.HS_OK  # ... but not across a group boundary
    assert call(m_off=[1, 0], m_group=None, n_groups=2) == capi.HS_OK
    assert call(m_off=[1, 1]) == capi.HS_OK                              # equal offsets are in order
    for a in out:
        a[:] = 9
    assert call(max_shift=65536) == bad and call(max_shift=65535) == capi.HS_OK
    for a in out:
        a[:] = 9
    for x in (np.nan, np.inf, -np.inf, -1.0, -5e-324):
        assert call(gap_open=x) == bad and call(gap_ext=x) == bad, x
    assert call(min_count=0) == bad
    # the family rule's own refusals
    assert call(ss=[1.0, 2.0, 0.5]) == bad                               # two scores for (0, 4)
    assert call(ss=[1.0, 1.0, np.nan]) == bad and call(ss=[1.0, 1.0, np.inf]) == bad
    assert call(nm=1, m_group=[0], m_off=[0]) == bad                     # m >= nm
    assert call(id_start=[0, 3, 6]) == bad                               # an id at id_start[n_seq]
    assert call(id_start=[1, 3, 10]) == bad and call(id_start=[0, 11, 10]) == bad and call(id_start=[0]) == bad
    assert call(id_start=None) == bad
    assert call(m_group=[1, 0], n_groups=2, m_off=[0, 0]) == bad         # m_group decreases
    assert call(m_group=[0, 1], n_groups=1) == bad                       # a value >= n_groups
    assert call(m_group=None, n_groups=1) == bad                         # n_groups != nm without m_group
    assert call(t_group=[np.nan]) == bad and call(t_group=[np.inf]) == bad
    assert call(m_off=[0, 1 << 31]) == bad                               # an offset above 2^31 - 1
    assert call(n_groups=(1 << 32) + 1) == bad
    assert call(outs=out[:4] + [None] + out[5:]) == bad                  # a null output with cap > 0
    assert call(n=None) == bad
    ps, pm = np.full(5, 9, np.uint64), np.full(4, 9, np.uint32)
    assert call(path=(ps, pm, None), path_cap=4, n_path=C.c_uint64(0)) == bad     # a path array missing
    assert call(path=(ps, pm, pm), path_cap=4, n_path=None) == bad
    assert all(np.all(a == 9) for a in out + [ps, pm])
    big = np.zeros(4097, np.uint32)                                      # a group of 4097 profiles
    assert call(nm=4097, m_group=big, m_off=big) == bad and all(np.all(a == 9) for a in out)
    assert call(nm=4096, m_group=big[:4096], m_off=big[:4096]) == capi.HS_OK
    for a in out:
        a[:] = 9
    # -0.0: a score and both penalties are read as +0.0
    assert call(ss=[1.0, 1.0, -0.0], gap_open=-0.0, gap_ext=-0.0) == capi.HS_OK and n_out.value == 1
    # (0, 4) and (1, 6) lie one diagonal apart in sequence 1; the free link is taken: two blocks, one gap, 1.0 + 0.0
    assert [int(a[0]) for a in out[:4]] == [0, 1, 2, 1] and out[4][0] == 1.0 and [int(a[0]) for a in out[5:]] == [0, 4, 1, 6, 1]
    assert call(ss=[1.0, 1.0, -0.0], m_group=[0, 1], n_groups=2, m_off=[0, 0]) == capi.HS_OK and n_out.value == 2
    assert out[4][:2].tolist() == [1.0, 0.0] and not np.signbit(out[4][1])
    with pytest.raises(HsError):
        capi.pssm_family_chain_hits([0], [1], [1.0], 1, [0, 2], None, None, 0)
    assert len(capi.pssm_family_chain_hits([], [], [], 0, [0], None, None, 3)["group"]) == 0


def test_exports_and_profile_fields():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in ("hs_pssm_family_chain", "hs_pssm_family_chain_dev", "hs_pssm_family_chain_hits"):
        assert re.search(r"HS_API hs_status %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name)
    for name in ("pssm_family_chain", "pssm_family_chain_dev"):
        assert callable(getattr(capi.Engine, name))
    assert [f for f, _ in capi.PSSM_CHAIN_FIELDS] == list(ref.FIELDS)
    assert [np.dtype(t) for _, t in capi.PSSM_CHAIN_FIELDS] == [np.dtype(t) for t in ref.TYPES]
    fields = [f for f, _ in capi._Profile._fields_]
    at = fields.index("pssm_fam_kept")
    assert fields[at + 1:at + 3] == ["pssm_chain_segs", "pssm_chain_kept"]
    struct = header[header.index("typedef struct hs_profile"):header.index("} hs_profile;")]
    declared = re.findall(r"^\s*(?:double|uint64_t|uint32_t)\s+(\w+);", struct, flags=re.M)
    assert declared == fields
    chain_h = open(os.path.join(ROOT, "hsearch_amd", "csrc", "hs_pssm_chain.h")).read()
    assert "#include <hip" not in chain_h and "__global__" not in chain_h     # host-compilable: no HIP in it
    assert re.search(r"#define HS_PSSM_CHAIN_MAX_SHIFT 65535u", chain_h)
    assert re.search(r"HS_FAM_BAD_OFF_ORDER = 32\b", open(os.path.join(ROOT, "hsearch_amd", "csrc", "hs_pssm_family.h")).read())


def test_header_under_asan_and_ubsan(tmp_path):
    """hs_pssm_chain.h with a stand-alone main (tests/pssm_chain_san.cpp), compiled and run under AddressSanitizer +
    UndefinedBehaviorSanitizer (the runtimes linked statically); nothing is loaded into python."""
    exe = tmp_path / "pssm_chain_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "pssm_chain_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pssm_chain_san ok" in res.stdout
