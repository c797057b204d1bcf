"""hs_pssm_family_scan without a GPU: the host rules (capi.pssm_family_hits, capi.pssm_family_layout) against the
contracts of tests/pssm_family_ref.py, bit for bit -- shuffled and repeated tuples under every group layout with and
without offsets, the filters, the capacity protocol, every refused input on sentinel-filled outputs; chains, families,
an inconsistent triangle and an oversized component for the layout; the constructions the GPU tests rely on (an order
of the sum that matters, a planted motif that only the family finds cleanly); and the header under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hsearch_amd import HsError, capi

import pssm_family_ref as ref
import pssm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# id_start arrays over 60 ids: empty sequences at the start, in the middle and at the end; one sequence
LAYOUTS = [[0, 0, 0, 5, 5, 5, 12, 40, 40, 41, 60, 60, 60], [0, 60], [0, 1, 2, 3, 60]]
NM = 11


def _tuples(rng, nm, n, nt):
    """a score per (m, id) -- small dyadic values (heavy ties), negative ones and +0.0 --, nt shuffled tuples with
    repeats, and the distinct ones"""
    table = rng.integers(-6, 7, size=(nm, n)) / 4.0
    m = rng.integers(0, nm, size=nt).astype(np.uint32)
    i = rng.integers(0, n, size=nt).astype(np.uint32)
    present = np.zeros((nm, n), dtype=bool)
    present[m, i] = True
    dm, di = np.nonzero(present)
    return table, m, i, dm, di


@pytest.mark.parametrize("groups", ["singletons", "one", "mixed"])
@pytest.mark.parametrize("with_off", [False, True])
def test_hits_rule_equals_reference(groups, with_off):
    m_group = ref.group_layouts(NM)[groups]
    m_off = ref.offsets_in_groups(m_group, NM, 6) if with_off else None
    rng = np.random.default_rng(7)
    for layout in LAYOUTS:
        id_start = np.array(layout, dtype=np.uint64)
        n = int(id_start[-1])
        for nt in (0, 40, 900):
            table, m, i, dm, di = _tuples(rng, NM, n, nt)
            kw = dict(m_group=m_group, m_off=m_off)
            got = capi.pssm_family_hits(m, i, table[m, i], NM, id_start, **kw)
            want = ref.rows_from_hits(dm, di, table[dm, di], NM, id_start, **kw)
            ref.same_rows(got, want, (groups, with_off, layout, nt))
            assert int(got["count"].sum()) == len(dm) and np.all(got["lo"] <= got["hi"])
            if with_off and nt == 900:
                assert (got["diag"] < 0).any() and (got["diag"] > 0).any()
            if not with_off:
                assert np.all(got["diag"] == 0)
            if nt == 900:
                assert len(dm) < nt                                   # repeats really occur
                assert (got["count"] > 1).any() or groups == "singletons" and with_off
            p = rng.permutation(nt)
            ref.same_rows(capi.pssm_family_hits(m[p], i[p], table[m, i][p], NM, id_start, **kw), got, "permuted")
            # the filters: min_count, and a threshold on the sum per group
            n_groups = NM if m_group is None else int(m_group.max()) + 1
            t_group = rng.integers(-4, 5, size=n_groups) / 4.0
            for min_count in (1, 2, 3):
                kw2 = dict(kw, min_count=min_count, t_group=t_group)
                ref.same_rows(capi.pssm_family_hits(m, i, table[m, i], NM, id_start, **kw2),
                              ref.rows_from_hits(dm, di, table[dm, di], NM, id_start, **kw2), ("filters", min_count))


def test_filters_at_the_edge():
    """t_group exactly at a row's sum keeps the row; the next double above drops it"""
    id_start = np.array([0, 30], dtype=np.uint64)
    m, i, sc = [0, 1, 2], [5, 6, 7], [0.1, 0.2, 0.3]
    kw = dict(m_group=[0, 0, 0], m_off=[0, 1, 2])
    row = capi.pssm_family_hits(m, i, sc, 3, id_start, **kw)
    assert row["count"].tolist() == [3] and row["diag"].tolist() == [5] and row["sum"][0] == (0.0 + 0.1 + 0.2) + 0.3
    assert row["sum"][0] != 0.1 + (0.2 + 0.3)                        # the order shows even here
    s = float(row["sum"][0])
    assert len(capi.pssm_family_hits(m, i, sc, 3, id_start, t_group=[s], **kw)["sum"]) == 1
    assert len(capi.pssm_family_hits(m, i, sc, 3, id_start, t_group=[np.nextafter(s, np.inf)], **kw)["sum"]) == 0
    assert len(capi.pssm_family_hits(m, i, sc, 3, id_start, min_count=3, **kw)["sum"]) == 1
    assert len(capi.pssm_family_hits(m, i, sc, 3, id_start, min_count=4, **kw)["sum"]) == 0
    # the best of a tie: the smaller m, then the smaller id
    tie = capi.pssm_family_hits([1, 0, 0], [9, 4, 3], [2.0, 2.0, 2.0], 2, id_start, m_group=[0, 0])
    assert tie["best_m"].tolist() == [0] and tie["best_id"].tolist() == [3] and tie["count"].tolist() == [3]
    assert tie["lo"].tolist() == [3] and tie["hi"].tolist() == [9]


def test_the_order_of_the_sum_matters():
    """The construction the GPU test of the order rests on: over profiles scaled by 2^40, 1 and 2^-12 in one group, the
    sum taken in the reversed order has other bits in at least one row."""
    k, A = 25, 20
    rng = np.random.default_rng(3)
    codes = rng.integers(0, A, size=(300, k)).astype(np.uint8)
    S = ref.order_sensitive_profiles(k, A)
    hits = pssm_ref.scan(S, np.full(3, -1e300), codes)
    id_start = np.array([0, 300], dtype=np.uint64)
    kw = dict(m_group=np.zeros(3, np.uint32), m_off=np.zeros(3, np.uint32))
    want = ref.rows(hits, 3, id_start, **kw)
    back = ref.rows(hits, 3, id_start, reverse_sum=True, **kw)
    assert np.all(want["count"] == 3) and len(want["sum"]) == 300
    differ = int((want["sum"].view(np.uint64) != back["sum"].view(np.uint64)).sum())
    assert differ >= 10, differ
    ref.same_rows(capi.pssm_family_hits(hits["m"], hits["id"], hits["score"], 3, id_start, **kw), want, "forward")


def test_capacity_protocol():
    id_start = np.array(LAYOUTS[0], dtype=np.uint64)
    rng = np.random.default_rng(5)
    table, m, i, dm, di = _tuples(rng, 3, 60, 2000)
    rows = capi.pssm_family_hits(m, i, table[m, i], 3, id_start, m_group=[0, 0, 1])
    n_rows = len(rows["group"])
    assert n_rows == 2 * 5
    lib = capi.load()
    n_out = C.c_uint64(0)
    grp = np.array([0, 0, 1], np.uint32)
    st = lib.hs_pssm_family_hits(capi._vp(m), capi._vp(i), capi._vp(table[m, i]), 2000, 3, capi._vp(grp), 2, None,
                                 capi._vp(id_start), 12, 1, None, *[None] * 10, 0, C.byref(n_out))
    assert st == capi.HS_ERR_CAPACITY and n_out.value == n_rows
    out = [np.full(n_rows - 1, 9, dtype=t) for _, t in capi.PSSM_FAMILY_FIELDS]
    with pytest.raises(HsError) as e:
        capi.pssm_family_hits(m, i, table[m, i], 3, id_start, m_group=grp, cap=n_rows - 1, out=out)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == n_rows
    assert all(np.all(a == 9) for a in out)
    out = [np.full(n_rows + 1, 9, dtype=t) for _, t in capi.PSSM_FAMILY_FIELDS]
    ref.same_rows(capi.pssm_family_hits(m, i, table[m, i], 3, id_start, m_group=grp, cap=n_rows + 1, out=out), rows,
                  "exact cap")
    assert all(a[n_rows] == 9 for a in out)


def test_refused_inputs_write_nothing():
    lib = capi.load()
    m = np.array([0, 0, 1], np.uint32)
    i = np.array([4, 4, 2], np.uint32)
    good = np.array([0, 3, 10], np.uint64)
    out = [np.full(4, 9, dtype=t) for _, t in capi.PSSM_FAMILY_FIELDS]
    n_out = C.c_uint64(5)

    def call(ss=(1.0, 1.0, 0.5), nm=2, id_start=good, n_seq=None, m_group=(0, 0), n_groups=1, m_off=(0, 1),
             min_count=1, t_group=None, outs=out, n=n_out):
        ss = np.asarray(ss, np.float64)
        ids = None if id_start is None else np.asarray(id_start, np.uint64)
        n_seq = len(ids) - 1 if n_seq is None else n_seq
        mg = None if m_group is None else np.asarray(m_group, np.uint32)
        mo = None if m_off is None else np.asarray(m_off, np.uint32)
        tg = None if t_group is None else np.asarray(t_group, np.float64)
        return lib.hs_pssm_family_hits(capi._vp(m), capi._vp(i), capi._vp(ss), 3, nm, None if mg is None else capi._vp(mg),
                                       n_groups, None if mo is None else capi._vp(mo),
                                       None if ids is None else capi._vp(ids), n_seq, min_count,
                                       None if tg is None else capi._vp(tg),
                                       *[None if a is None else capi._vp(a) for a in outs], 4,
                                       None if n is None else C.byref(n))

    bad = capi.HS_ERR_INVALID
    assert call(ss=[1.0, 2.0, 0.5]) == bad and n_out.value == 0          # two scores for (0, 4)
    assert call(ss=[1.0, 1.0, np.nan]) == bad                            # a NaN
    assert call(nm=1, m_group=[0], m_off=[0]) == bad                     # m >= nm
    assert call(id_start=[0, 3, 4]) == bad                               # an id at id_start[n_seq]
    assert call(id_start=[1, 3, 10]) == bad                              # does not start at 0
    assert call(id_start=[0, 11, 10]) == bad                             # does not ascend
    assert call(id_start=[0]) == bad                                     # no sequence owns the ids
    assert call(id_start=None, n_seq=2) == bad                           # a null id_start
    assert call(m_group=[1, 0], n_groups=2) == bad                       # m_group decreases
    assert call(m_group=[0, 1], n_groups=1) == bad                       # a value >= n_groups
    assert call(m_group=None, n_groups=1) == bad                         # n_groups != nm without m_group
    assert call(min_count=0) == bad
    assert call(t_group=[np.nan]) == bad and call(t_group=[np.inf]) == bad and call(t_group=[-np.inf]) == bad
    assert call(m_off=[0, 1 << 31]) == bad                               # an offset above 2^31 - 1
    assert call(n_groups=(1 << 32) + 1) == bad
    assert call(outs=out[:4] + [None] + out[5:]) == bad                  # a null output with cap > 0
    assert call(n=None) == bad
    assert all(np.all(a == 9) for a in out)
    big = np.zeros(4097, np.uint32)                                      # a group of 4097 profiles
    assert call(nm=4097, m_group=big, m_off=big) == bad and all(np.all(a == 9) for a in out)
    assert call(nm=4096, m_group=big[:4096], m_off=big[:4096]) == capi.HS_OK
    for a in out:
        a[:] = 9
    assert call(ss=[1.0, 1.0, -0.0]) == capi.HS_OK and n_out.value == 2
    assert out[0][:2].tolist() == [0, 0] and out[1][:2].tolist() == [0, 1] and out[2][:2].tolist() == [1, 1]
    assert out[3][:2].tolist() == [1, 1] and out[6][:2].tolist() == [1, 0] and out[7][:2].tolist() == [2, 4]
    assert not np.signbit(out[4][0]) and not np.signbit(out[5][0]) and out[4][0] == 0.0
    with pytest.raises(HsError):
        capi.pssm_family_hits([0], [1], [np.nan], 1, [0, 2])
    assert len(capi.pssm_family_hits([], [], [], 0, [0])["group"]) == 0


def _same_layout(got, want, what=""):
    for f in ("group", "off", "order"):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f, got[f], want[f])
    assert (got["n_groups"], got["n_conflicts"]) == (want["n_groups"], want["n_conflicts"]), what


def test_layout_chain_families_and_conflicts():
    # windows of one motif at shifts 0, 3, 6, 9 as all pairs in (x, y) order, and as a spanning set
    shifts = [0, 3, 6, 9]
    pairs = [(x, y, shifts[y] - shifts[x]) for x in range(4) for y in range(x + 1, 4)]
    for hits in (pairs, [pairs[0], pairs[3], pairs[5]], [pairs[5], pairs[4], pairs[2]]):
        x, y, d = zip(*hits)
        got = capi.pssm_family_layout(x, y, d, 4)
        _same_layout(got, ref.layout(x, y, d, 4), hits)
        assert got["off"].tolist() == shifts and got["n_groups"] == 1 and got["order"].tolist() == [0, 1, 2, 3]
    # two families and a loner, profiles interleaved and hits with x > y; family 1's first member is not its leftmost
    x, y, d = [4, 0, 5, 3], [2, 2, 1, 5], [-4, 2, 5, -7]
    got = capi.pssm_family_layout(x, y, d, 7)
    _same_layout(got, ref.layout(x, y, d, 7), "two families")
    assert got["group"].tolist() == [0, 1, 0, 1, 0, 1, 2] and got["n_groups"] == 3 and got["n_conflicts"] == 0
    assert got["off"].tolist() == [0, 5, 2, 7, 6, 0, 0] and got["order"].tolist() == [0, 2, 4, 5, 1, 3, 6]
    # an inconsistent triangle: one conflict, the layout of the first two hits
    got = capi.pssm_family_layout([0, 1, 0], [1, 2, 2], [3, 3, 7], 3)
    _same_layout(got, ref.layout([0, 1, 0], [1, 2, 2], [3, 3, 7], 3), "triangle")
    assert got["n_conflicts"] == 1 and got["off"].tolist() == [0, 3, 6]
    assert capi.pssm_family_layout([0, 1, 0], [1, 2, 2], [3, 3, 6], 3)["n_conflicts"] == 0
    # the order of the hits decides which of two disagreeing ones wins
    assert capi.pssm_family_layout([0, 0], [1, 1], [2, 5], 2)["off"].tolist() == [0, 2]
    assert capi.pssm_family_layout([0, 0], [1, 1], [5, 2], 2)["off"].tolist() == [0, 5]
    # random forests with extra, partly inconsistent hits
    rng = np.random.default_rng(9)
    for nm in (1, 2, 30, 200):
        nh = 0 if nm == 1 else 2 * nm
        x = rng.integers(0, nm, size=nh)
        y = (x + 1 + rng.integers(0, max(nm - 1, 1), size=nh)) % nm
        pos = rng.integers(-40, 40, size=nm)
        d = pos[y] - pos[x] + (rng.random(nh) < 0.1) * rng.integers(1, 4, size=nh)
        keep = rng.random(nh) < 0.4
        got = capi.pssm_family_layout(x[keep], y[keep], d[keep], nm)
        _same_layout(got, ref.layout(x[keep], y[keep], d[keep], nm), nm)
        assert sorted(got["order"].tolist()) == list(range(nm))
    empty = capi.pssm_family_layout([], [], [], 3)
    assert empty["group"].tolist() == [0, 1, 2] and empty["off"].tolist() == [0, 0, 0] and empty["n_groups"] == 3


def test_layout_refusals_write_nothing():
    lib = capi.load()

    def refused(x, y, d, nm):
        x, y, d = np.asarray(x, np.uint32), np.asarray(y, np.uint32), np.asarray(d, np.int32)
        out = [np.full(nm, 9, np.uint32) for _ in range(3)]
        ng, nc = C.c_uint64(7), C.c_uint64(7)
        st = lib.hs_pssm_family_layout(capi._vp(x), capi._vp(y), capi._vp(d), len(x), nm, *[capi._vp(a) for a in out],
                                       C.byref(ng), C.byref(nc))
        assert all(np.all(a == 9) for a in out) and ng.value == 7 and nc.value == 7
        return st == capi.HS_ERR_INVALID

    assert refused([0, 1], [1, 1], [1, 1], 3)                            # x == y
    assert refused([0, 3], [1, 1], [1, 1], 3)                            # an index >= nm
    assert refused([0], [1], [1 << 30], 3) and refused([0], [1], [-(1 << 30)], 3)
    big = (1 << 30) - 1
    assert refused([0, 1, 2], [1, 2, 3], [big, big, 5], 4)               # an offset passes 2^31 - 1
    assert capi.pssm_family_layout([0, 1, 2], [1, 2, 3], [big, big, 1], 4)["off"][3] == (1 << 31) - 1
    chain = np.arange(4097)
    assert refused(chain[1:], chain[:-1], np.full(4096, -1), 4097)       # a component of 4097
    ok = capi.pssm_family_layout(chain[1:-1], chain[:-2], np.full(4095, -1), 4097)
    assert ok["n_groups"] == 2 and ok["off"][:4096].tolist() == list(range(4096)) and ok["group"][4096] == 1
    with pytest.raises(HsError):
        capi.pssm_family_layout([0], [0], [1], 2)


def test_the_planted_motif_is_a_test():
    """Seed 20261: 9 of 40 proteins carry a 31-residue motif with three substitutions each.  On the reference, the chain
    compare -> layout -> family rows with min_count = 3 reports exactly the planted proteins at the planted position,
    and every single profile alone also hits decoys."""
    c = ref.planted_case()
    assert len(c["planted"]) == 9 and 3000 < len(c["codes"]) < 4000
    X = capi.pssm_compare_columns(c["S"], "pearson")
    h = capi.pssm_compare_host(X, 10.0, None, 13)
    assert list(zip(h["x"].tolist(), h["y"].tolist(), h["d"].tolist())) == [(0, 1, 3), (0, 2, 6), (1, 2, 3)]
    lay = capi.pssm_family_layout(h["x"], h["y"], h["d"], 3)
    assert lay["group"].tolist() == [0, 0, 0] and lay["off"].tolist() == c["shifts"].tolist() and lay["n_conflicts"] == 0
    hits = pssm_ref.scan(c["S"], c["t"], c["codes"])
    rows = ref.rows(hits, 3, c["id_start"], m_group=lay["group"], m_off=lay["off"], min_count=3)
    assert dict(zip(rows["seq"].tolist(), rows["diag"].tolist())) == c["planted"] and len(rows["seq"]) == 9
    alone = ref.rows(hits, 3, c["id_start"])                  # every profile its own family
    for m in range(3):
        decoys = set(alone["seq"][alone["group"] == m].tolist()) - set(c["planted"])
        assert len(decoys) >= 5, (m, decoys)
    ref.same_rows(capi.pssm_family_hits(hits["m"], hits["id"], hits["score"], 3, c["id_start"], m_group=lay["group"],
                                        m_off=lay["off"], min_count=3), rows, "planted")


def test_exports_and_profile_fields():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in ("hs_pssm_family_scan", "hs_pssm_family_scan_dev", "hs_pssm_family_hits", "hs_pssm_family_layout"):
        assert re.search(r"HS_API hs_status %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name)
    for name in ("pssm_family_scan", "pssm_family_scan_dev"):
        assert callable(getattr(capi.Engine, name))
    assert [f for f, _ in capi.PSSM_FAMILY_FIELDS] == list(ref.FIELDS)
    fields = [f for f, _ in capi._Profile._fields_]
    at = fields.index("pssm_fam_rows")
    assert fields[at + 1] == "pssm_fam_kept" and at + 1 < fields.index("pssm_rank_sample")
    struct = header[header.index("typedef struct hs_profile"):header.index("} hs_profile;")]
    declared = re.findall(r"^\s*(?:double|uint64_t|uint32_t)\s+(\w+);", struct, flags=re.M)
    assert declared == fields


def test_header_under_asan_and_ubsan(tmp_path):
    """hs_pssm_family.h with a stand-alone main (tests/pssm_family_san.cpp), compiled and run under AddressSanitizer +
    UndefinedBehaviorSanitizer (the runtimes linked statically); nothing is loaded into python."""
    exe = tmp_path / "pssm_family_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "pssm_family_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pssm_family_san ok" in res.stdout
