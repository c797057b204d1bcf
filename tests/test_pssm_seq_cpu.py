"""hs_pssm_seq_scan without a GPU: the host rule (capi.pssm_seq_hits) against the numpy contract of
tests/pssm_seq_ref.py, bit for bit -- shuffled and repeated tuples, empty sequences at the start, in the middle and at
the end, one sequence, the capacity protocol, every refused input -- and the header under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hsearch_amd import HsError, capi

import pssm_ref
import pssm_seq_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# id_start arrays over 60 ids: empty sequences at the start, in the middle and at the end; one sequence; sequences
# of one id; everything in the one sequence between two empty ones
LAYOUTS = [[0, 0, 0, 5, 5, 5, 12, 40, 40, 41, 60, 60, 60], [0, 60], [0, 1, 2, 3, 60], [0, 0, 60, 60]]


def _table(rng, nm, n):
    """a score per (m, id): small dyadic values (heavy ties), negative ones and +0.0"""
    return rng.integers(-6, 7, size=(nm, n)) / 4.0


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_hits_rule_equals_reference(layout):
    id_start = np.array(LAYOUTS[layout], dtype=np.uint64)
    n = int(id_start[-1])
    rng = np.random.default_rng(60 + layout)
    for nm, nt in ((1, 30), (5, 250), (3, 2000), (4, 0)):
        table = _table(rng, nm, n)
        m = rng.integers(0, nm, size=nt).astype(np.uint32)
        i = rng.integers(0, n, size=nt).astype(np.uint32)   # shuffled, and with repeats of one (m, id)
        got = capi.pssm_seq_hits(m, i, table[m, i], nm, id_start)
        present = np.zeros((nm, n), dtype=bool)
        present[m, i] = True
        dm, di = np.nonzero(present)
        want = ref.rows_from_hits(dm, di, table[dm, di], nm, id_start)
        ref.same_rows(got, want, (layout, nm, nt))
        assert int(got["count"].sum()) == len(dm) and np.all(got["lo"] <= got["hi"])
        if nt:
            assert len(dm) < nt or nt < 40      # repeats really occur
        # the owner of an id at equal neighbours is the LAST sequence starting at or below it: never an empty one
        assert np.all(id_start[got["seq"]] + got["hi"] < id_start[got["seq"].astype(np.int64) + 1])
        p = rng.permutation(nt)
        ref.same_rows(capi.pssm_seq_hits(m[p], i[p], table[m, i][p], nm, id_start), got, "permuted")
    assert (table == 0).any() and (table < 0).any()


def test_over_a_reference_scan():
    """The rows of pssm_ref.scan's hit list over a windows layout: the everything-hits profile has one row per
    sequence with windows, count = its windows, lo = 0, hi = windows - 1; ties go to the smaller id."""
    rng = np.random.default_rng(8)
    k, A, nm = 6, 20, 5
    wins = np.array([0, 3, 0, 70, 1, 0, 130, 0])
    id_start = np.concatenate([[0], np.cumsum(wins)]).astype(np.uint64)
    codes = rng.integers(0, A, size=(int(wins.sum()), k)).astype(np.uint8)
    S = rng.integers(-1, 2, size=(nm, k, A)) / 2.0     # scores are multiples of 1/2 within +-3: ties abound
    sc = pssm_ref.scores(S, codes)
    t = np.sort(sc, axis=1)[:, -40].copy()
    t[1] = -1e6
    t[2] = sc[2].max() + 1.0
    hits = pssm_ref.scan(S, t, codes)
    want = ref.rows(hits, nm, id_start)
    got = capi.pssm_seq_hits(hits["m"], hits["id"], hits["score"], nm, id_start)
    ref.same_rows(got, want, "scan")
    all_hit = got["m"] == 1
    assert got["seq"][all_hit].tolist() == [1, 3, 4, 6] and got["count"][all_hit].tolist() == [3, 70, 1, 130]
    assert np.all(got["lo"][all_hit] == 0) and got["hi"][all_hit].tolist() == [2, 69, 0, 129]
    assert not (got["m"] == 2).any() and want["seq_cnt"].tolist()[1:3] == [4, 0]
    # a best score attained twice in one row goes to the smaller id
    tied = 0
    for r in range(len(got["m"])):
        sel = (hits["m"] == got["m"][r]) & (hits["score"] == got["best_score"][r])
        sel &= (hits["id"] >= id_start[got["seq"][r]]) & (hits["id"] < id_start[got["seq"][r] + 1])
        tied += int(sel.sum() > 1)
        assert got["best_id"][r] == hits["id"][sel].min()
    assert tied >= 3


def test_capacity_protocol():
    id_start = np.array(LAYOUTS[0], dtype=np.uint64)
    rng = np.random.default_rng(5)
    table = _table(rng, 3, 60)
    m = rng.integers(0, 3, size=2000).astype(np.uint32)
    i = rng.integers(0, 60, size=2000).astype(np.uint32)
    rows = capi.pssm_seq_hits(m, i, table[m, i], 3, id_start)
    n_rows = len(rows["m"])
    assert n_rows == 3 * 5
    lib = capi.load()
    n_out = C.c_uint64(0)
    st = lib.hs_pssm_seq_hits(capi._vp(m), capi._vp(i), capi._vp(table[m, i]), 2000, 3, capi._vp(id_start), 12,
                              *[None] * 7, 0, C.byref(n_out))
    assert st == capi.HS_ERR_CAPACITY and n_out.value == n_rows
    out = [np.full(n_rows - 1, 9, dtype=t) for _, t in capi.PSSM_SEQ_FIELDS]
    with pytest.raises(HsError) as e:
        capi.pssm_seq_hits(m, i, table[m, i], 3, id_start, cap=n_rows - 1, out=out)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == n_rows
    assert all(np.all(a == 9) for a in out)
    out = [np.full(n_rows + 1, 9, dtype=t) for _, t in capi.PSSM_SEQ_FIELDS]
    ref.same_rows(capi.pssm_seq_hits(m, i, table[m, i], 3, id_start, cap=n_rows + 1, out=out), rows, "exact cap")
    assert all(a[n_rows] == 9 for a in out)


def test_refused_inputs_write_nothing():
    lib = capi.load()
    m = np.array([0, 0, 1], np.uint32)
    i = np.array([4, 4, 2], np.uint32)
    good = np.array([0, 3, 10], np.uint64)
    out = [np.full(4, 9, dtype=t) for _, t in capi.PSSM_SEQ_FIELDS]
    n_out = C.c_uint64(5)

    def call(ss, nm, id_start, n_seq=None, outs=out, n=n_out):
        ss = np.asarray(ss, np.float64)
        ids = None if id_start is None else np.asarray(id_start, np.uint64)
        n_seq = len(ids) - 1 if n_seq is None else n_seq
        return lib.hs_pssm_seq_hits(capi._vp(m), capi._vp(i), capi._vp(ss), 3, nm, None if ids is None else capi._vp(ids),
                                    n_seq, *[None if a is None else capi._vp(a) for a in outs], 4,
                                    None if n is None else C.byref(n))

    bad = capi.HS_ERR_INVALID
    assert call([1.0, 2.0, 0.5], 2, good) == bad and n_out.value == 0      # two scores for (0, 4)
    assert call([1.0, 1.0, np.nan], 2, good) == bad                        # a NaN
    assert call([1.0, 1.0, 0.5], 1, good) == bad                           # m >= nm
    assert call([1.0, 1.0, 0.5], 2, [0, 3, 4]) == bad                      # an id at id_start[n_seq]
    assert call([1.0, 1.0, 0.5], 2, [1, 3, 10]) == bad                     # does not start at 0
    assert call([1.0, 1.0, 0.5], 2, [0, 11, 10]) == bad                    # does not ascend
    assert call([1.0, 1.0, 0.5], 2, [0]) == bad                            # no sequence owns the ids
    assert call([1.0, 1.0, 0.5], 2, None, n_seq=2) == bad                  # a null id_start
    assert call([1.0, 1.0, 0.5], 2, good, outs=[None] + out[1:]) == bad    # a null output with cap > 0
    assert call([1.0, 1.0, 0.5], 2, good, n=None) == bad
    assert all(np.all(a == 9) for a in out)
    assert call([1.0, 1.0, -0.0], 2, good) == capi.HS_OK and n_out.value == 2
    assert out[0][:2].tolist() == [0, 1] and out[1][:2].tolist() == [1, 0] and out[2][:2].tolist() == [1, 1]
    assert out[4][:2].tolist() == [4, 2] and out[5][:2].tolist() == [1, 2] and not np.signbit(out[3][1])
    with pytest.raises(HsError):
        capi.pssm_seq_hits([0], [1], [np.nan], 1, [0, 2])
    assert len(capi.pssm_seq_hits([], [], [], 0, [0])["m"]) == 0


def test_exports_and_profile_field():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in ("hs_pssm_seq_scan", "hs_pssm_seq_scan_dev", "hs_pssm_seq_hits"):
        assert re.search(r"HS_API hs_status %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name)
    fields = [f for f, _ in capi._Profile._fields_]
    assert "pssm_seq_rows" in fields
    struct = header[header.index("typedef struct hs_profile"):header.index("} hs_profile;")]
    declared = re.findall(r"^\s*(?:double|uint64_t|uint32_t)\s+(\w+);", struct, flags=re.M)
    assert declared == fields
    assert "a per-sequence reduction of profile hits" not in header


def test_header_under_asan_and_ubsan(tmp_path):
    """hs_pssm_seq.h with a stand-alone main (tests/pssm_seq_san.cpp), compiled and run under AddressSanitizer +
    UndefinedBehaviorSanitizer (the runtimes linked statically); nothing is loaded into python."""
    exe = tmp_path / "pssm_seq_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "pssm_seq_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pssm_seq_san ok" in res.stdout
