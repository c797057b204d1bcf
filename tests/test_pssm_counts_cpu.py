"""hs_pssm_hit_counts / hs_pssm_refine without a GPU: the host rules (capi.pssm_count_hits, capi.pssm_log_odds_exact,
capi.pssm_background) against the numpy contract of tests/pssm_counts_ref.py -- shuffled and repeated tuples, both
modes over proteins of 0, fewer than k, exactly k and 300 residues, every refused input -- and the header under ASan +
UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hsearch_amd import HsError, capi

import pssm_counts_ref as ref
import pssm_ref
import pssm_seq_ref
import seqmatch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, A = 15, 20


def _windows(P, k=K):
    starts = P["db_start"].astype(np.int64)
    lens = np.diff(starts)
    pos = np.concatenate([np.arange(s, s + max(0, l - k + 1)) for s, l in zip(starts[:-1], lens)]).astype(np.int64)
    codes = np.ascontiguousarray(P["db"][pos[:, None] + np.arange(k)[None, :]], dtype=np.uint8)
    return codes, capi.window_id_start(P["db_start"], k)


@pytest.fixture(scope="module")
def case():
    P = seqmatch_ref.make_proteins(K)
    lens = np.diff(P["db_start"].astype(np.int64))
    assert (lens == 0).any() and ((lens > 0) & (lens < K)).any() and (lens == K).any() and (lens == 300).any()
    codes, id_start = _windows(P)
    rng = np.random.default_rng(77)
    nm = 6
    S = rng.integers(-4, 5, size=(nm, K, A)) / 2.0       # coarse: the best of a protein is often tied
    sc = pssm_ref.scores(S, codes)
    t = np.sort(sc, axis=1)[:, -len(codes) // 10].copy()
    t[1] = -1e6                                          # everything hits
    t[2] = sc[2].max() + 1.0                             # nothing does
    hits = pssm_ref.scan(S, t, codes)
    return dict(codes=codes, id_start=id_start, S=S, t=t, hits=hits, nm=nm)


@pytest.mark.parametrize("per_protein", [False, True])
def test_count_rule_equals_numpy(case, per_protein):
    ids = case["id_start"] if per_protein else None
    h, nm, codes = case["hits"], case["nm"], case["codes"]
    want = ref.from_hits(codes, A, h, nm, ids)
    got = capi.pssm_count_hits(codes, A, h["m"], h["id"], h["score"], nm, ids)
    ref.same_counts(got, want, per_protein)
    assert want["used"][2] == 0 and not got["counts"][2].any()
    n_with = int((np.diff(case["id_start"].astype(np.int64)) > 0).sum())
    assert want["used"][1] == (n_with if per_protein else len(codes))
    if per_protein:
        rows = pssm_seq_ref.rows(h, nm, ids)
        assert np.array_equal(got["used"], rows["seq_cnt"]) and (rows["count"] > 1).any()
    # shuffled, and with every tuple of the first half given twice
    rng = np.random.default_rng(3)
    m = np.concatenate([h["m"], h["m"][: len(h["m"]) // 2]])
    i = np.concatenate([h["id"], h["id"][: len(h["m"]) // 2]])
    s = np.concatenate([h["score"], h["score"][: len(h["m"]) // 2]])
    p = rng.permutation(len(m))
    ref.same_counts(capi.pssm_count_hits(codes, A, m[p], i[p], s[p], nm, ids), want, "shuffled, repeated")
    # a repeat with another score is refused
    s2 = s.copy()
    s2[-1] += 0.5
    with pytest.raises(HsError) as e:
        capi.pssm_count_hits(codes, A, m, i, s2, nm, ids)
    assert e.value.status == capi.HS_ERR_INVALID
    # no tuples
    empty = capi.pssm_count_hits(codes, A, [], [], [], 3, ids)
    assert not empty["counts"].any() and not empty["used"].any() and empty["counts"].shape == (3, K, A)


@pytest.mark.parametrize("k,alphabet", [(1, 20), (25, 20), (4, 32), (75, 32)])
def test_shapes(k, alphabet):
    rng = np.random.default_rng(k * alphabet)
    n, nm = 301, 3
    codes = rng.integers(0, alphabet, size=(n, k)).astype(np.uint8)
    id_start = np.array([0, 0, 5, 5, 100, 300, 301, 301], np.uint64)
    nt = 900
    m = rng.integers(0, nm, size=nt).astype(np.uint32)
    i = rng.integers(0, n, size=nt).astype(np.uint32)
    table = rng.integers(-3, 4, size=(nm, n)) / 2.0
    present = np.zeros((nm, n), dtype=bool)
    present[m, i] = True
    dm, di = np.nonzero(present)
    hits = dict(m=dm.astype(np.uint32), id=di.astype(np.uint32), score=table[dm, di])
    for ids in (None, id_start):
        ref.same_counts(capi.pssm_count_hits(codes, alphabet, m, i, table[m, i], nm, ids),
                        ref.from_hits(codes, alphabet, hits, nm, ids), (k, alphabet, ids is None))


def test_log_odds_and_background(case):
    got = capi.pssm_count_hits(case["codes"], A, case["hits"]["m"], case["hits"]["id"], case["hits"]["score"],
                               case["nm"])
    bg = ref.background(case["codes"], A)
    comp = np.bincount(case["codes"].ravel(), minlength=A)
    assert np.array_equal(bg, comp / comp.sum()) and abs(bg.sum() - 1) < 1e-12
    assert np.array_equal(bg, capi.pssm_background(got["counts"][1]))      # the profile that hits everything
    for pseudo in (1.0, 0.25, 20.0):
        S = capi.pssm_log_odds_exact(got["counts"], bg, pseudo)
        assert np.isfinite(S).all() and np.abs(S).max() < 2.0 ** 100
        np.testing.assert_allclose(S, ref.log_odds_numpy(got["counts"], bg, pseudo), rtol=1e-12, atol=1e-12)
        assert np.array_equal(S.view(np.uint64), capi.pssm_log_odds_exact(got["counts"], bg, pseudo).view(np.uint64))
        # a profile without sites: log2(pseudo * bg / pseudo / bg), zero up to the roundings
        assert np.abs(S[2]).max() < 1e-15
    # a residue that never occurs takes the smallest positive frequency, without renormalising
    row = np.zeros((3, 5), np.uint32)
    row[:, 0], row[:, 3], row[0, 4] = 6, 3, 1
    assert capi.pssm_background(row).tolist() == [18 / 28, 1 / 28, 1 / 28, 9 / 28, 1 / 28]
    with pytest.raises(HsError):
        capi.pssm_background(np.zeros((3, 5), np.uint32))


def test_refused_inputs_write_nothing():
    lib = capi.load()
    k, alphabet, n = 3, 20, 10
    codes = np.ones((n, k), np.uint8)
    m = np.array([0, 0, 1], np.uint32)
    i = np.array([4, 4, 2], np.uint32)
    good = np.array([0, 3, 10], np.uint64)
    counts = np.full((2, k, alphabet), 9, np.uint32)
    used = np.full(2, 9, np.uint64)
    bad = capi.HS_ERR_INVALID

    def call(ss, nm=2, ids=None, cds=codes, c=counts, kk=k, AA=alphabet, nn=n):
        ss = np.asarray(ss, np.float64)
        ids = None if ids is None else np.asarray(ids, np.uint64)
        return lib.hs_pssm_count_hits(capi._vp(cds), nn, kk, AA, capi._vp(m), capi._vp(i), capi._vp(ss), 3, nm,
                                      None if ids is None else capi._vp(ids), 0 if ids is None else len(ids) - 1,
                                      None if c is None else capi._vp(c), capi._vp(used))

    for ids in (None, good):
        assert call([1.0, 2.0, 0.5], ids=ids) == bad                       # two scores for (0, 4)
        assert call([1.0, 1.0, np.nan], ids=ids) == bad
        assert call([1.0, 1.0, 0.5], nm=1, ids=ids) == bad                 # m >= nm
        assert call([1.0, 1.0, 0.5], ids=ids, nn=4) == bad                 # an id at n
        assert call([1.0, 1.0, 0.5], ids=ids, c=None) == bad
        assert call([1.0, 1.0, 0.5], ids=ids, kk=0) == bad
        assert call([1.0, 1.0, 0.5], ids=ids, AA=33) == bad
        big = codes.copy()
        big[4, 1] = alphabet
        assert call([1.0, 1.0, 0.5], ids=ids, cds=big) == bad              # a counted code at the alphabet's size
    assert call([1.0, 1.0, 0.5], ids=[0, 3, 9]) == bad                     # does not end at n
    assert call([1.0, 1.0, 0.5], ids=[1, 3, 10]) == bad
    assert call([1.0, 1.0, 0.5], ids=[0, 11, 10]) == bad
    assert np.all(counts == 9) and np.all(used == 9)
    assert call([1.0, 1.0, -0.0], ids=good) == capi.HS_OK
    assert used.tolist() == [1, 1] and counts[:, :, 1].tolist() == [[1] * k] * 2 and counts.sum() == 2 * k
    # the log-odds
    S = np.full((2, k, alphabet), 9.0)
    bg = np.full(alphabet, 0.05)

    def lo(b=bg, pseudo=1.0, out=S):
        return lib.hs_pssm_log_odds(capi._vp(counts), 2, k, alphabet, None if b is None else capi._vp(b), pseudo,
                                    None if out is None else capi._vp(out))

    for pseudo in (0.0, -1.0, np.inf, np.nan):
        assert lo(pseudo=pseudo) == bad
    for v in (0.0, -0.5, np.inf, np.nan):
        b = bg.copy()
        b[7] = v
        assert lo(b=b) == bad
    assert lo(b=None) == bad and lo(out=None) == bad
    assert np.all(S == 9.0)
    assert lo() == capi.HS_OK and np.isfinite(S).all()


def test_exports_option_and_profile_fields():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in ("hs_pssm_hit_counts", "hs_pssm_hit_counts_dev", "hs_pssm_refine", "hs_pssm_count_hits",
                 "hs_pssm_log_odds", "hs_pssm_background"):
        assert re.search(r"HS_API hs_status %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name)
    assert capi.Engine.OPTIONS["pssm_count_chunk"] == 25 and "HS_OPT_PSSM_COUNT_CHUNK = 25" in header
    fields = [f for f, _ in capi._Profile._fields_]
    assert "pssm_count_sites" in fields and "pssm_count_items" in fields
    struct = header[header.index("typedef struct hs_profile"):header.index("} hs_profile;")]
    declared = re.findall(r"^\s*(?:double|uint64_t|uint32_t)\s+(\w+);", struct, flags=re.M)
    assert declared == fields


def test_header_under_asan_and_ubsan(tmp_path):
    """hs_pssm_counts.h with a stand-alone main (tests/pssm_counts_san.cpp), compiled and run under AddressSanitizer +
    UndefinedBehaviorSanitizer (the runtimes linked statically); nothing is loaded into python."""
    exe = tmp_path / "pssm_counts_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "pssm_counts_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pssm_counts_san ok" in res.stdout
