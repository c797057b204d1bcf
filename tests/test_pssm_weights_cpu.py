"""hs_pssm_weighted_counts / hs_pssm_refine_weighted without a GPU: the host rules (capi.pssm_weight_hits,
capi.pssm_log_odds_weighted, capi.pssm_weight_u) against the Python-integer contract of tests/pssm_weights_ref.py -- a
hand example in literals, shuffled and repeated tuples in both modes over proteins of 0, fewer than k, exactly k and
300 residues, the column sums and the bound on wsum, u at its extremes, every refused input, a planted redundant
family -- and the header under ASan + UBSan."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from hsearch_amd import HsError, capi

import pssm_counts_ref
import pssm_ref
import pssm_weights_ref as ref
import seqmatch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, A = 15, 20
ONE = 1 << 56


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
    rng = np.random.default_rng(78)
    nm = 6
    S = rng.integers(-4, 5, size=(nm, K, A)) / 2.0       # coarse: the best of a protein is often tied
    S[3] = 0.0
    S[3, 0, :] = -8.0
    S[3, 0, 5] = 8.0                                     # profile 3 hits the windows that start with residue 5
    sc = pssm_ref.scores(S, codes)
    t = np.sort(sc, axis=1)[:, -len(codes) // 10].copy()
    t[1] = -1e6                                          # everything hits
    t[2] = sc[2].max() + 1.0                             # nothing does
    t[3] = 0.0
    hits = pssm_ref.scan(S, t, codes)
    return dict(codes=codes, id_start=id_start, S=S, t=t, hits=hits, nm=nm)


def test_hand_example():
    """k = 2, alphabet 4, sites AA, AC, CC -- every number written out"""
    codes = np.array([[0, 0], [0, 1], [1, 1], [3, 3]], np.uint8)
    got = capi.pssm_weight_hits(codes, 4, [0, 0, 0], [0, 1, 2], [1.0, 1.0, 1.0], 1)
    assert got["counts"].tolist() == [[[2, 1, 0, 0], [1, 2, 0, 0]]]
    # u[0][A] = 2^56 / (2 * 2), u[0][C] = 2^56 / (2 * 1), u[1][A] = 2^55, u[1][C] = 2^54; W = 3 * 2^54, 2^55, 3 * 2^54
    assert got["wcounts"].tolist() == [[[5 << 54, 3 << 54, 0, 0], [3 << 54, 5 << 54, 0, 0]]]
    assert got["wsum"].tolist() == [1 << 57] and got["distinct"].tolist() == [4] and got["used"].tolist() == [3]
    assert got["wcounts"].dtype == np.uint64 and got["wsum"].dtype == np.uint64 and got["distinct"].dtype == np.uint32
    want = ref.weigh(codes, 4, [0, 0, 0], [0, 1, 2], 1)
    assert want["weights"] == [3 << 54, 1 << 55, 3 << 54]
    ref.same_weights(got, want, "hand")


def test_u_at_its_extremes():
    assert capi.pssm_weight_u(1, 1) == ONE
    assert capi.pssm_weight_u(32, 2 ** 32 - 1) == ONE // (32 * (2 ** 32 - 1)) == 524288
    assert capi.pssm_weight_u(20, 0) == 0 and capi.pssm_weight_u(0, 7) == 0
    for r, c in ((2, 2), (3, 7), (20, 4001), (32, 1), (1, 2 ** 32 - 1), (19, 65537)):
        assert capi.pssm_weight_u(r, c) == ref.u(r, c) == ONE // (r * c)
        assert c * capi.pssm_weight_u(r, c) * r <= ONE               # what keeps wsum <= k 2^56


def test_the_construction_is_a_test(case):
    every = ref.from_hits(case["codes"], A, case["hits"], case["nm"])
    one = ref.from_hits(case["codes"], A, case["hits"], case["nm"], case["id_start"])
    for want in (every, one):
        c = want["counts"]
        assert want["used"][2] == 0 and not want["wcounts"][2].any() and want["wsum"][2] == 0        # a dead profile
        assert want["distinct"][2] == 0
        assert (c[3, 0] > 0).sum() == 1 and want["used"][3] > 1                   # a column of one residue
        assert want["distinct"][3] < want["distinct"][1] <= K * A
    assert (every["counts"][1] > 0).all() and every["distinct"][1] == K * A   # columns of all residues
    by_m = {}
    sm, _ = ref.sites(case["hits"], case["nm"])
    for m, w in zip(sm.tolist(), every["weights"]):
        by_m.setdefault(m, set()).add(w)
    assert len(by_m[1]) > 10 and len(by_m[0]) > 1                                 # sites that do not weigh the same
    assert not np.array_equal(every["wcounts"], one["wcounts"])
    # ... and the library's rule sees the same fixture: the same columns, the dead profile, the unequal sites
    h = case["hits"]
    for want, ids in ((every, None), (one, case["id_start"])):
        got = capi.pssm_weight_hits(case["codes"], A, h["m"], h["id"], h["score"], case["nm"], ids)
        assert not got["wcounts"][2].any() and got["wsum"][2] == 0 and got["distinct"][2] == 0
        assert (got["wcounts"][3, 0] > 0).sum() == 1 and got["wcounts"][3, 0, 5] == got["wsum"][3] > 0
        assert np.array_equal(got["distinct"], want["distinct"])
    assert (got["counts"][1] > 0).sum() < K * A
    got = capi.pssm_weight_hits(case["codes"], A, h["m"], h["id"], h["score"], case["nm"])
    assert (got["wcounts"][1] > 0).all() and got["distinct"][1] == K * A
    per_site = got["wcounts"][1].astype(object) / got["counts"][1].astype(object)  # equal weights would make it constant
    assert len(set(per_site[0].tolist())) > 10


@pytest.mark.parametrize("per_protein", [False, True])
def test_weight_rule_equals_the_reference(case, per_protein):
    ids = case["id_start"] if per_protein else None
    h, nm, codes = case["hits"], case["nm"], case["codes"]
    want = ref.from_hits(codes, A, h, nm, ids)
    got = capi.pssm_weight_hits(codes, A, h["m"], h["id"], h["score"], nm, ids)
    ref.same_weights(got, want, per_protein)
    raw = capi.pssm_count_hits(codes, A, h["m"], h["id"], h["score"], nm, ids)
    assert np.array_equal(raw["counts"], got["counts"]) and np.array_equal(raw["used"], got["used"])
    # shuffled, and with every tuple of the first half given twice
    rng = np.random.default_rng(3)
    m = np.concatenate([h["m"], h["m"][: len(h["m"]) // 2]])
    i = np.concatenate([h["id"], h["id"][: len(h["m"]) // 2]])
    s = np.concatenate([h["score"], h["score"][: len(h["m"]) // 2]])
    p = rng.permutation(len(m))
    ref.same_weights(capi.pssm_weight_hits(codes, A, m[p], i[p], s[p], nm, ids), want, "shuffled, repeated")
    s2 = s.copy()
    s2[-1] += 0.5
    with pytest.raises(HsError) as e:
        capi.pssm_weight_hits(codes, A, m, i, s2, nm, ids)
    assert e.value.status == capi.HS_ERR_INVALID
    empty = capi.pssm_weight_hits(codes, A, [], [], [], 3, ids)
    assert not empty["wcounts"].any() and not empty["wsum"].any() and not empty["distinct"].any()
    assert empty["wcounts"].shape == (3, K, A)


@pytest.mark.parametrize("k,alphabet", [(1, 20), (25, 20), (4, 32), (75, 32)])
def test_shapes(k, alphabet):
    rng = np.random.default_rng(k * alphabet + 1)
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
        ref.same_weights(capi.pssm_weight_hits(codes, alphabet, m, i, table[m, i], nm, ids),
                         ref.from_hits(codes, alphabet, hits, nm, ids), (k, alphabet, ids is None))


def test_log_odds_weighted(case):
    got = capi.pssm_weight_hits(case["codes"], A, case["hits"]["m"], case["hits"]["id"], case["hits"]["score"],
                                case["nm"])
    bg = pssm_counts_ref.background(case["codes"], A)
    for pseudo, neff in ((1.0, "sites"), (0.25, "columns"), (20.0, "sites")):
        ne = ref.n_eff(got, K, neff)
        S = capi.pssm_log_odds_weighted(got["wcounts"], got["wsum"], ne, bg, pseudo)
        assert np.isfinite(S).all() and np.abs(S).max() < 2.0 ** 100
        np.testing.assert_allclose(S, ref.log_odds_numpy(got["wcounts"], got["wsum"], ne, bg, pseudo), rtol=1e-12,
                                   atol=1e-12)
        again = capi.pssm_log_odds_weighted(got["wcounts"], got["wsum"], ne, bg, pseudo)
        assert np.array_equal(S.view(np.uint64), again.view(np.uint64))
        # bit for bit, every entry: the expression one entry at a time in Python floats (IEEE doubles, no contraction)
        exact = ref.log_odds_exact(got["wcounts"], got["wsum"], ne, bg, pseudo)
        assert np.array_equal(S.view(np.uint64), exact.view(np.uint64))
        assert np.abs(S[2]).max() < 1e-15          # a profile without sites: log2(pseudo * bg / pseudo / bg)
    # equal weights give the raw frequencies: with one site per profile wc / wsum is c / used exactly
    one = capi.pssm_weight_hits(case["codes"], A, [0], [5], [1.0], 1)
    assert np.array_equal(capi.pssm_log_odds_weighted(one["wcounts"], one["wsum"], [1.0], bg, 1.0).view(np.uint64),
                          capi.pssm_log_odds_exact(one["counts"], bg, 1.0).view(np.uint64))


def test_refused_inputs_write_nothing():
    lib = capi.load()
    k, alphabet, n = 3, 20, 10
    codes = np.ones((n, k), np.uint8)
    m = np.array([0, 0, 1], np.uint32)
    i = np.array([4, 4, 2], np.uint32)
    good = np.array([0, 3, 10], np.uint64)
    counts = np.full((2, k, alphabet), 9, np.uint32)
    wcounts = np.full((2, k, alphabet), 9, np.uint64)
    wsum, used, distinct = np.full(2, 9, np.uint64), np.full(2, 9, np.uint64), np.full(2, 9, np.uint32)
    bad = capi.HS_ERR_INVALID

    def call(ss, nm=2, ids=None, cds=codes, w=wcounts, kk=k, AA=alphabet, nn=n):
        ss = np.asarray(ss, np.float64)
        ids = None if ids is None else np.asarray(ids, np.uint64)
        return lib.hs_pssm_weight_hits(capi._vp(cds), nn, kk, AA, capi._vp(m), capi._vp(i), capi._vp(ss), 3, nm,
                                       None if ids is None else capi._vp(ids), 0 if ids is None else len(ids) - 1,
                                       capi._vp(counts), None if w is None else capi._vp(w), capi._vp(wsum),
                                       capi._vp(distinct), capi._vp(used))

    for ids in (None, good):
        assert call([1.0, 2.0, 0.5], ids=ids) == bad                       # two scores for (0, 4)
        assert call([1.0, 1.0, np.nan], ids=ids) == bad
        assert call([1.0, 1.0, 0.5], nm=1, ids=ids) == bad                 # m >= nm
        assert call([1.0, 1.0, 0.5], ids=ids, nn=4) == bad                 # an id at n
        assert call([1.0, 1.0, 0.5], ids=ids, w=None) == bad
        assert call([1.0, 1.0, 0.5], ids=ids, kk=0) == bad
        assert call([1.0, 1.0, 0.5], ids=ids, kk=128) == bad
        assert call([1.0, 1.0, 0.5], ids=ids, AA=33) == bad
        big = codes.copy()
        big[4, 1] = alphabet
        assert call([1.0, 1.0, 0.5], ids=ids, cds=big) == bad              # a counted code at the alphabet's size
    assert call([1.0, 1.0, 0.5], ids=[0, 3, 9]) == bad                     # does not end at n
    assert call([1.0, 1.0, 0.5], ids=[1, 3, 10]) == bad
    assert call([1.0, 1.0, 0.5], ids=[0, 11, 10]) == bad
    for arr in (counts, wcounts, wsum, used, distinct):
        assert np.all(arr == 9)
    assert call([1.0, 1.0, -0.0], ids=good) == capi.HS_OK
    assert used.tolist() == [1, 1] and counts.sum() == 2 * k and distinct.tolist() == [k, k]
    assert wsum.tolist() == [k * ONE] * 2 and wcounts[:, :, 1].tolist() == [[k * ONE] * k] * 2
    # the weighted log-odds
    S = np.full((2, k, alphabet), 9.0)
    bg = np.full(alphabet, 0.05)
    ne = np.array([1.0, 1.0])

    def lo(b=bg, pseudo=1.0, out=S, n_eff=ne, wc=wcounts, ws=wsum):
        return lib.hs_pssm_log_odds_weighted(None if wc is None else capi._vp(wc), None if ws is None else capi._vp(ws),
                                             None if n_eff is None else capi._vp(np.asarray(n_eff, np.float64)), 2, k,
                                             alphabet, None if b is None else capi._vp(b), pseudo,
                                             None if out is None else capi._vp(out))

    for pseudo in (0.0, -1.0, np.inf, np.nan):
        assert lo(pseudo=pseudo) == bad
    for v in (0.0, -0.5, np.inf, np.nan):
        b = bg.copy()
        b[7] = v
        assert lo(b=b) == bad
    for v in (-1.0, -5e-324, np.inf, np.nan):
        assert lo(n_eff=[1.0, v]) == bad
    over = wcounts.copy()
    over[1, 2, 19] = wsum[1] + 1
    assert lo(wc=over) == bad                                              # an entry above its wsum
    assert lo(b=None) == bad and lo(out=None) == bad and lo(n_eff=None) == bad and lo(wc=None) == bad
    assert lo(ws=None) == bad
    assert np.all(S == 9.0)
    assert lo() == capi.HS_OK and np.isfinite(S).all()
    assert lo(n_eff=[0.0, 0.0]) == capi.HS_OK and np.abs(S).max() < 1e-15


def _planted(seed):
    """5000 25-mers over 20 residues: one k-mer X copied 4000 times, 12 members of a second family (a motif M with 6 of
    its 25 positions redrawn in every member, none copied) and random k-mers.  X is itself such a member: a search
    started at M finds the copies with the family."""
    rng = np.random.default_rng(seed)
    k = 25
    M = rng.integers(0, A, size=k).astype(np.uint8)

    def member():
        x = M.copy()
        at = rng.choice(k, size=6, replace=False)
        x[at] = (x[at] + rng.integers(1, A, size=6)) % A          # 6 positions that differ from M
        return x

    X = member()
    fam = np.array([member() for _ in range(12)], np.uint8)
    noise = rng.integers(0, A, size=(1000 - 12, k)).astype(np.uint8)
    codes = np.concatenate([np.tile(X, (4000, 1)), fam, noise]).astype(np.uint8)
    S0 = np.full((1, k, A), -1.0)
    S0[0, np.arange(k), M] = 2.0                                    # a member scores 19 * 2 - 6 = 32
    return dict(codes=codes, X=X, M=M, fam_ids=np.arange(4000, 4012), S0=S0, k=k)


PLANTED_SEED = 1


def test_planted_redundancy():
    P = _planted(PLANTED_SEED)
    codes, k = P["codes"], P["k"]
    n = len(codes)
    # every k-mer a site: the copied residue's exact weighted share lies below its raw share in every column
    rng = np.random.default_rng(5)
    flat = np.concatenate([np.tile(P["X"], (4000, 1)), rng.integers(0, A, size=(1000, k)).astype(np.uint8)])
    hits = dict(m=np.zeros(n, np.uint32), id=np.arange(n, dtype=np.uint32), score=np.zeros(n))
    want = ref.from_hits(flat, A, hits, 1)
    got = capi.pssm_weight_hits(flat, A, hits["m"], hits["id"], hits["score"], 1)
    ref.same_weights(got, want, "planted")
    for res in (want, got):
        ws = int(res["wsum"][0])
        assert ws <= k * ONE and Fraction(ws, k * ONE) > Fraction(999999, 1000000)
        for p in range(k):
            raw = Fraction(int(res["counts"][0, p, P["X"][p]]), n)
            weighted = Fraction(int(res["wcounts"][0, p, P["X"][p]]), ws)
            assert raw > Fraction(4, 5) and weighted < Fraction(1, 5) and weighted < raw, (p, raw, weighted)
    # the loop from a start at the family's motif at the fixed threshold 32 (a member scores 19 * 2 - 6 against the
    # start): weights keep the family's members, raw counts converge onto the copies and lose them -- shown on the
    # reference first.  (Every seed tried, 1 .. 3, shows it; under raw counts the members fall to about -50.)
    fam = P["fam_ids"]
    t = np.array([32.0])

    def members(res):
        return int((pssm_ref.scores(res["S"], codes)[0][fam] >= t[0]).sum())

    first = set(pssm_ref.scan(P["S0"], t, codes)["id"].tolist())
    assert set(fam.tolist()) <= first and set(range(4000)) <= first and len(first) == 4012
    plain = ref.refine(codes, A, P["S0"], 4, t=t, weighted=False)
    assert plain["converged"] and members(plain) < len(fam) and plain["used"][0] >= 4000
    for neff in ("sites", "columns"):
        weighted = ref.refine(codes, A, P["S0"], 4, t=t, neff=neff)
        assert weighted["converged"] and members(weighted) == len(fam) and weighted["used"][0] == 4012
        # ... and the library's host rules walk the reference's trajectory, scan for scan
        S = P["S0"]
        bg = pssm_counts_ref.background(codes, A)
        for i, (c, wc) in enumerate(weighted["history"]):
            h = pssm_ref.scan(S, t, codes)
            got = capi.pssm_weight_hits(codes, A, h["m"], h["id"], h["score"], 1)
            assert np.array_equal(got["counts"], c) and np.array_equal(got["wcounts"], wc), (neff, i)
            if i + 1 < len(weighted["history"]):
                S = capi.pssm_log_odds_weighted(got["wcounts"], got["wsum"], ref.n_eff(got, k, neff), bg, 1.0)
        assert np.array_equal(S.view(np.uint64), weighted["S"].view(np.uint64)), neff
        assert (pssm_ref.scores(S, codes)[0][fam] >= t[0]).all()


def test_exports_and_profile_fields():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in ("hs_pssm_weighted_counts", "hs_pssm_weighted_counts_dev", "hs_pssm_refine_weighted",
                 "hs_pssm_weight_hits", "hs_pssm_log_odds_weighted"):
        assert re.search(r"HS_API hs_status %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name)
    assert "HS_API uint64_t hs_pssm_weight_u(" in header and "hs_pssm_weight_u" in capi.EXPORTS
    fields = [f for f, _ in capi._Profile._fields_]
    at = fields.index("pssm_count_items")
    assert fields[at + 1:at + 3] == ["pssm_weight_sites", "pssm_weight_items"]
    struct = header[header.index("typedef struct hs_profile"):header.index("} hs_profile;")]
    declared = re.findall(r"^\s*(?:double|uint64_t|uint32_t)\s+(\w+);", struct, flags=re.M)
    assert declared == fields
    for name in ("pssm_weighted_counts", "pssm_weighted_counts_dev", "pssm_refine_weighted"):
        assert callable(getattr(capi.Engine, name))


def test_header_under_asan_and_ubsan(tmp_path):
    """hs_pssm_weights.h with a stand-alone main (tests/pssm_weights_san.cpp), compiled and run under AddressSanitizer
    + UndefinedBehaviorSanitizer (the runtimes linked statically); nothing is loaded into python."""
    exe = tmp_path / "pssm_weights_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "pssm_weights_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pssm_weights_san ok" in res.stdout
