"""hs_cluster_weighted_profile / hs_cluster_pssm_cover without a GPU: the host rules (capi.cluster_weights_codes,
capi.cluster_cover_codes) against tests/cluster_pssm_ref.py bit for bit -- every shape, noise, clusters below min_size,
one cluster of everything, n clusters of one member, the (row, member) tuples through hs_pssm_weight_hits, the column
sums, a planted redundant family, planted ties of the minimum, extreme profiles, every refusal on sentinel-filled
outputs -- and the header under ASan + UBSan in a stand-alone program."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from hsearch_amd import HsError, capi

import cluster_pssm_ref as ref
import pssm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 20), (25, 20), (26, 20), (4, 32), (75, 32)]
NOISE = capi.NOISE
ONE = 1 << 56


def _labels(rng, n):
    """label sets over n k-mers: mixed with noise and small clusters, one cluster of everything, n singletons"""
    mixed = rng.integers(0, max(1, n // 7), size=n).astype(np.uint32)
    mixed = (mixed * 3 + 1) % n                     # label values that are not the smallest member id
    mixed[rng.random(n) < 0.2] = NOISE
    mixed[:3] = n - 1                               # a cluster of exactly three
    return dict(mixed=mixed, one=np.full(n, n // 2, np.uint32), singles=rng.permutation(n).astype(np.uint32),
                noise=np.full(n, NOISE, np.uint32))


def _profiles(rng, rows, k, A):
    return rng.integers(-6, 7, size=(rows, k, A)) / 2.0      # coarse: the minimum of a row is often tied


@pytest.mark.parametrize("k,alphabet", SHAPES)
def test_host_rules_equal_the_reference(k, alphabet):
    rng = np.random.default_rng(100 * k + alphabet)
    n = 211
    codes = rng.integers(0, alphabet, size=(n, k)).astype(np.uint8)
    codes[rng.random(n) < 0.3] = codes[0]                     # repeats: columns of few residues, unequal weights
    for name, label in _labels(rng, n).items():
        for min_size in (1, 3, 4):
            want = ref.weighted_profile(codes, alphabet, label, min_size)
            got = capi.cluster_weights_codes(codes, alphabet, label, min_size, want_counts=True)
            ref.assert_same(got, want, (name, min_size))
            rows = len(want["label"])
            assert rows == {"one": 1, "noise": 0}.get(name, rows) and (name != "singles" or rows == (n if min_size == 1 else 0))
            assert all(int(s) <= k * ONE for s in got["wsum"].tolist())
            bare = capi.cluster_weights_codes(codes, alphabet, label, min_size)
            assert "counts" not in bare and np.array_equal(bare["wcounts"], got["wcounts"])
            # the same thing as hs_pssm_weight_hits over the (row, member) tuples, shuffled
            _, _, sm, si = ref.members(label, min_size)
            p = rng.permutation(len(sm))
            hits = capi.pssm_weight_hits(codes, alphabet, sm[p], si[p], np.zeros(len(sm)), rows)
            for f in ("counts", "wcounts", "wsum", "distinct"):
                assert np.array_equal(hits[f], got[f]), (name, min_size, f)
            assert np.array_equal(hits["used"], got["size"].astype(np.uint64))
            S = _profiles(rng, rows, k, alphabet)
            ref.assert_same(capi.cluster_cover_codes(codes, alphabet, label, S, min_size),
                            ref.cover(codes, label, min_size, S), (name, min_size, "cover"))


def test_capacity_follows_the_two_call_pattern():
    rng = np.random.default_rng(2)
    codes = rng.integers(0, 20, size=(50, 5)).astype(np.uint8)
    label = (np.arange(50) % 7).astype(np.uint32)
    with pytest.raises(HsError) as e:
        capi.cluster_weights_codes(codes, 20, label, cap=3)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == 7
    assert len(capi.cluster_weights_codes(codes, 20, label, cap=7)["label"]) == 7


def test_planted_redundancy():
    """500 members of one cluster, 400 of them copies of one k-mer: the copied residue owns the raw profile and not the
    weighted one"""
    rng = np.random.default_rng(9)
    k, A = 25, 20
    X = rng.integers(0, A, size=k).astype(np.uint8)
    codes = np.concatenate([np.tile(X, (400, 1)), rng.integers(0, A, size=(100, k)).astype(np.uint8),
                            rng.integers(0, A, size=(60, k)).astype(np.uint8)])
    label = np.concatenate([np.full(500, 7, np.uint32), np.full(60, NOISE, np.uint32)])
    want = ref.weighted_profile(codes, A, label, 1)
    got = capi.cluster_weights_codes(codes, A, label, 1, want_counts=True)
    ref.assert_same(got, want, "planted")
    assert got["size"].tolist() == [500]
    ws = int(got["wsum"][0])
    for p in range(k):
        raw = Fraction(int(got["counts"][0, p, X[p]]), 500)
        weighted = Fraction(int(got["wcounts"][0, p, X[p]]), ws)
        assert raw > Fraction(4, 5) and weighted < Fraction(1, 5), (p, raw, weighted)


def test_cover_minimum_is_attained_and_ties_take_the_smallest_id():
    rng = np.random.default_rng(4)
    k, A, n = 6, 20, 300
    codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
    label = (np.arange(n) % 3).astype(np.uint32)
    S = rng.normal(size=(3, k, A))
    # plant the worst k-mer of every profile at several members of its row: ids 201 + r, 99 + r, 249 + r (given in
    # this order; the smallest must win)
    worst = S.argmin(axis=2).astype(np.uint8)
    for r in range(3):
        for i in (201 + r, 99 + r, 249 + r):
            assert label[i] == r
            codes[i] = worst[r]
    got = capi.cluster_cover_codes(codes, A, label, S)
    ref.assert_same(got, ref.cover(codes, label, 1, S), "ties")
    assert got["argmin"].tolist() == [99, 100, 101]
    sc = pssm_ref.scores(S, codes)
    for r in range(3):
        mine = sc[r][label == r]
        assert got["min_score"][r] == mine.min() == sc[r, got["argmin"][r]] and (mine == mine.min()).sum() == 3
        # the contract: a scan at t = min_score returns every member of the row under its profile
        assert (mine >= got["min_score"][r]).all()


def test_cover_extreme_profiles_match_the_left_to_right_sum():
    """a forbidden residue at -10^30 and entries at +-2^100: sums that cancel, absorb and are all negative"""
    rng = np.random.default_rng(6)
    k, A, n = 26, 20, 120
    codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
    label = (np.arange(n) % 2).astype(np.uint32)
    S = rng.normal(size=(2, k, A))
    S[0, :, 3] = -1e30
    S[1, 0, :] = 2.0 ** 100
    S[1, 1, :] = -2.0 ** 100
    S[1, 2, ::2] = 2.0 ** 100
    S[1, 5, 1::2] = -2.0 ** 100
    got = capi.cluster_cover_codes(codes, A, label, S)
    want = ref.cover(codes, label, 1, S)
    ref.assert_same(got, want, "extreme")
    for r in range(2):                                            # ... one k-mer at a time in Python floats
        x = codes[got["argmin"][r]]
        s = 0.0
        for p in range(k):
            s = s + float(S[r, p, x[p]])
        assert np.float64(s).view(np.uint64) == got["min_score"][r:r + 1].view(np.uint64)[0]
    assert got["min_score"][0] < -1e29 and (got["min_score"] < 0).all()


def test_refused_inputs_write_nothing():
    lib = capi.load()
    k, A, n = 3, 20, 10
    codes = np.ones((n, k), np.uint8)
    label = np.array([0, 0, 0, 5, 5, NOISE, 5, 0, 9, 9], np.uint32)       # rows at min_size 2: 0 (4), 5 (3), 9 (2)
    ol, osz, di = np.full(4, 9, np.uint32), np.full(4, 9, np.uint32), np.full(4, 9, np.uint32)
    cnt, wc, ws = np.full((4, k, A), 9, np.uint32), np.full((4, k, A), 9, np.uint64), np.full(4, 9, np.uint64)
    n_out = capi.C.c_uint64(77)
    bad = capi.HS_ERR_INVALID
    vp = capi._vp

    def weights(cds=codes, nn=n, kk=k, AA=A, lab=label, ms=2, w=wc, cap=4, out=ol):
        return lib.hs_cluster_weights_codes(None if cds is None else vp(cds), nn, kk, AA, None if lab is None else vp(lab),
                                            ms, None if out is None else vp(out), vp(osz), vp(cnt),
                                            None if w is None else vp(w), vp(ws), vp(di), cap, capi.C.byref(n_out))

    big = codes.copy()
    big[5, 1] = A                                   # a code at the alphabet's size, in a NOISE k-mer: refused all the same
    wrong = label.copy()
    wrong[2] = n                                    # a label at n
    for kw in (dict(ms=0), dict(kk=0), dict(kk=76), dict(AA=0), dict(AA=33), dict(cds=big), dict(lab=wrong),
               dict(w=None), dict(out=None), dict(cds=None), dict(lab=None), dict(nn=1 << 31)):
        assert weights(**kw) == bad, kw
        assert n_out.value == 0
    assert weights(cap=2) == capi.HS_ERR_CAPACITY and n_out.value == 3
    assert lib.hs_cluster_weights_codes(vp(codes), n, k, A, vp(label), 2, None, None, None, None, None, None, 0,
                                        capi.C.byref(n_out)) == capi.HS_ERR_CAPACITY and n_out.value == 3
    assert lib.hs_cluster_weights_codes(vp(codes), n, k, A, vp(label), 2, vp(ol), vp(osz), vp(cnt), vp(wc), vp(ws),
                                        vp(di), 4, None) == bad
    for arr in (ol, osz, di, cnt, wc, ws):
        assert np.all(arr == 9)
    assert weights() == capi.HS_OK and n_out.value == 3
    assert ol.tolist() == [0, 5, 9, 9] and osz.tolist() == [4, 3, 2, 9] and di.tolist() == [k, k, k, 9]
    assert ws.tolist()[:3] == [k * (ONE // s) * s for s in (4, 3, 2)] and np.all(wc[3] == 9) and cnt[:3].sum() == 9 * k
    # the cover
    S = np.zeros((3, k, A))
    ms, am = np.full(3, 9.0), np.full(3, 9, np.uint32)

    def cover(cds=codes, kk=k, AA=A, lab=label, mn=2, SS=S, rows=3, o1=ms, o2=am):
        return lib.hs_cluster_cover_codes(vp(cds), n, kk, AA, vp(lab), mn, None if SS is None else vp(SS), rows,
                                          None if o1 is None else vp(o1), None if o2 is None else vp(o2))

    for v in (np.nan, np.inf, -np.inf, 2.0 ** 101, -1.3e30):
        T = S.copy()
        T[2, 1, 7] = v
        assert cover(SS=T) == bad, v
    for kw in (dict(mn=0), dict(kk=0), dict(kk=76), dict(AA=33), dict(cds=big), dict(lab=wrong), dict(rows=2),
               dict(rows=4), dict(SS=None), dict(o1=None), dict(o2=None)):
        assert cover(**kw) == bad, kw
    assert np.all(ms == 9.0) and np.all(am == 9)
    T = S.copy()
    T[:, :, 1] = 2.0 ** 100                          # the cap itself is legal
    assert cover(SS=T) == capi.HS_OK and ms.tolist() == [3 * 2.0 ** 100] * 3 and am.tolist() == [0, 3, 8]


def test_exports_and_profile_fields():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in ("hs_cluster_weighted_profile", "hs_cluster_weighted_profile_dev", "hs_cluster_pssm_cover",
                 "hs_cluster_pssm_cover_dev", "hs_cluster_weights_codes", "hs_cluster_cover_codes"):
        assert re.search(r"HS_API hs_status %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name)
    fields = [f for f, _ in capi._Profile._fields_]
    at = fields.index("summary_weight_rows")
    assert fields[at + 1] == "summary_weight_items" and at + 1 < fields.index("pssm_topk_sample")
    assert fields[-2:] == ["pssm_topk_sample", "pssm_topk_raised"]
    struct = header[header.index("typedef struct hs_profile"):header.index("} hs_profile;")]
    assert re.findall(r"^\s*(?:double|uint64_t|uint32_t)\s+(\w+);", struct, flags=re.M) == fields
    for name in ("cluster_weighted_profile", "cluster_weighted_profile_dev", "cluster_pssm_cover",
                 "cluster_pssm_cover_dev", "cluster_pssm"):
        assert callable(getattr(capi.Engine, name))


def test_header_under_asan_and_ubsan(tmp_path):
    """hs_cluster_pssm.h with a stand-alone main (tests/cluster_pssm_san.cpp), compiled and run under AddressSanitizer
    + UndefinedBehaviorSanitizer (the runtimes linked statically); nothing is loaded into python."""
    exe = tmp_path / "cluster_pssm_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cluster_pssm_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "cluster_pssm_san ok" in res.stdout
