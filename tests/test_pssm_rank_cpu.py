"""hs_pssm_rank without a GPU: the host rule (capi.pssm_rank_scores) and the sample rule (capi.pssm_rank_plan) against
the numpy contract of tests/pssm_rank_ref.py, every refused input on sentinel-filled outputs, the exports, and the
header under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hsearch_amd import HsError, capi

import pssm_rank_ref as ref
import pssm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NM = 33


def _mix(k, A, n):
    """The 33-profile mix of test_gpu_pssm_topk.py: dyadic entries (equal scores are common), a forbidden residue."""
    rng = np.random.default_rng(1000 * k + 10 * A + n)
    codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
    S = rng.normal(0, 2, size=(NM, k, A))
    S[::2] = rng.integers(-16, 17, size=S[::2].shape) / 4.0
    if k == 3:
        S = rng.integers(-1, 2, size=S.shape).astype(np.float64)  # 64 distinct k-mers, 7 distinct scores
    S[3, :, 0] = -1e30
    return codes, S, pssm_ref.scores(S, codes)


@pytest.mark.parametrize("k,A,n", [(25, 20, 5000), (3, 4, 200), (75, 32, 300)])
def test_host_rule_equals_numpy(k, A, n):
    codes, S, sc = _mix(k, A, n)
    rng = np.random.default_rng(5)
    for rank in (1, 2, 64, 65, 100, n - 1, n, rng.integers(1, n + 1, size=NM)):
        want = ref.from_scores(sc, rank)
        got = capi.pssm_rank_scores(codes, A, S, rank)
        ref.same(got, want, (k, A, n, rank))
        r = ref.ranks(rank, NM)
        assert np.all(got["cnt_gt"] < r) and np.all(r <= got["cnt_ge"])
        assert np.all((sc == got["t"][:, None]).any(axis=1))          # the bits of a score that occurs
    if k == 3:   # ties fill every rank
        got = capi.pssm_rank_scores(codes, A, S, n // 2)
        assert np.all(got["cnt_ge"] - got["cnt_gt"] > 1)
    empty = capi.pssm_rank_scores(codes, A, np.zeros((0, k, A)), 1)
    assert len(empty["t"]) == 0


def test_plan_equals_numpy():
    n = 5000
    for n_s in (1, 64, n):
        for rank in (1, 2, 64, 65, 100, 4999, n):
            for rnd in range(7):
                assert capi.pssm_rank_plan(rank, n, n_s, rnd) == ref.plan(rank, n, n_s, rnd), (n_s, rank, rnd)
    assert [capi.pssm_rank_plan(65, 5000, 64, j) for j in range(3)] == [13, 49, 65]
    assert [capi.pssm_rank_plan(100, 5000, 64, j) for j in range(2)] == [18, 65]
    assert capi.pssm_rank_plan(10 ** 4, 10 ** 7, 2 ** 16, 0) == 66 + 4 * 9 + 8
    big = 2 ** 32 - 1
    for rnd in (0, 5, 16, 17, 40):
        assert capi.pssm_rank_plan(big - 1, big, big - 1, rnd) == ref.plan(big - 1, big, big - 1, rnd)
    for rank, nn, n_s in ((0, 10, 5), (11, 10, 5), (1, 10, 0), (1, 10, 11), (1, 2 ** 32, 5)):
        with pytest.raises(HsError) as e:
            capi.pssm_rank_plan(rank, nn, n_s, 0)
        assert e.value.status == capi.HS_ERR_INVALID
    assert capi.load().hs_pssm_rank_plan(1, 10, 5, 0, None) == capi.HS_ERR_INVALID


def test_refused_inputs_write_nothing():
    lib = capi.load()
    k, A, n, nm = 3, 4, 10, 2
    codes = np.ones((n, k), np.uint8)
    S = np.full((nm, k, A), 0.5)
    rank = np.array([1, 10], np.uint64)
    t, ge, gt = np.full(nm, 9.0), np.full(nm, 9, np.uint64), np.full(nm, 9, np.uint64)
    v = capi._vp

    def call(cds=codes, nn=n, kk=k, AA=A, SS=S, m=nm, rk=rank, tt=t, g1=ge, g2=gt):
        def p(a):
            return None if a is None else v(a)
        return lib.hs_pssm_rank_scores(p(cds), nn, kk, AA, p(SS), m, p(rk), p(tt), p(g1), p(g2))

    bad = capi.HS_ERR_INVALID
    assert call(kk=0) == bad and call(AA=0) == bad and call(AA=33) == bad
    assert call(cds=None) == bad and call(SS=None) == bad and call(rk=None) == bad
    assert call(tt=None) == bad and call(g1=None) == bad and call(g2=None) == bad
    assert call(m=1 << 27) == bad
    assert call(nn=0) == bad                                           # an empty index refuses every rank
    assert call(rk=np.array([0, 10], np.uint64)) == bad and call(rk=np.array([1, 11], np.uint64)) == bad
    for x in (np.nan, np.inf, -np.inf, 2.0 ** 101):
        S2 = S.copy()
        S2[1, 2, 3] = x
        assert call(SS=S2) == bad
    c2 = codes.copy()
    c2[7, 1] = A
    assert call(cds=c2) == bad
    assert np.all(t == 9.0) and np.all(ge == 9) and np.all(gt == 9)
    assert call(m=0, SS=None, rk=None, tt=None, g1=None, g2=None) == capi.HS_OK       # nm == 0: nothing written
    assert call() == capi.HS_OK
    assert t.tolist() == [1.5, 1.5] and ge.tolist() == [10, 10] and gt.tolist() == [0, 0]


def test_exports_option_and_profile_fields():
    header = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in ("hs_pssm_rank", "hs_pssm_rank_dev", "hs_pssm_rank_scores", "hs_pssm_rank_plan", "hs_pssm_refine_rank"):
        assert re.search(r"HS_API hs_status %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name)
    assert capi.Engine.OPTIONS["pssm_rank_sample"] == 26 and "HS_OPT_PSSM_RANK_SAMPLE = 26" in header
    for name in ("pssm_rank", "pssm_rank_dev", "pssm_refine_rank"):
        assert callable(getattr(capi.Engine, name))
    fields = [f for f, _ in capi._Profile._fields_]
    i = fields.index("pssm_topk_sample")
    assert fields[i - 2:i] == ["pssm_rank_sample", "pssm_rank_retries"] and fields[-2:] == ["pssm_topk_sample",
                                                                                           "pssm_topk_raised"]
    struct = header[header.index("typedef struct hs_profile"):header.index("} hs_profile;")]
    declared = re.findall(r"^\s*(?:double|uint64_t|uint32_t)\s+(\w+);", struct, flags=re.M)
    assert declared == fields


def test_header_under_asan_and_ubsan(tmp_path):
    """hs_pssm_rank.h with a stand-alone main (tests/pssm_rank_san.cpp), compiled and run under AddressSanitizer +
    UndefinedBehaviorSanitizer (the runtimes linked statically); nothing is loaded into python."""
    exe = tmp_path / "pssm_rank_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "pssm_rank_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pssm_rank_san ok" in res.stdout
