"""The PSSM scan filter's tables (hsearch_amd/csrc/hs_pssm_tables.h, exported as hs_pssm_tables), on the host: no GPU.

THE INVARIANT: for every k-mer x, if the contract's ROUNDED fp64 score (pssm_ref.scores: +0.0, left to right) reaches
t[m], then F(x) = sum_p E2M3[code[m][p][x_p]] >= tau[m]; dead[m] = 1 only if no k-mer hits.  F is a sum of multiples
of 1/8 and is computed here exactly.  For k = 3 over 4 residues all 64 k-mers are checked, so "only if no k-mer hits"
is checked exhaustively too."""
import os
import subprocess

import numpy as np
import pytest

from hsearch_amd import HsError, capi

import pssm_cases
import pssm_ref
from pssm_cases import ALL64, check_invariant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exhaustive_random_profiles():
    S, t = pssm_cases.random_scales()
    nm = len(S)
    hits, passed, T = check_invariant(S, t, ALL64)
    assert hits[::3].min() >= 1
    # the filter is worth something on this set as well: it does not simply pass everything
    assert passed.sum() < 0.8 * 64 * nm
    # where t is the maximum the hits are exactly the maximisers, and none is lost
    assert np.all(hits[1::17] >= 1)


def test_exhaustive_threshold_outside_the_range():
    S, above = pssm_cases.threshold_above()
    hits, passed, T = check_invariant(S, above, ALL64)
    assert not hits.any() and np.all(T["dead"] == 1) and not passed.any()
    S, below = pssm_cases.threshold_below()
    hits, passed, T = check_invariant(S, below, ALL64)
    assert np.all(hits == 64) and np.all(passed == 64) and not T["dead"].any()
    # thresholds of any finite size
    for tt in (1e300, -1e300, 1.7e308, -1.7e308):
        S, t = pssm_cases.threshold_of_any_size(tt)
        hits, passed, T = check_invariant(S, t, ALL64)
        assert np.all(T["dead"] == (1 if tt > 0 else 0))
        assert np.all(hits == (0 if tt > 0 else 64))


def test_exhaustive_constant_profiles_and_zero():
    for S, t in (pssm_cases.constant_at_the_score(),     # exactly the one attainable score: all hit
                 pssm_cases.constant_below_the_score()):
        hits, passed, T = check_invariant(S, t, ALL64)
        assert np.all(hits == 64) and np.all(passed == 64)
    S, t = pssm_cases.constant_above_the_score()
    hits, passed, T = check_invariant(S, t, ALL64)
    assert not hits.any() and np.all(T["dead"] == 1)


def test_cancellation_family():
    """{+-1, +-2^60} in every position order: -1 + 2^60 - 2^60 is 0 in fp64 and -1 over the reals; at t = -0.5 the
    rounded sum is a hit where the real sum is none, and the filter must keep it."""
    S, t = pssm_cases.cancellation()
    sc = pssm_ref.scores(S, ALL64)
    # the family does what it is here for: some rounded score reaches t where the exact sum does not
    from fractions import Fraction
    exact = np.array([[sum(Fraction(S[m, p, x[p]]) for p in range(3)) for x in ALL64] for m in range(len(S))])
    assert np.any((sc >= t[:, None]) & (exact < t[:, None]))
    hits, passed, T = check_invariant(S, t, ALL64)
    assert hits.min() >= 1


def _planted(rng, k, A, members, mut):
    """Log-odds profile of a planted family: `members` copies of a random consensus, each position mutated with
    probability mut."""
    cons = rng.integers(0, A, size=k)
    fam = np.where(rng.random((members, k)) < mut, rng.integers(0, A, size=(members, k)), cons)
    counts = np.zeros((k, A))
    for p in range(k):
        counts[p] = np.bincount(fam[:, p], minlength=A)
    return capi.pssm_log_odds(counts[None], background=np.full(A, 1.0 / A))[0], fam.astype(np.uint8)


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(2303)
    k, A = 25, 20
    profs, fams = zip(*[_planted(rng, k, A, 50, mut) for mut in (0.2, 0.35, 0.5) for _ in range(2)])
    codes = rng.integers(0, A, size=(400000, k)).astype(np.uint8)
    S = np.array(profs)
    return dict(S=S, fams=fams, codes=codes, sc=pssm_ref.scores(S, codes))


def test_planted_families_invariant(planted):
    S, codes = planted["S"], planted["codes"][:100000]
    sc = planted["sc"][:, :100000]
    for rate in (1e-2, 1e-3, 1e-4):
        t = np.quantile(sc, 1.0 - rate, axis=1)
        hits, passed, T = check_invariant(S, t, codes)
        assert not T["dead"].any()
    # the families themselves, at the score of their weakest member (an attained score)
    for m, fam in enumerate(planted["fams"]):
        t = pssm_ref.scores(S[m:m + 1], fam).min(axis=1)
        hits, passed, T = check_invariant(S[m:m + 1], t, fam)
        assert hits[0] == len(fam)


def test_long_kmers_large_alphabet():
    rng = np.random.default_rng(2304)
    k, A = 75, 32
    S = np.array([_planted(rng, k, A, 50, mut)[0] for mut in (0.2, 0.5)] + [rng.normal(size=(k, A)) * 3])
    codes = rng.integers(0, A, size=(100000, k)).astype(np.uint8)
    sc = pssm_ref.scores(S, codes)
    for rate in (1e-2, 1e-4):
        hits, passed, T = check_invariant(S, np.quantile(sc, 1.0 - rate, axis=1), codes)
        assert np.all(passed < len(codes))


def test_selectivity(planted):
    """The table passes at most 4 x the hits at hit rates 10^-3 and 10^-4 (the construction passed <= 2.3 x when it
    was simulated; 4 x catches a table that rounds with a whole step of slack)."""
    S, codes, sc = planted["S"], planted["codes"], planted["sc"]
    for rate in (1e-3, 1e-4):
        t = np.quantile(sc, 1.0 - rate, axis=1)
        hits, passed, T = check_invariant(S, t, codes)
        print("rate %g: hits %s passed %s ratio %s" % (rate, hits, passed, np.round(passed / hits, 2)))
        assert np.all(hits >= 0.5 * rate * len(codes))
        assert np.all(passed <= 4 * hits)


def test_invalid_inputs_are_refused():
    S, t = np.zeros((2, 3, 4)), np.zeros(2)
    capi.pssm_tables(S, t)
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 101, -(2.0 ** 101)):
        S2 = S.copy()
        S2[1, 2, 3] = bad
        with pytest.raises(HsError) as e:
            capi.pssm_tables(S2, t)
        assert e.value.status == capi.HS_ERR_INVALID
    S2 = S.copy()
    S2[0, 0, 0] = 2.0 ** 100     # the cap itself is legal
    capi.pssm_tables(S2, t)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(HsError) as e:
            capi.pssm_tables(S, np.array([0.0, bad]))
        assert e.value.status == capi.HS_ERR_INVALID
    for shape in ((1, 76, 4), (1, 3, 33)):
        with pytest.raises(HsError):
            capi.pssm_tables(np.zeros(shape), np.zeros(1))


def test_decode_table_and_log_odds():
    assert pssm_ref.E2M3[8] == 1.0 and pssm_ref.E2M3[31] == 7.5 and pssm_ref.E2M3[63] == -7.5
    assert len(set(pssm_ref.E2M3[:32])) == 32 and np.all(np.diff(pssm_ref.E2M3[:32]) > 0)
    counts = np.array([[[3, 1, 0, 0], [0, 0, 4, 0]]])
    S = capi.pssm_log_odds(counts, background=np.full(4, 0.25), pseudo=1.0)
    assert np.allclose(S[0, 0], np.log2((np.array([3, 1, 0, 0]) + 0.25) / 5 / 0.25))
    S = capi.pssm_log_odds(counts)   # background from the counts: residue 3 never occurs, and nothing is infinite
    assert np.all(np.isfinite(S))


def test_host_tables_under_asan_and_ubsan(tmp_path):
    """The header with a stand-alone main (tests/pssm_tables_san.cpp), compiled and run under AddressSanitizer +
    UndefinedBehaviorSanitizer (the runtimes linked statically); nothing is loaded into python."""
    exe = tmp_path / "pssm_tables_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "pssm_tables_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pssm_tables_san ok" in res.stdout
