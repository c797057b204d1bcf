"""Multi-probe restatement on the CPU: the heap generator against exhaustive enumeration, and the T = 0 search
against the oracle's one-probe search."""
import numpy as np
import pytest

from hsearch_amd import capi, synth
from tests import multiprobe_ref as mp


def _z_from(x):
    return mp.sorted_distances(np.asarray(x, dtype=np.float64))


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6])
def test_heap_matches_exhaustive_order(K):
    rng = np.random.default_rng(100 + K)
    for trial in range(25):
        x = rng.random(K)
        if trial % 5 == 1:
            x[:] = 0.5  # every distance ties
        elif trial % 5 == 2:
            x[: K // 2 + 1] = rng.choice([0.25, 0.75], size=K // 2 + 1)  # ties across functions and deltas
        elif trial % 5 == 3:
            x = np.round(x * 4) / 4  # z = 0 and z = 1 included
        z = _z_from(x)
        full = mp.all_valid_sets(z)
        assert len(full) == 3 ** K - 1
        for T in sorted({1, 2, 5, 7, 13, min(63, 3 ** K - 1)}):
            if T > 3 ** K - 1:
                continue
            got = mp.perturbation_sets(z, T)
            # the heap pops every set (valid or not) in (score, mask) order: its emitted sets are a prefix of the
            # exhaustive valid order, cut by the T limit or the 4 (T + 1) pop limit
            assert got == full[:len(got)]
            pops_order = sorted((mp.score(z, m), m) for m in range(1, 1 << (2 * K)))
            first_pops = [m for _, m in pops_order[:4 * (T + 1)]]
            want = [m for m in first_pops if mp.is_valid(z, m)][:T]
            assert got == want


def test_probe_zero_is_home_bucket(oracle):
    k, K, L, W = 15, 6, 3, 7.0
    a, b = synth.make_planes(k, K, L, W)
    pts = oracle.embed_codes(synth.make_db(40, k, seed=3))
    buckets, valid = mp.probe_buckets(oracle, a, b, W, pts, 4)
    assert np.array_equal(buckets[:, :, 0, :], oracle.hash_all(a, b, W, pts))
    assert valid[:, :, 0].all()
    # every probe differs from the home bucket in one to three functions by exactly one
    diff = buckets[:, :, 1:, :].astype(np.int64) - buckets[:, :, :1, :]
    assert np.abs(diff).max() == 1
    assert (np.abs(diff).sum(axis=3)[valid[:, :, 1:] == 1] >= 1).all()


@pytest.mark.parametrize("k,K,L,W,R", [(25, 4, 4, 100.0, 40.0), (15, 6, 3, 30.0, 30.0)])
def test_search_without_extra_probes_is_the_oracle(oracle, k, K, L, W, R):
    a, b = synth.make_planes(k, K, L, W)
    codes = synth.make_db(3000, k)
    db = oracle.embed_codes(codes)
    centers, _ = synth.make_queries(codes, 60, jitter=0.25)
    want = oracle.Index(a, b, W, db).query(centers, R)
    got = mp.search(oracle, a, b, W, db, centers, R, 0)
    for f in ("q", "id", "table", "dist", "cand"):
        assert np.array_equal(got[f], want[f]), f
    more = mp.search(oracle, a, b, W, db, centers, R, 6)
    assert set(zip(got["q"], got["id"])) <= set(zip(more["q"], more["id"]))


def test_exports_name_the_calls():
    assert "hs_set_multiprobe" in capi.EXPORTS and "hs_probe_buckets" in capi.EXPORTS
