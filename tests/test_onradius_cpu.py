"""The premises of tests/test_gpu_onradius.py, proved with the oracle alone (no GPU): every case's script family
really puts hundreds of co-bucketed pairs exactly on the radius, the three hit rules really split where the GPU
file says they do, and the own-radii construction really moves one hit per query across one double."""
import math

import numpy as np
import pytest

from tests import onradius_ref as orr
from tests import radii_ref as rr

FAMILIES, RANK = orr.FAMILIES, orr.RANK
MIN_PAIRS, MIN_QUERIES, MIN_NONZERO = 256, 64, 0.9


def test_covering_radius_and_radii_of():
    for d2 in (0.0, 1.0, 2.0, 1387.25, 1387.2500000000002, 3.0e6, 1e-300):
        r_on, r_sqrt, r_off = orr.radii_of(d2)
        assert r_on * r_on >= d2 and r_sqrt <= r_on <= math.nextafter(r_sqrt, math.inf)
        if d2 > 0.0:
            assert r_off < r_sqrt and r_off * r_off < d2 and not (math.sqrt(d2) <= r_off)
            assert math.nextafter(r_off, math.inf) == r_sqrt


@pytest.mark.parametrize("name,which", FAMILIES)
def test_family_puts_pairs_on_the_radius(oracle, name, which):
    f = orr.case_family(oracle, name, which)
    r_on, r_sqrt, r_off = f["radii"]
    regime = orr.CASES[name]["regime"]
    assert regime is None or regime[0] <= r_on <= regime[1]
    assert r_on * r_on < 30000.0 or f["table"] is not None
    db = orr.embed(oracle, f["db"], f["table"])
    centres = orr.embed(oracle, f["centres"], f["table"])
    ix = oracle.Index(f["a"], f["b"], f["W"], db)
    q, i, dist = orr.on_radius_pairs(oracle, ix, centres, f["radii"])
    print("%s/%s: R_on %r, %d on-radius pairs over %d queries, %d hits at R_on" %
          (name, which, r_on, len(q), len(set(q.tolist())), len(ix.query(centres, r_on)["q"])))
    assert len(q) >= MIN_PAIRS and len(set(q.tolist())) >= MIN_QUERIES
    want = np.full(len(dist), math.sqrt(f["d2"]))
    assert np.array_equal(dist.view(np.uint64), want.view(np.uint64))
    # ... and by the exact squared distance of each pair
    for qq, ii in list(zip(q.tolist(), i.tolist()))[::17]:
        assert oracle.pairwise_square(db[ii:ii + 1], centres[qq:qq + 1])[0, 0] == f["d2"]
    on = set(zip(q.tolist(), i.tolist()))
    at_sqrt = ix.query(centres, r_sqrt)
    lsh_sqrt = set(zip(at_sqrt["q"].tolist(), at_sqrt["id"].tolist()))
    brute = oracle.bruteforce(db, centres, r_sqrt)
    assert on <= set(zip(brute["q"].tolist(), brute["id"].tolist()))
    if which == "split":
        assert r_sqrt < r_on and r_sqrt * r_sqrt < f["d2"]
        assert not (on & lsh_sqrt)
        owner_sqrt = oracle.clustering(f["a"], f["b"], f["W"], r_sqrt, db)[1]
        owner_off = oracle.clustering(f["a"], f["b"], f["W"], r_off, db)[1]
        assert not np.array_equal(owner_sqrt, owner_off)
    else:
        assert on <= lsh_sqrt
    ix.close()


@pytest.mark.parametrize("name,which", FAMILIES)
def test_own_radii_move_one_hit_per_query(oracle, name, which):
    f = orr.case_family(oracle, name, which)
    db = orr.embed(oracle, f["db"], f["table"])
    centres = orr.jittered(orr.embed(oracle, f["centres"], f["table"]))
    ix = oracle.Index(f["a"], f["b"], f["W"], db)
    radii, picked = orr.own_radii(oracle, ix, db, centres, RANK)
    assert (radii > 0.0).mean() >= MIN_NONZERO
    up = np.nonzero((radii > 0.0) & (np.arange(len(radii)) % 2 == 0))[0]
    assert len(up) >= MIN_QUERIES
    at, _ = rr.stitch(ix.query, centres, radii)
    below, _ = rr.stitch(ix.query, centres, orr.lowered(radii))
    n_at, n_below = np.bincount(at["q"], minlength=len(radii)), np.bincount(below["q"], minlength=len(radii))
    assert np.array_equal(n_at[up], n_below[up] + 1)
    down = np.setdiff1d(np.arange(len(radii)), up)
    assert np.array_equal(n_at[down], n_below[down])       # already below their pair
    # the one hit more is the picked pair, the farthest of its query
    for q in up[::7]:
        sel = at["q"] == q
        assert at["id"][sel][np.argmax(at["dist"][sel])] == picked[q]
    ix.close()
