"""The probes' ranks inside their buckets (hs_rank_kernel, in front of the counting sort of the probes): every
probe must reach exactly one position of exactly one segment, whatever the batch looks like -- thousands of probes
of one bucket, no two probes of a bucket, probes of no bucket, one query, a batch after a larger one.

A small index whose few buckets hold most k-mers (2 * 10^4 25-mers, L = 4, K = 4, W = 300: 15 to 19 buckets per
table).  Every case draws its queries from one pool of distinct queries, so the CPU oracle runs once, over the
pool, and a case's expected hits are the pool's, repeated per query.  Each case first asserts from the oracle that
it is the case it claims to be (hits, probes of the hottest bucket, probes of no bucket), then compares the GPU's
hits under the automatic grouping, the counting sort (seg_mode=2: the ranks) and the sort of the probes
(seg_mode=1: no ranks) with the oracle's, and the candidate and join pair counts with the sum over the probes of
the probed bucket's size, computed in numpy from the bucket ints."""
import numpy as np
import pytest

from hsearch_amd import Engine, synth

pytestmark = pytest.mark.gpu

K_MER, K, L, W, R, N_DB = 25, 4, 4, 300.0, 40.0, 20000
_FIELDS = ("q", "id", "table", "dist", "cand")
N_HOT, N_NEAR, N_NOISY, N_FAR, N_SKEW = 3, 250, 60, 12, 12


def _rows_key(ints):
    """One bytes key per row of bucket ints."""
    ints = np.ascontiguousarray(ints, dtype=np.int32)
    return [r.tobytes() for r in ints]


@pytest.fixture(scope="module")
def world(oracle):
    a, b = synth.make_planes(K_MER, K, L, W)
    codes = synth.make_db(N_DB, K_MER)
    db = oracle.embed_codes(codes)
    db_ints = oracle.hash_all(a, b, W, db)
    size = []  # per table: bucket ints -> members
    for l in range(L):
        u, c = np.unique(db_ints[:, l, :], axis=0, return_counts=True)
        size.append(dict(zip(_rows_key(u), c.tolist())))
    # the pool: [hot | near | noisy | far | skew | distinct]
    hot = synth.embed(codes[[11, 4242, 17017]])
    near_codes, _ = synth.make_query_codes(codes, N_NEAR)
    near = synth.embed(near_codes)
    rng = np.random.Generator(np.random.MT19937(77))
    noisy = synth.embed(codes[rng.integers(0, N_DB, N_NOISY)]) + rng.normal(0.0, 1.0, size=(N_NOISY, 8 * K_MER))
    # Queries of no bucket that the join filter's int8 rows still carry: inside the coordinate table's range in
    # every column, but lined up with the first plane of every table (far) or of one table (skew), where no sum of
    # k table rows ever gets.  far: no bucket in any table; skew i: none in table i % L.
    lim = np.tile(np.abs(synth.coords()).max(axis=0), K_MER)
    far = np.sign(a[:, 0, :].sum(axis=0)) * lim * rng.uniform(0.8, 0.95, size=(N_FAR, 8 * K_MER))
    skew = np.stack([np.sign(a[i % L, 0, :]) * lim * rng.uniform(0.5, 0.65, size=8 * K_MER) for i in range(N_SKEW)])
    distinct, used = [], [set() for _ in range(L)]  # DB k-mers no two of which share a bucket in any table
    keys = [_rows_key(db_ints[:, l, :]) for l in range(L)]
    for i in range(N_DB):
        if all(keys[l][i] not in used[l] for l in range(L)):
            distinct.append(i)
            for l in range(L):
                used[l].add(keys[l][i])
    pool = np.ascontiguousarray(np.concatenate([hot, near, noisy, far, skew, synth.embed(codes[distinct])]))
    ix = oracle.Index(a, b, W, db)
    ref = ix.query(pool, R)
    ix.close()
    assert np.all(np.diff(ref["q"].astype(np.int64)) >= 0)
    cut = np.searchsorted(ref["q"], np.arange(len(pool) + 1))
    pool_ints = oracle.hash_all(a, b, W, pool)
    pool_keys = [_rows_key(pool_ints[:, l, :]) for l in range(L)]
    # members of the bucket each (pool query, table) probes; 0: no such bucket
    pool_size = np.array([[size[l].get(pool_keys[l][i], 0) for l in range(L)] for i in range(len(pool))], dtype=np.uint64)
    assert np.array_equal(pool_size, ref["cand"])  # (the oracle's own candidate counts say the same)
    eng = Engine(K_MER, K, L, W, a, b)
    eng.index_build(codes)
    o = np.cumsum([0, N_HOT, N_NEAR, N_NOISY, N_FAR, N_SKEW, len(distinct)])
    groups = {name: np.arange(o[i], o[i + 1]) for i, name in enumerate(("hot", "near", "noisy", "far", "skew", "distinct"))}
    yield dict(pool=pool, ref=ref, cut=cut, pool_keys=pool_keys, pool_size=pool_size, eng=eng, groups=groups)
    eng.close()


def _expected(w, pick):
    """The oracle's answer for the queries pool[pick]."""
    ref, cut = w["ref"], w["cut"]
    rows = np.concatenate([np.arange(cut[p], cut[p + 1]) for p in pick]) if len(pick) else np.zeros(0, dtype=np.int64)
    reps = np.array([cut[p + 1] - cut[p] for p in pick], dtype=np.int64)
    want = {f: ref[f][rows] for f in ("id", "table", "dist")}
    want["q"] = np.repeat(np.arange(len(pick), dtype=np.uint32), reps)
    want["cand"] = ref["cand"][pick]
    return want


def _probe_census(w, pick):
    """(probes of the hottest bucket, probes of no bucket, sum over the probes of their bucket's size)"""
    hottest, none = 0, 0
    for l in range(L):
        number = {}
        keys = np.array([number.setdefault(w["pool_keys"][l][p], len(number)) for p in pick])
        found = w["pool_size"][pick, l] > 0
        none += int((~found).sum())
        if found.any():
            hottest = max(hottest, int(np.unique(keys[found], return_counts=True)[1].max()))
    return hottest, none, int(w["pool_size"][pick].sum())


def _check(w, pick, what):
    eng, want = w["eng"], _expected(w, pick)
    centers = np.ascontiguousarray(w["pool"][pick])
    total = _probe_census(w, pick)[2]
    got = {}
    for mode in (0, 2, 1):  # automatic, counting sort over the bucket slots (ranks), sort of the probes (no ranks)
        eng.set_option("seg_mode", mode)
        try:
            got[mode] = eng.query(centers, R)
            prof = eng.profile()
        finally:
            eng.set_option("seg_mode", 0)
        for f in _FIELDS:
            assert np.array_equal(got[mode][f], want[f]), (what, mode, f)
        assert prof["candidates"] == total, (what, mode, prof["candidates"], total)
        assert prof["join_pairs"] == total, (what, mode, prof["join_pairs"], total)
    for f in _FIELDS:
        assert np.array_equal(got[2][f], got[1][f]), (what, f)


def _draw(w, names, nq, seed):
    ids = np.concatenate([w["groups"][n] for n in names])
    return ids[np.random.Generator(np.random.MT19937(seed)).integers(0, len(ids), nq)]


def test_copies_of_three_kmers_fill_one_bucket(world):
    pick = np.tile(world["groups"]["hot"], 1667)[:5000]
    hottest, none, total = _probe_census(world, pick)
    assert hottest >= 1600 and none == 0 and total > 0
    assert len(_expected(world, pick)["q"]) >= 5000  # every copy finds at least its own k-mer
    _check(world, pick, "hot")


def test_no_two_probes_share_a_bucket(world):
    pick = world["groups"]["distinct"]
    hottest, none, _ = _probe_census(world, pick)
    assert len(pick) >= 4 and hottest == 1 and none == 0  # (as many as the table with the fewest buckets allows)
    assert len(_expected(world, pick)["q"]) >= len(pick)
    _check(world, pick, "distinct")


def test_probes_of_no_bucket(world):
    g = world["groups"]
    hottest, none, _ = _probe_census(world, g["far"])
    assert none == L * N_FAR and hottest == 0
    missing = (world["pool_size"][g["skew"]] == 0).sum(axis=1)
    assert np.all((missing > 0) & (missing < L))
    _check(world, g["far"], "far alone")  # the pseudo-bucket alone: no hit, no item
    pick = _draw(world, ("far", "skew", "noisy", "near"), 700, 5)
    hottest, none, total = _probe_census(world, pick)
    assert none > 100 and hottest > 20 and total > 0 and len(_expected(world, pick)["q"]) > 0
    _check(world, pick, "mixed")


@pytest.mark.parametrize("nq", [1, 31, 257, 4097])
def test_batch_sizes(world, nq):
    pick = _draw(world, ("hot", "near", "noisy", "far", "skew"), nq, nq)
    if nq == 1:
        pick = world["groups"]["hot"][:1]
    assert len(_expected(world, pick)["q"]) > 0
    _check(world, pick, nq)


def test_smaller_call_after_a_larger_one(world):
    big = _draw(world, ("hot", "near", "noisy", "far", "skew"), 5000, 9)
    small = _draw(world, ("near", "noisy", "far", "skew"), 31, 10)
    assert len(_expected(world, small)["q"]) > 0
    for mode in (2, 0, 1):
        world["eng"].set_option("seg_mode", mode)
        try:
            got_big = world["eng"].query(np.ascontiguousarray(world["pool"][big]), R)
            got_small = world["eng"].query(np.ascontiguousarray(world["pool"][small]), R)
        finally:
            world["eng"].set_option("seg_mode", 0)
        for got, pick in ((got_big, big), (got_small, small)):
            want = _expected(world, pick)
            for f in _FIELDS:
                assert np.array_equal(got[f], want[f]), (mode, len(pick), f)
    _check(world, small, "small after large")
