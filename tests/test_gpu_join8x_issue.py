"""hs_join8x_kernel's sign test and query-tile loads, pinned at the smallest shapes that reach them.

The kernel holds a work item's 128 bucket members as two groups of 64 (X, Y), streams the probing queries past
them in tiles of 32 (three tiles in flight), and decides per group and tile from ONE value per lane -- the signed
maximum over the lane's 32 accumulators -- whether any pair survived the filter.  A reduction that misses an
accumulator loses exactly the pairs that sit alone in their group and tile; a query-tile load with a wrong lane
offset mixes up queries of full tiles (32 rows) or of a segment's ragged last tile.  So one small index is built
whose buckets and query segments have chosen sizes, and neighbours are planted by hand:

  bucket (members)   segment (probing queries)   planted
  129                129                         every member is the source of one query (0..4 substitutions, a hit):
                                                 a survivor on every member position 0..127 of an item -- both groups,
                                                 all row tiles, result registers and lane quarters -- and on every
                                                 query position 0..95 of a group of three tiles, whatever order the
                                                 probes arrive in; the 129th member is an item of one row
  128                65                          two pairs EXACTLY on the radius, on the item's first and last member
                                                 (one survivor per group), each beside a query just outside; 61 queries
                                                 near nothing
  127                96                          no neighbour at all
  1                  97                          one neighbour of the only member, 96 queries near nothing
  700 (6 items)      127                         one neighbour in every item, each alone in its item

Queries near nothing are k-mers that hash to the bucket but are not in the database (random 25-mers are > 50 apart).
The radius is the covering radius of an edit script's squared distance (tests/onradius_ref.py), about 40 like the
benchmark's.  Everything planted is checked on the oracle alone first (`_case`): a set that does not hold there
fails the test, it is never skipped.  Then the library has to return the oracle's candidates and hits exactly, with
the streaming kernel taking all segments or only those above 64 queries, items dealt in chunks and XCD runs, in
`join` and in `stream` verify mode, at the radius and one double below it."""
import math

import numpy as np
import pytest

from hsearch_amd import Engine, synth

from tests import onradius_ref as onr

K_MER, KK, L, W, N_POOL = 25, 2, 2, 150.0, 40000
SIZES = {"full": (129, 129), "radius": (128, 65), "none": (127, 96), "single": (1, 97), "items": (700, 127)}
_CASE = {}


def _bucket_ids(ints, table):
    """Bucket number per row in one table (rows of equal ints share a number)."""
    _, inv = np.unique(ints[:, table, :], axis=0, return_inverse=True)
    return inv.ravel()


def _mutate(rng, x, m):
    y = x.copy()
    pos = rng.choice(K_MER, size=m, replace=False)
    y[pos] = (y[pos] + rng.integers(1, 20, size=m)) % 20
    return y


def _dist(oracle, x, y):
    p = oracle.embed_codes(np.stack([x, y]).astype(np.uint8))
    return math.sqrt(float(oracle.pairwise_square(p[1:], p[:1])[0, 0]))


def _case(oracle):
    """The database, the queries and the oracle's answers, built once: dict(codes, qcodes, a, b, R, R_off, want,
    want_off, ...).  Asserts on the oracle alone that every planted set is what the docstring says."""
    if _CASE:
        return _CASE
    rng = np.random.default_rng(771)
    a, b = synth.make_planes(K_MER, KK, L, W, seed=772)
    pool = synth.make_db(N_POOL, K_MER, seed=773)

    def key0(c):          # table-0 bucket ints of k-mers
        c = np.ascontiguousarray(np.atleast_2d(c), dtype=np.uint8)
        return oracle.hash_all(a, b, W, oracle.embed_codes(c))[:, 0, :]

    pool_b = _bucket_ids(oracle.hash_all(a, b, W, oracle.embed_codes(pool)), 0)
    by_size = sorted(range(pool_b.max() + 1), key=lambda g: (pool_b == g).sum())
    # the five target buckets: the smallest pool buckets with spare members to serve as queries near nothing
    need = sorted(SIZES.items(), key=lambda kv: kv[1][0] + kv[1][1])
    target, used = {}, set()
    for name, (m_size, q_size) in need:
        g = next(g for g in by_size if g not in used and (pool_b == g).sum() >= m_size + q_size + 8)
        used.add(g)
        target[name] = g
    # the database: every other bucket whole, the targets cut to size (the first members by id); the rest are spares
    keep = np.ones(N_POOL, dtype=bool)
    spare = {}
    for name, g in target.items():
        ids = np.flatnonzero(pool_b == g)
        keep[ids[SIZES[name][0]:]] = False
        spare[name] = pool[ids[SIZES[name][0]:]]
    # big buckets of the pool would only cost time: drop whatever is in no target bucket beyond 3000 members a bucket
    for g in range(pool_b.max() + 1):
        if g not in used:
            keep[np.flatnonzero(pool_b == g)[3000:]] = False
    codes = np.ascontiguousarray(pool[keep])
    members = {name: np.flatnonzero(pool_b[keep] == g) for name, g in target.items()}     # ids, ascending
    bkey = {name: key0(codes[members[name][0]])[0] for name in target}

    def in_bucket(name, x):
        return bool((key0(x)[0] == bkey[name]).all())

    # ---- the radius: an edit script of 5 substitutions whose d2 has sqrt(d2) == its covering radius
    (src, dst, d2_on), _ = onr.find_scripts(oracle, K_MER, None, 7801, 5, (38.0, 43.0))
    R, _, R_off = onr.radii_of(d2_on)
    assert R * R >= d2_on > R_off * R_off
    # the item's first and last member become k-mers that carry the script's source residues, still in the bucket
    on_pairs, queries, owner = [], [], []

    def add(name, q):
        assert in_bucket(name, q), name
        queries.append(q)
        owner.append(name)

    taken = 0
    for slot in (0, 127):
        for _ in range(4000):
            # (a spare beyond those that serve as queries: the member made from it stays near it)
            base = spare["radius"][rng.integers(SIZES["radius"][1], len(spare["radius"]))].copy()
            pos = np.sort(rng.choice(K_MER, size=5, replace=False))
            x = base.copy()
            x[pos] = src[:5]
            y = x.copy()
            y[pos] = dst[:5]
            free = np.setdiff1d(np.arange(K_MER), pos)
            z = y.copy()
            p = rng.choice(free)
            z[p] = (z[p] + 1 + int(dst[5]) % 19) % 20
            if in_bucket("radius", x) and in_bucket("radius", y) and in_bucket("radius", z):
                break
        else:
            raise AssertionError("no on-radius member for slot %d" % slot)
        codes[members["radius"][slot]] = x
        on_pairs.append((len(queries), int(members["radius"][slot])))
        add("radius", y)        # exactly on the radius
        add("radius", z)        # one more edit: just outside
        taken += 2
    for q in spare["radius"][:SIZES["radius"][1] - taken]:
        add("radius", q)

    def neighbour(name, x, m):
        """x with m substitutions (fewer if that is what it takes), in x's bucket and within R of x."""
        for mm in range(m, -1, -1):
            for _ in range(200):
                y = _mutate(rng, x, mm)
                if in_bucket(name, y) and _dist(oracle, x, y) <= R_off:
                    return y
        raise AssertionError("no neighbour")

    for i, mid in enumerate(members["full"]):
        add("full", neighbour("full", codes[mid], i % 5))
    for q in spare["none"][:SIZES["none"][1]]:
        add("none", q)
    add("single", neighbour("single", codes[members["single"][0]], 1))
    for q in spare["single"][:SIZES["single"][1] - 1]:
        add("single", q)
    lone_slots = [5, 128 + 70, 256 + 127, 384 + 0, 512 + 64, 640 + 59]      # one per item; 699 = the last member
    for s in lone_slots:
        add("items", neighbour("items", codes[members["items"][s]], 2))
    for q in spare["items"][:SIZES["items"][1] - len(lone_slots)]:
        add("items", q)
    order = rng.permutation(len(queries))
    qcodes = np.ascontiguousarray(np.array(queries, dtype=np.uint8)[order])
    owner = [owner[i] for i in order]
    new_index = np.argsort(order)
    on_pairs = [(int(new_index[q]), mid) for q, mid in on_pairs]

    # ---- the oracle alone: sizes, then every planted set
    pts, cpts = oracle.embed_codes(codes), oracle.embed_codes(qcodes)
    db_b = _bucket_ids(oracle.hash_all(a, b, W, np.concatenate([pts, cpts])), 0)
    q_b = db_b[len(codes):]
    db_b = db_b[:len(codes)]
    ix = oracle.Index(a, b, W, pts)
    want, want_off = ix.query(cpts, R), ix.query(cpts, R_off)
    ix.close()
    hits = set(zip(want["q"].tolist(), want["id"].tolist()))
    for name, (m_size, q_size) in SIZES.items():
        g = db_b[members[name][0]]
        assert (db_b == g).sum() == m_size, (name, "members")
        assert np.array_equal(np.flatnonzero(db_b == g), members[name])
        qs = np.flatnonzero(q_b == g)
        assert len(qs) == q_size and all(owner[q] == name for q in qs), (name, "queries")
        inside = [(q, i) for (q, i) in hits if q_b[q] == g and db_b[i] == g]
        if name == "full":
            assert {i for _, i in inside} == set(members[name].tolist())       # every member position
            assert {q for q, _ in inside} == set(qs.tolist())                 # every query position
        elif name == "radius":
            assert sorted(inside) == sorted(on_pairs)
        elif name == "none":
            assert inside == []
        elif name == "single":
            assert len(inside) == 1
        else:
            slots = sorted(int(np.searchsorted(members[name], i)) for _, i in inside)
            assert slots == lone_slots                                         # one survivor per item, alone in it
    off = set(zip(want_off["q"].tolist(), want_off["id"].tolist()))
    for q, i in on_pairs:
        sel = (want["q"] == q) & (want["id"] == i)
        assert sel.sum() == 1 and want["dist"][sel][0] == math.sqrt(d2_on) and (q, i) not in off
    assert len(want["q"]) - len(want_off["q"]) == len(on_pairs)
    _CASE.update(codes=codes, qcodes=qcodes, a=a, b=b, R=R, R_off=R_off, want=want, want_off=want_off,
                 on_pairs=on_pairs)
    return _CASE


def _assert_equal(got, want, what):
    assert np.array_equal(got["cand"], want["cand"]), what
    for f in ("q", "id", "table", "dist"):
        assert np.array_equal(got[f], want[f]), (what, f)


def test_planted_sets_hold_on_the_oracle(oracle):
    """No GPU: the construction alone (sizes of buckets and segments, every planted neighbour, the pairs on the
    radius), so that a planted set that does not hold shows up where there is no GPU, too."""
    c = _case(oracle)
    assert len(c["want"]["q"]) > 129 and len(c["on_pairs"]) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("routing", ["all_streamed", "above_64_streamed", "chunks_of_3_xcd_runs", "chunks_of_64"])
def test_join8x_every_slot_ragged_tiles_and_on_radius(oracle, routing):
    c = _case(oracle)
    opts = {"all_streamed": dict(join_resident=1), "above_64_streamed": dict(join_resident=2),
            "chunks_of_3_xcd_runs": dict(join_resident=1, join_xcd_run=2, join_chunk=3),
            "chunks_of_64": dict(join_resident=2, join_xcd_run=0, join_chunk=64)}[routing]
    eng = Engine(K_MER, KK, L, W, c["a"], c["b"], options=opts)
    eng.index_build(c["codes"])
    eng.set_verify_mode("join")
    for R, want in ((c["R"], c["want"]), (c["R_off"], c["want_off"])):
        got = eng.query_codes(c["qcodes"], R)
        p = eng.profile()
        # the streaming kernel ran, on items of its own: the test cannot pass on another kernel
        assert p["join_i8_batches"] > 0 and p["join_items"] > p["join_items_resident"], p
        _assert_equal(got, want, (routing, "join", R))
    eng.set_verify_mode("stream")
    _assert_equal(eng.query_codes(c["qcodes"], c["R"]), c["want"], (routing, "stream"))
    eng.close()
