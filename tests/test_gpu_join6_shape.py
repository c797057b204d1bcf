"""hs_join6x_kernel's survivor path: one compare per accumulator register is the wave's ballot for that register,
only a column tile whose maximum passed is looked at, and per-lane indices are formed for registers that hold a
survivor.  A register, a row tile, a lane quarter or a column that the path skips loses exactly the pairs that sit
there, so the pairs are put everywhere:

  own      a bucket of 128 members queried with the codes of its own members: pair (m, m) is a hit at every radius, so
           every row of every row tile, both accumulator halves, every accumulator register, every lane quarter and
           every column of a query tile carries a survivor
  edges    buckets of 31 / 32 / 33 / 97 / 700 members against segments of 128 / 65 / 96 / 97 / 95 queries (last tiles of
           32, 1, 32, 1 and 31 rows): rows past the last member and columns past the last query are computed and must
           be masked
  edges2   the same segments against buckets of 63 / 64 / 65 / 1 / 129 members

The first queries of a segment are the codes of members spread over the whole bucket (a hit each, in every work item),
the rest are k-mers of the same bucket that are not in the database.  R = 0 leaves the pairs (m, m) and duplicates
alone; the second radius is about the benchmark's 40.  k = 25 and 21, `join_resident=1` so that every segment takes the
streaming kernel, with and without XCD runs, and with one radius per parity.  Every result is the oracle's, compared
exactly; `join_f6_batches` says that the FP6 kernel ran.  The constructions are checked on the oracle alone where
there is no GPU."""
import numpy as np
import pytest

from hsearch_amd import Engine, synth

KK, L, W, N_POOL = 2, 2, 150.0, 40000
R_NEAR = 40.0
SEGMENTS = (128, 65, 96, 97, 95)
SETS = {"own": ((128, 128),),
        "edges": tuple(zip((31, 32, 33, 97, 700), SEGMENTS)),
        "edges2": tuple(zip((63, 64, 65, 1, 129), SEGMENTS))}
_CASES = {}


def _case(oracle, k, name):
    """dict(codes, qcodes, a, b, want={R: oracle's answer}, own=[(query, member id)]), built once per (k, name)."""
    if (k, name) in _CASES:
        return _CASES[k, name]
    sizes = SETS[name]
    rng = np.random.default_rng(9100 + k)
    a, b = synth.make_planes(k, KK, L, W, seed=772)
    pool = synth.make_db(N_POOL, k, seed=773)
    ints = oracle.hash_all(a, b, W, oracle.embed_codes(pool))
    _, pool_b = np.unique(ints[:, 0, :], axis=0, return_inverse=True)
    pool_b = pool_b.ravel()
    count = np.bincount(pool_b)
    by_size = np.argsort(count, kind="stable")
    keep = np.zeros(N_POOL, dtype=bool)
    used, spares, target = set(), [], []
    for m_size, q_size in sizes:
        g = int(next(g for g in by_size if g not in used and count[g] >= max(m_size, q_size) + 8))
        used.add(g)
        ids = np.flatnonzero(pool_b == g)
        keep[ids[:m_size]] = True
        spares.append(pool[ids[m_size:]])
        target.append(g)
    for g in range(len(count)):            # the rest of the database: up to 200 members of every other bucket
        if g not in used:
            keep[np.flatnonzero(pool_b == g)[:200]] = True
    codes = np.ascontiguousarray(pool[keep])
    db_b = pool_b[keep]
    queries, own = [], []
    for (m_size, q_size), g, spare in zip(sizes, target, spares):
        members = np.flatnonzero(db_b == g)
        assert len(members) == m_size
        n_own = min(m_size, q_size)
        for j in range(n_own):             # members spread over the bucket: every work item has one
            mid = int(members[j * m_size // n_own])
            own.append((len(queries), mid))
            queries.append(codes[mid])
        queries.extend(spare[:q_size - n_own])
    order = rng.permutation(len(queries))
    qcodes = np.ascontiguousarray(np.array(queries, dtype=np.uint8)[order])
    new_index = np.argsort(order)
    own = [(int(new_index[q]), mid) for q, mid in own]
    # ---- the oracle alone: segment sizes, and every own pair a hit at both radii
    pts, cpts = oracle.embed_codes(codes), oracle.embed_codes(qcodes)
    q_ints = oracle.hash_all(a, b, W, cpts)[:, 0, :]
    for (m_size, q_size), g in zip(sizes, target):
        key = ints[np.flatnonzero(pool_b == g)[0], 0, :]
        assert int((q_ints == key).all(axis=1).sum()) == q_size, (name, m_size, q_size)
    ix = oracle.Index(a, b, W, pts)
    want = {R: ix.query(cpts, R) for R in (0.0, R_NEAR)}
    ix.close()
    for R, w in want.items():
        hits = set(zip(w["q"].tolist(), w["id"].tolist()))
        assert all(p in hits for p in own), (name, R)
    assert len(want[R_NEAR]["q"]) >= len(want[0.0]["q"]) >= len(own)
    _CASES[k, name] = dict(codes=codes, qcodes=qcodes, a=a, b=b, want=want, own=own)
    return _CASES[k, name]


def _engine(c, k, **opts):
    opts = dict(dict(join_resident=1, join_f6=1), **opts)
    eng = Engine(k, KK, L, W, c["a"], c["b"], options=opts)
    eng.index_build(c["codes"])
    eng.set_verify_mode("join")
    return eng


def _assert_equal(got, want, what):
    assert np.array_equal(got["cand"], want["cand"]), what
    for f in ("q", "id", "table", "dist"):
        assert np.array_equal(got[f], want[f]), (what, f)


@pytest.mark.parametrize("name", sorted(SETS))
def test_constructions_hold_on_the_oracle(oracle, name):
    """No GPU: bucket and segment sizes, and a hit on every own pair (asserted in _case)."""
    c = _case(oracle, 25, name)
    n_own = sum(min(m, q) for m, q in SETS[name])
    assert len(c["own"]) == n_own and len(c["qcodes"]) == sum(q for _, q in SETS[name])
    if name == "own":                      # every member position 0..127 and every query position 0..127
        assert len({q for q, _ in c["own"]}) == 128 and len({i for _, i in c["own"]}) == 128


@pytest.mark.gpu
@pytest.mark.parametrize("k", [25, 21])
@pytest.mark.parametrize("routing", ["default", "xcd_runs"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_survivors_everywhere_equal_the_oracle(oracle, name, routing, k):
    c = _case(oracle, k, name)
    opts = dict() if routing == "default" else dict(join_xcd_run=2, join_chunk=3)
    eng = _engine(c, k, **opts)
    for R, want in c["want"].items():
        got = eng.query_codes(c["qcodes"], R)
        p = eng.profile()
        assert p["join_f6_batches"] > 0 and p["join_items_resident"] == 0, p
        _assert_equal(got, want, (name, k, routing, R))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges", "edges2"])
def test_per_query_radii(oracle, name):
    """Even queries at R_NEAR, odd ones at 0: the threshold differs from column to column of a tile."""
    k = 25
    c = _case(oracle, k, name)
    nq = len(c["qcodes"])
    wants = (c["want"][R_NEAR], c["want"][0.0])
    parts = [{f: w[f][(w["q"] % 2) == r] for f in ("q", "id", "table", "dist")} for r, w in enumerate(wants)]
    order = np.argsort(np.concatenate([p["q"] for p in parts]), kind="stable")
    want = {f: np.concatenate([p[f] for p in parts])[order] for f in ("q", "id", "table", "dist")}
    want["cand"] = wants[0]["cand"]
    eng = _engine(c, k, wide_rows=2)       # (4-column rows whatever the radius)
    got = eng.query_radii(c["qcodes"], np.where(np.arange(nq) % 2 == 0, R_NEAR, 0.0), codes=True)
    assert eng.profile()["join_f6_batches"] > 0
    _assert_equal(got, want, (name, "parity radii"))
    eng.close()
