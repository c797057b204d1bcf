"""The join's survivors refined from residue codes (hs_refine_codes_kernel) and the single query row that path
keeps (hs_qprep8_codes_kernel without its second row): every way a k-mer query enters -- recognised centres,
codes, per-query radii, the self-join from codes -- against the CPU oracle, exactly (q, id, table, dist, cand),
at one and two packed words per k-mer, with the built-in 20-letter table and a table of 29 letters.  The same
queries jittered run from the centres, where hs_refine8_kernel still refines: they must agree with the oracle too.

The small world of tests/test_gpu_probe_ranks.py: 2 * 10^4 k-mers, L = 4, K = 4, W = 300 -- a few buckets per table,
so nearly every pair is a candidate and the filters see what the hashing of a large index would have kept from
them -- and copies of three k-mers among the queries for the first-seen rule.  One oracle run per shape over the
pool of 257 queries; a batch of n queries is the pool's first n, and its expected hits are the pool's for them.
Each case asserts from the oracle first that it has hits in more than one table.

Pairs exactly on the radius and just outside it: a small script family of tests/onradius_ref.py; the premise (the
on-radius pairs are hits under both rules at R_on and no hit at R_off) is asserted on the oracle before the GPU
runs."""
import numpy as np
import pytest

from hsearch_amd import Engine, synth
from tests import onradius_ref as orr
from tests import radii_ref as rr

pytestmark = pytest.mark.gpu

K, L, W, R, N_DB, N_POOL, N_SELF = 4, 4, 300.0, 40.0, 20000, 257, 257
_FIELDS = ("q", "id", "table", "dist", "cand")
# shape -> (k, rows of a custom coordinate table or None): one and two packed words, both table sizes
SHAPES = {"k21": (21, None), "k25": (25, None), "k39": (39, None), "k50": (50, None), "k25_a29": (25, 29)}
BATCHES = (1, 63, 64, 65, 257)


def _table(rows):
    """A coordinate table of `rows` letters on the built-in table's scale, rounded with "%g" (the points-file
    route, as tests/onradius_ref.py:case_table does)."""
    if rows is None:
        return None
    t = np.random.default_rng(2900 + rows).normal(0.0, float(synth.coords().std()), size=(rows, 8))
    return np.array([[float("%g" % v) for v in row] for row in t])


def build_world(oracle, shape):
    """Everything of a shape that needs no GPU: the index, the query pool and the oracle's answers."""
    k, rows = SHAPES[shape]
    table = _table(rows)
    alpha = 20 if table is None else len(table)
    rng = np.random.Generator(np.random.MT19937(1000 + k + alpha))
    a, b = synth.make_planes(k, K, L, W)
    codes = rng.integers(0, alpha, size=(N_DB, k), dtype=np.uint8)
    # neighbours inside the DB, for the self-join: rows 0..127 are rows 128..255 with 0..2 substitutions
    codes[:128] = codes[128:256]
    for s in range(2):
        sel = np.nonzero(rng.integers(0, 3, 128) > s)[0]
        codes[sel, rng.integers(0, k, len(sel))] = rng.integers(0, alpha, len(sel), dtype=np.uint8)
    # the pool: three DB k-mers, copies of them (first-seen rule: every copy meets the same members in the same
    # tables), then DB k-mers with 0..4 substitutions
    hot = codes[[11, 4242, 17017]]
    near = codes[rng.integers(0, N_DB, N_POOL - 9)].copy()
    for s in range(4):
        sel = np.nonzero(rng.integers(0, 5, len(near)) > s)[0]
        near[sel, rng.integers(0, k, len(sel))] = rng.integers(0, alpha, len(sel), dtype=np.uint8)
    q_codes = np.ascontiguousarray(np.concatenate([hot, hot, hot, near]))
    assert len(q_codes) == N_POOL
    db = orr.embed(oracle, codes, table)
    pts = orr.embed(oracle, q_codes, table)
    ix = oracle.Index(a, b, W, db)
    ref = ix.query(pts, R)
    assert np.all(np.diff(ref["q"].astype(np.int64)) >= 0)
    assert len(np.unique(ref["table"])) > 1, "premise: hits in more than one table"
    jit = pts + np.random.default_rng(11).normal(0.0, 0.05, size=pts.shape)
    ref_jit = ix.query(jit, R)
    assert len(np.unique(ref_jit["table"])) > 1
    # per-query radii: R, a little less, zero (only an equal k-mer is a hit) and a larger one, by query number
    radii = np.array([R, 0.75 * R, 0.0, 1.1 * R])[np.arange(N_POOL) % 4]
    ref_radii, _ = rr.stitch(ix.query, pts, radii)
    assert len(np.unique(ref_radii["table"])) > 1
    # the self-join's first N_SELF rows: the search of those k-mers without each one's pair with itself
    own = ix.query(db[:N_SELF], R)
    keep = own["id"] != own["q"]
    ref_self = dict(i=own["q"][keep], j=own["id"][keep], table=own["table"][keep], dist=own["dist"][keep])
    assert len(ref_self["i"]) > 0
    # R = 0: the queries equal to a DB k-mer find it and its equals -- the oracle's hits at distance 0 (d2 <= 0)
    zero = ref["dist"] == 0.0
    ref_zero = dict({f: ref[f][zero] for f in ("q", "id", "table", "dist")}, cand=ref["cand"])
    assert len(ref_zero["q"]) >= 9
    ix.close()
    return dict(k=k, table=table, a=a, b=b, codes=codes, q_codes=q_codes, pts=pts, jit=jit, radii=radii, ref=ref,
                ref_jit=ref_jit, ref_radii=ref_radii, ref_self=ref_self, ref_zero=ref_zero)


@pytest.fixture(scope="module", params=list(SHAPES))
def world(request, oracle):
    w = build_world(oracle, request.param)
    eng = Engine(w["k"], K, L, W, w["a"], w["b"], coords=w["table"])
    eng.index_build(w["codes"])
    w["eng"] = eng
    yield w
    eng.close()


def _first(ref, n):
    """The oracle's answer for the pool's first n queries."""
    m = int(np.searchsorted(ref["q"], n))
    out = {f: ref[f][:m] for f in ("q", "id", "table", "dist")}
    out["cand"] = ref["cand"][:n]
    return out


def _same(got, want, what, fields=_FIELDS):
    for f in fields:
        assert np.array_equal(got[f], want[f]), (what, f, len(got[f]), len(want[f]))
    assert np.array_equal(got["dist"].view(np.uint64), want["dist"].view(np.uint64)), (what, "dist bits")


def test_recognised_centres_and_codes(world):
    eng = world["eng"]
    got = eng.query(world["pts"], R)
    assert eng.profile()["queries_recognised"] == N_POOL
    _same(got, world["ref"], "k-mer centres")
    _same(eng.query_codes(world["q_codes"], R), world["ref"], "codes")
    # the two filters against no refinement at all: the refinement never changes a result
    eng.set_option("refine8", 0)
    try:
        _same(eng.query_codes(world["q_codes"], R), world["ref"], "codes, refine8=0")
    finally:
        eng.set_option("refine8", 1)


def test_jittered_centres_take_the_int8_refinement(world):
    eng = world["eng"]
    got = eng.query(world["jit"], R)
    assert eng.profile()["queries_recognised"] == 0
    _same(got, world["ref_jit"], "jittered centres")


def test_per_query_radii(world):
    eng = world["eng"]
    _same(eng.query_radii(world["q_codes"], world["radii"], codes=True), world["ref_radii"], "radii, codes")
    _same(eng.query_radii(world["pts"], world["radii"]), world["ref_radii"], "radii, k-mer centres")


def test_self_join_from_codes(world):
    got = world["eng"].self_join(R, sqrt_test=False, first=0, count=N_SELF)
    _same(got, world["ref_self"], "self-join", ("i", "j", "table", "dist"))


def test_radius_zero(world):
    eng = world["eng"]
    _same(eng.query_codes(world["q_codes"], 0.0), world["ref_zero"], "R = 0, codes")
    _same(eng.query(world["pts"], 0.0), world["ref_zero"], "R = 0, k-mer centres")


@pytest.mark.parametrize("n", BATCHES)
def test_batch_sizes(world, n):
    eng = world["eng"]
    want = _first(world["ref"], n)
    assert len(want["q"]) > 0
    _same(eng.query_codes(world["q_codes"][:n], R), want, ("codes", n))
    _same(eng.query(np.ascontiguousarray(world["pts"][:n]), R), want, ("k-mer centres", n))


# ---- pairs exactly on the radius, and one double outside
# (name of the tests/onradius_ref.py case whose script and hash family are used, smaller: 64 centres, 1000 noise k-mers)
ON_RADIUS = ("k25", "k39", "k50", "k25_t05")


def build_family(oracle, name):
    c = orr.CASES[name]
    table = orr.case_table(name)
    seed = 7000 + sum(map(ord, name))
    agree, _ = orr.find_scripts(oracle, c["k"], table, seed, c["m"], c["regime"])
    centres, db_codes, d2 = orr.script_family(oracle, c["k"], c["m"], seed, table, n_centres=64, noise=1000,
                                              script=agree[:2])
    assert d2 == agree[2]
    radii = orr.radii_of(d2)
    assert radii[0] == radii[1]      # (both rules tie at the same double)
    Wf = c["W"] if c["W"] is not None else float("%.3g" % (3.2 * radii[0]))
    a, b = synth.make_planes(c["k"], c["K"], c["L"], Wf)
    db = orr.embed(oracle, db_codes, table)
    kmers = orr.embed(oracle, centres, table)
    ix = oracle.Index(a, b, Wf, db)
    want = {r: ix.query(kmers, r) for r in (radii[0], radii[2])}
    q, i, dist = orr.on_radius_pairs(oracle, ix, kmers, radii)
    ix.close()
    # the premise, on the oracle: pairs on the radius exist, are hits under both rules at R_on and under neither at R_off
    assert len(q) >= 64
    d2s = oracle.pairwise_square(db[i[:64]], kmers[q[:64]])[np.arange(64), np.arange(64)]
    assert np.all(d2s == d2)
    assert np.all(d2s <= radii[0] * radii[0]) and np.all(np.sqrt(d2s) <= radii[0])
    assert not np.any(d2s <= radii[2] * radii[2]) and not np.any(np.sqrt(d2s) <= radii[2])
    pairs = orr.bucket_pairs(oracle, a, b, Wf, db, radii[0])
    where = {row.tobytes(): n for n, row in enumerate(db_codes)}
    ids = [where[row.tobytes()] for row in centres]
    on_edges = {(ids[x], y) for x, y in zip(q.tolist(), i.tolist())}
    return dict(k=c["k"], K=c["K"], L=c["L"], W=Wf, a=a, b=b, table=table, db_codes=db_codes, centres=centres,
                kmers=kmers, radii=radii, want=want, on=set(zip(q.tolist(), i.tolist())), pairs=pairs,
                on_edges=on_edges)


@pytest.mark.parametrize("name", ON_RADIUS)
def test_pairs_on_the_radius_and_just_outside(oracle, name):
    f = build_family(oracle, name)
    eng = Engine(f["k"], f["K"], f["L"], f["W"], f["a"], f["b"], coords=f["table"])
    try:
        eng.index_build(f["db_codes"])
        r_on, _, r_off = f["radii"]
        for r in (r_on, r_off):
            for what, got in (("codes", eng.query_codes(f["centres"], r)), ("k-mer centres", eng.query(f["kmers"], r))):
                _same(got, f["want"][r], (name, what, r))
                have = set(zip(got["q"].tolist(), got["id"].tolist()))
                assert (f["on"] <= have) if r == r_on else not (f["on"] & have), (name, what, r)
            for sq in (False, True):
                got = eng.self_join(r, sqrt_test=sq)
                _same(got, orr.edges_at(f["pairs"], r, sq), (name, "self-join", r, sq), ("i", "j", "table", "dist"))
                have = set(zip(got["i"].tolist(), got["j"].tolist()))
                assert (f["on_edges"] <= have) if r == r_on else not (f["on_edges"] & have), (name, "self-join", r, sq)
    finally:
        eng.close()
