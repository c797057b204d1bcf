"""The two forms of the FP6 join (HS_OPT_JOIN_F6_FORM): hs_join6x_kernel on work items of 128 members and
hs_join6w_kernel on items of 192, at every item boundary of both.

One small index per k-mer length is built whose buckets and query segments have chosen sizes (the construction of
tests/test_gpu_join8x_issue.py, restated for twelve buckets):

  members per bucket   1, 127, 128, 129, 191, 192, 193, 511, 512, 513, 700, 1025 -- both sides of 128, 192 (an item
                       of either form), 384 = 3 x 128 = 2 x 192 lies inside 511, 512 (four items of 128) and 576 / 1024
                       (items of 192 / 128) inside 700 and 1025;
  queries per segment  65, 95, 96, 97, 128, 193 -- last tiles of 1, 31 and 32 rows, an odd and an even number of tiles
                       (the 192-member kernel walks them in groups of two), more than one group; a segment of at most
                       64 queries is hs_join8r_kernel's and none is built here.

A segment's queries are k-mers of the bucket that are not in the database (random 25-mers lie more than 50 apart:
near nothing), except those planted: a copy, or a copy with one substitution where that stays in the bucket, of the
member in slot 0, 63, 64, 127, 128, 191, 192, 255, 256, 383, 384, 511, 512, 575, 576, 699, 1023, 1024 and the last
one -- the first and last row of every item and accumulator set of both forms.  The bucket of 193 members is queried
with its own 193 members: a survivor in every row, register, lane quarter and column of its items (192 + 1 members in
form 1: the 12-row-tile body and the 8-row-tile body).

Expected: the oracle's candidates and hits, element for element, from both forms, at R = 40 and R = 0 (the copies
alone), with per-query radii, with items dealt in XCD runs and chunks of 3, at k = 25 and k = 21; and
`join_f6_wide_items` > 0 exactly where form 1 ran; and the batch whose FP6 member records find no room, which the
int8 kernel takes on its own items.  Without a GPU the construction is checked on the oracle."""
import numpy as np
import pytest

from hsearch_amd import Engine, synth

KK, L, W, N_POOL = 3, 2, 100.0, 60000
R = 40.0
# (members, queries); queries None: the bucket's own members
BUCKETS = [(1, 97), (127, 65), (128, 96), (129, 95), (191, 128), (192, 97), (193, None), (511, 65), (512, 95),
           (513, 96), (700, 128), (1025, 193)]
SLOTS = (0, 63, 64, 127, 128, 191, 192, 255, 256, 383, 384, 511, 512, 575, 576, 699, 1023, 1024)
_CASES = {}


def _bucket_ids(ints, table):
    _, inv = np.unique(ints[:, table, :], axis=0, return_inverse=True)
    return inv.ravel()


def _case(oracle, k):
    if k in _CASES:
        return _CASES[k]
    rng = np.random.default_rng(9100 + k)
    a, b = synth.make_planes(k, KK, L, W, seed=9200 + k)
    pool = synth.make_db(N_POOL, k, seed=9300 + k)

    def key0(c):
        c = np.ascontiguousarray(np.atleast_2d(c), dtype=np.uint8)
        return oracle.hash_all(a, b, W, oracle.embed_codes(c))[:, 0, :]

    pool_b = _bucket_ids(oracle.hash_all(a, b, W, oracle.embed_codes(pool)), 0)
    sizes = np.bincount(pool_b)
    by_size = np.argsort(sizes, kind="stable")
    need = sorted(range(len(BUCKETS)), key=lambda i: BUCKETS[i][0] + (BUCKETS[i][1] or 0))
    target, used = {}, set()
    for i in need:
        m, nq = BUCKETS[i]
        g = next(int(g) for g in by_size if int(g) not in used and sizes[g] >= m + (nq or 0) + 8)
        used.add(g)
        target[i] = g
    keep = np.ones(N_POOL, dtype=bool)
    spare = {}
    for i, g in target.items():
        ids = np.flatnonzero(pool_b == g)
        keep[ids[BUCKETS[i][0]:]] = False
        spare[i] = pool[ids[BUCKETS[i][0]:]]
    for g in range(len(sizes)):        # (big buckets of the pool would only cost time)
        if g not in used:
            keep[np.flatnonzero(pool_b == g)[1500:]] = False
    codes = np.ascontiguousarray(pool[keep])
    members = {i: np.flatnonzero(pool_b[keep] == g) for i, g in target.items()}
    queries, owner, planted = [], [], []
    for i, (m, nq) in enumerate(BUCKETS):
        bkey = key0(codes[members[i][0]])[0]
        if nq is None:
            for mid in members[i]:
                queries.append(codes[mid].copy())
                owner.append(i)
                planted.append((len(queries) - 1, int(mid)))
            continue
        slots = sorted({s for s in SLOTS if s < m} | {m - 1})[:nq]
        for j, s in enumerate(slots):
            mid = int(members[i][s])
            y = codes[mid].copy()
            if j % 2:       # one substitution, where that stays in the bucket (a copy otherwise)
                for _ in range(50):
                    z = y.copy()
                    p = rng.integers(k)
                    z[p] = (z[p] + rng.integers(1, 20)) % 20
                    if (key0(z)[0] == bkey).all():
                        y = z
                        break
            queries.append(y)
            owner.append(i)
            planted.append((len(queries) - 1, mid))
        for q in spare[i][:nq - len(slots)]:
            queries.append(q)
            owner.append(i)
    order = rng.permutation(len(queries))
    qcodes = np.ascontiguousarray(np.array(queries, dtype=np.uint8)[order])
    new_index = np.argsort(order)
    owner = [owner[j] for j in order]
    planted = [(int(new_index[q]), mid) for q, mid in planted]

    # ---- on the oracle alone: the sizes, and every planted pair a hit
    pts, cpts = oracle.embed_codes(codes), oracle.embed_codes(qcodes)
    all_b = _bucket_ids(oracle.hash_all(a, b, W, np.concatenate([pts, cpts])), 0)
    db_b, q_b = all_b[:len(codes)], all_b[len(codes):]
    ix = oracle.Index(a, b, W, pts)
    want, want0 = ix.query(cpts, R), ix.query(cpts, 0.0)
    ix.close()
    for i, (m, nq) in enumerate(BUCKETS):
        g = db_b[members[i][0]]
        assert (db_b == g).sum() == m, (i, "members")
        qs = np.flatnonzero(q_b == g)
        assert len(qs) == (nq or m) and all(owner[q] == i for q in qs), (i, "queries")
    hits = set(zip(want["q"].tolist(), want["id"].tolist()))
    assert all(p in hits for p in planted)
    hits0 = set(zip(want0["q"].tolist(), want0["id"].tolist()))
    assert len(hits0) >= 193 and hits0 <= hits and len(hits0) < len(hits)
    _CASES[k] = dict(codes=codes, qcodes=qcodes, a=a, b=b, want=want, want0=want0, planted=planted)
    return _CASES[k]


def _assert_equal(got, want, what):
    assert np.array_equal(got["cand"], want["cand"]), what
    for f in ("q", "id", "table", "dist"):
        assert np.array_equal(got[f], want[f]), (what, f)


def _engine(c, k, form, **opts):
    opts = dict(dict(join_resident=1, join_f6=1, join_f6_form=form), **opts)      # (every segment streamed)
    eng = Engine(k, KK, L, W, c["a"], c["b"], options=opts)
    eng.index_build(c["codes"])
    eng.set_verify_mode("join")
    return eng


@pytest.mark.parametrize("k", [25, 21])
def test_construction_holds_on_the_oracle(oracle, k):
    """No GPU: bucket and segment sizes, every planted pair a hit (asserted in _case)."""
    c = _case(oracle, k)
    assert len(c["qcodes"]) == sum(nq or m for m, nq in BUCKETS)
    assert len(c["planted"]) >= 193 + 12


@pytest.mark.gpu
@pytest.mark.parametrize("k", [25, 21])
@pytest.mark.parametrize("routing", ["default", "xcd_runs"])
def test_both_forms_equal_the_oracle(oracle, k, routing):
    c = _case(oracle, k)
    opts = dict() if routing == "default" else dict(join_xcd_run=2, join_chunk=3)
    got = {}
    for form in (0, 1, -1):
        eng = _engine(c, k, form, **opts)
        for Rq, want in ((R, c["want"]), (0.0, c["want0"])):
            got[form, Rq] = eng.query_codes(c["qcodes"], Rq)
            _assert_equal(got[form, Rq], want, (k, routing, form, Rq))
            p = eng.profile()
            # all items are the streaming kernel's, of 192 members unless the form is 0
            assert p["join_f6_batches"] > 0 and p["join_items_resident"] == 0, p
            assert p["join_f6_wide_items"] == (0 if form == 0 else p["join_items"]), p
        got[form, "items"] = p["join_items"]
        eng.close()
    for Rq in (R, 0.0):
        _assert_equal(got[1, Rq], got[0, Rq], (k, routing, "form 1 against form 0", Rq))
    # a segment of m members is ceil(m / 128) items in form 0 and ceil(m / 192) in form 1 (one query group each):
    # the planted buckets alone make this difference, the table-1 segments of the same queries can only add to it
    n128 = sum(-(-m // 128) for m, _ in BUCKETS)
    n192 = sum(-(-m // 192) for m, _ in BUCKETS)
    assert got[-1, "items"] == got[1, "items"] <= got[0, "items"] - (n128 - n192), [got[f, "items"] for f in (0, 1, -1)]


@pytest.mark.gpu
def test_resident_class_keeps_its_items(oracle):
    """With the query-resident kernel on (segments of at most 64 queries are its class; none here) and with the FP6
    join off, the plan is the old one: no item of 192 members."""
    c = _case(oracle, 25)
    eng = _engine(c, 25, 1, join_resident=2)
    _assert_equal(eng.query_codes(c["qcodes"], R), c["want"], "join_resident=2")
    p = eng.profile()
    assert p["join_f6_wide_items"] == p["join_items"] - p["join_items_resident"] > 0, p
    eng.close()
    eng = _engine(c, 25, 1, join_f6=0)
    _assert_equal(eng.query_codes(c["qcodes"], R), c["want"], "join_f6=0")
    p = eng.profile()
    assert p["join_f6_wide_items"] == 0 and p["join_f6_batches"] == 0, p
    eng.close()


@pytest.mark.gpu
def test_no_room_for_the_member_records(oracle, monkeypatch):
    """The FP6 member records find no room (the library's TEST build reports that: HS_TEST_REC6_NO_ROOM) after the
    batch was planned on the FP6 join: the int8 kernel takes it, on items of ITS size -- cut at 192 members it would
    never join members 128..191 of an item and lose their hits without an error.  The batch after it plans the int8
    join from the start."""
    c = _case(oracle, 25)
    monkeypatch.setenv("HS_TEST_REC6_NO_ROOM", "1")
    eng = Engine(25, KK, L, W, c["a"], c["b"], hooks=True, options=dict(join_resident=1, join_f6=1, join_f6_form=1))
    eng.index_build(c["codes"])
    eng.set_verify_mode("join")
    for call in range(2):
        _assert_equal(eng.query_codes(c["qcodes"], R), c["want"], ("no room", call))
        p = eng.profile()
        assert p["join_i8_batches"] > 0 and p["join_f6_batches"] == 0 and p["join_f6_wide_items"] == 0, (call, p)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1])
def test_per_query_radii(oracle, form):
    """Even queries at R, odd ones at 0: every query's own threshold C in its column of the tile."""
    k = 25
    c = _case(oracle, k)
    nq = len(c["qcodes"])
    parts = [{f: w[f][(w["q"] % 2) == r] for f in ("q", "id", "table", "dist")}
             for r, w in enumerate((c["want"], c["want0"]))]
    order = np.argsort(np.concatenate([p["q"] for p in parts]), kind="stable")
    want = {f: np.concatenate([p[f] for p in parts])[order] for f in ("q", "id", "table", "dist")}
    want["cand"] = c["want"]["cand"]
    eng = _engine(c, k, form, wide_rows=2)      # (4-column rows whatever the radius)
    got = eng.query_radii(c["qcodes"], np.where(np.arange(nq) % 2 == 0, R, 0.0), codes=True)
    p = eng.profile()
    assert p["join_f6_batches"] > 0 and (p["join_f6_wide_items"] > 0) == (form == 1), p
    _assert_equal(got, want, ("parity radii", form))
    eng.close()
