"""hs_recognise_kmers_kernel finds a group's candidate row from its first coordinate alone and compares the other
seven doubles with that one row; a table in which rows share a first coordinate takes the full scan for such a
group.  Same codes, same count of unrecognised groups as the scan of every row: centres that are k-mers run from
their codes (`queries_recognised` == nq) and give the oracle's answer, and ONE double moved by one ulp -- in the
first coordinate or in a later one, in the first group of the first query or in the last group of the last -- keeps
the whole call on the points path, with the oracle's answer for the moved centres.

Tables: the built-in one (all first coordinates distinct) and one of 24 letters in which rows 5 and 9 share their
first coordinate, rows 11 and 12 their first three, and rows 3 and 7 are equal (the first such row is the code; the
results cannot tell them apart).  The small world of tests/test_gpu_probe_ranks.py, smaller: 5000 k-mers."""
import numpy as np
import pytest

from hsearch_amd import Engine, synth
from tests import onradius_ref as orr

pytestmark = pytest.mark.gpu

K_MER, K, L, W, R, N_DB, NQ = 25, 4, 4, 300.0, 40.0, 5000, 130
_FIELDS = ("q", "id", "table", "dist", "cand")


def _shared_table():
    t = np.random.default_rng(2424).normal(0.0, float(synth.coords().std()), size=(24, 8))
    t = np.array([[float("%g" % v) for v in row] for row in t])
    t[9, 0] = t[5, 0]
    t[12, :3] = t[11, :3]
    t[7] = t[3]
    return t


@pytest.fixture(scope="module", params=["built-in", "shared"])
def world(request, oracle):
    table = None if request.param == "built-in" else _shared_table()
    alpha = 20 if table is None else len(table)
    rng = np.random.Generator(np.random.MT19937(515 + alpha))
    a, b = synth.make_planes(K_MER, K, L, W)
    codes = rng.integers(0, alpha, size=(N_DB, K_MER), dtype=np.uint8)
    q_codes = codes[rng.integers(0, N_DB, NQ)].copy()
    q_codes[np.arange(NQ), rng.integers(0, K_MER, NQ)] = rng.integers(0, alpha, NQ, dtype=np.uint8)
    if table is not None:  # every special row at the places the moved doubles sit in, and all over the queries
        q_codes[0, 0], q_codes[-1, -1] = 9, 12
        q_codes[1:9, 3] = [3, 5, 7, 9, 11, 12, 7, 3]
    db = orr.embed(oracle, codes, table)
    pts = orr.embed(oracle, q_codes, table)
    ix = oracle.Index(a, b, W, db)
    want = ix.query(pts, R)
    assert len(np.unique(want["table"])) > 1
    eng = Engine(K_MER, K, L, W, a, b, coords=table)
    eng.index_build(codes)
    yield dict(eng=eng, ix=ix, pts=pts, q_codes=q_codes, want=want)
    eng.close()
    ix.close()


def _same(got, want, what):
    for f in _FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)


def test_kmer_centres_are_recognised(world):
    eng = world["eng"]
    got = eng.query(world["pts"], R)
    assert eng.profile()["queries_recognised"] == NQ
    _same(got, world["want"], "k-mer centres")
    _same(eng.query_codes(world["q_codes"], R), world["want"], "codes")


@pytest.mark.parametrize("row,col", [(0, 0), (0, 5), (NQ - 1, 8 * K_MER - 8), (NQ - 1, 8 * K_MER - 1), (NQ // 2, 8 * 7 + 2)])
def test_one_double_moved_by_one_ulp(world, row, col):
    eng = world["eng"]
    moved = world["pts"].copy()
    moved[row, col] = np.nextafter(moved[row, col], np.inf)
    want = world["ix"].query(moved, R)
    got = eng.query(moved, R)
    assert eng.profile()["queries_recognised"] == 0
    _same(got, want, ("moved", row, col))
    # ... and the k-mers themselves are recognised again in the next call
    got = eng.query(world["pts"], R)
    assert eng.profile()["queries_recognised"] == NQ
    _same(got, world["want"], "k-mer centres after moved ones")
