"""hs_merge_best (host only, no GPU): the annotation rule -- per distinct id the hit smallest under
(dist, table, q), rows in ascending id -- against its numpy restatement (tests/annotate_ref.py), on the CPU oracle's
hit lists, on lists built by hand for every level of the tie rule, and through the capacity protocol."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hsearch_amd import capi, synth
from tests import annotate_ref as ar
from tests.test_gpu_multiprobe import _case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _merge(h, **kw):
    return capi.merge_best(h["id"], h["q"], h["table"], h["dist"], **kw)


def _shuffled(h, seed):
    p = np.random.default_rng(seed).permutation(len(h["id"]))
    return {f: np.asarray(h[f])[p] for f in ar.FIELDS}


@pytest.mark.parametrize("k,R", [(15, 30.0), (25, 40.0), (39, 50.0)])
def test_merge_best_equals_rule_on_oracle_hits(oracle, k, R):
    a, b, W, codes, qcodes, centers = _case(k)
    ix = oracle.Index(a, b, W, oracle.embed_codes(codes))
    # duplicated query rows: two centres that are the same k-mer reach every k-mer at identical distances
    dup = np.concatenate([qcodes, qcodes[:60][::-1]])
    lists = [ix.query(centers, R), ix.query(synth.embed(qcodes), R), ix.query(synth.embed(dup), R)]
    ix.close()
    for n_list, hits in enumerate(lists):
        assert len(hits["q"]) > 0
        want = ar.annotate(hits)
        assert 0 < len(want["id"]) <= len(codes)
        ar.assert_same(_merge(hits), want, (k, n_list))
        for seed in (1, 2):  # the input order is irrelevant
            ar.assert_same(_merge(_shuffled(hits, seed)), want, (k, n_list, "shuffled", seed))
        # a concatenation with itself and with another list's tuples: duplicates change nothing
        ar.assert_same(_merge(ar.concat([hits, _shuffled(hits, 3)])), want, (k, n_list, "doubled"))
    both = ar.concat([lists[0], lists[1]])
    ar.assert_same(_merge(both), ar.annotate(both), (k, "two lists"))
    # merging two annotations = annotating the union
    ar.assert_same(_merge(ar.concat([ar.annotate(lists[0]), ar.annotate(lists[1])])), ar.annotate(both), (k, "merge"))
    by_table, by_q = ar.tie_levels(lists[2])
    assert by_q > 0, "the duplicated centres must tie on (dist, table)"


def test_empty_list():
    got = capi.merge_best([], [], [], [])
    assert all(len(got[f]) == 0 for f in ar.FIELDS)
    n_out = C.c_uint64(7)
    st = capi.load().hs_merge_best(None, None, None, None, 0, None, None, None, None, 0, C.byref(n_out))
    assert st == capi.HS_OK and n_out.value == 0


def test_every_level_of_the_tie_rule():
    d = 12.5
    up = np.nextafter(d, np.inf)
    hits = dict(
        id=np.array([9, 9, 4, 4, 4, 7, 7, 2, 2, 2, 30, 30], dtype=np.uint32),
        q=np.array([1, 0, 5, 3, 8, 6, 2, 1, 0, 2, 3, 3], dtype=np.uint32),
        table=np.array([0, 3, 2, 1, 1, 4, 4, 0, 0, 1, 5, 2], dtype=np.uint32),
        dist=np.array([up, d,        # id 9: distances one ulp apart: the smaller wins against table and q
                       d, d, d,      # id 4: equal distance: table 1 beats 2, then q 3 beats 8
                       d, d,         # id 7: equal distance and table: q 2
                       3.0, 3.0, 1.0,  # id 2: the strictly smaller distance at the larger table and q
                       d, d]))       # id 30: the same centre in two tables
    want = dict(id=np.array([2, 4, 7, 9, 30], dtype=np.uint32), q=np.array([2, 3, 2, 0, 3], dtype=np.uint32),
                table=np.array([1, 1, 4, 3, 2], dtype=np.uint32), dist=np.array([1.0, d, d, d, d]))
    ar.assert_same(ar.annotate(hits), want, "the restatement itself")
    ar.assert_same(_merge(hits), want)
    for seed in range(5):
        ar.assert_same(_merge(_shuffled(hits, seed)), want, seed)
    # one ulp the other way round
    hits["dist"][:2] = (d, up)
    want["q"][3], want["table"][3] = 1, 0
    ar.assert_same(_merge(hits), want, "ulp swapped")


def test_capacity_protocol():
    rng = np.random.default_rng(4)
    n = 5000
    hits = dict(id=rng.integers(0, 700, n).astype(np.uint32), q=rng.integers(0, 90, n).astype(np.uint32),
                table=rng.integers(0, 8, n).astype(np.uint32), dist=rng.integers(0, 6, n).astype(np.float64))
    want = ar.annotate(hits)
    need = len(want["id"])
    for cap in (0, need - 1):
        with pytest.raises(capi.HsError) as e:
            _merge(hits, cap=cap)
        assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == need
    ar.assert_same(_merge(hits, cap=need), want)
    # null outputs with room asked for, null inputs with tuples announced
    n_out = C.c_uint64(0)
    lib = capi.load()
    assert lib.hs_merge_best(capi._vp(hits["id"]), capi._vp(hits["q"]), capi._vp(hits["table"]),
                             capi._vp(hits["dist"]), n, None, None, None, None, need, C.byref(n_out)) == capi.HS_ERR_INVALID
    assert lib.hs_merge_best(None, None, None, None, n, None, None, None, None, 0, C.byref(n_out)) == capi.HS_ERR_INVALID


def test_header_declares_and_library_exports():
    text = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in ("hs_annotate", "hs_annotate_dev", "hs_merge_best"):
        assert re.search(r"HS_API\s+hs_status\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
