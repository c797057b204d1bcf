"""hs_components_merge (host only, no GPU): the labels of the union of m forests, each given as a label array,
against the plain union-find of tests/components_ref.py -- on random forests, under permutation of the inputs,
merged twice, on invalid inputs and on nothing at all."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hsearch_amd import capi
from tests import components_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stack(seed, n, m):
    rng = np.random.default_rng(seed)
    return np.stack([cr.random_forest(rng, n, p) for p in rng.uniform(0.05, 0.6, m)]) if m else \
        np.empty((0, n), dtype=np.uint32)


@pytest.mark.parametrize("n,m", [(1, 1), (2, 3), (17, 2), (257, 7), (1000, 4), (2000, 1), (2000, 5), (1999, 7)])
def test_merge_equals_reference_rule(n, m):
    stack = _stack(n + m, n, m)
    want = cr.merge_labels(stack)
    got = capi.components_merge(stack)
    assert got["label"].dtype == np.uint32 and np.array_equal(got["label"], want)
    assert got["n_components"] == cr.n_components(want)
    assert (got["label"] <= np.arange(n)).all()
    if m > 1 and n > 100:  # the merge really joined trees of different inputs
        assert got["n_components"] < min(cr.n_components(s) for s in stack)


def test_order_of_the_inputs_is_irrelevant():
    stack = _stack(3, 1500, 6)
    want = capi.components_merge(stack)
    rng = np.random.default_rng(8)
    for _ in range(5):
        got = capi.components_merge(stack[rng.permutation(len(stack))])
        assert np.array_equal(got["label"], want["label"]) and got["n_components"] == want["n_components"]


def test_idempotent_and_one_input_comes_back():
    stack = _stack(4, 1800, 5)
    once = capi.components_merge(stack)
    for s in stack:  # m = 1 returns its input
        got = capi.components_merge(s[None, :])
        assert np.array_equal(got["label"], s) and got["n_components"] == cr.n_components(s)
    again = capi.components_merge(once["label"][None, :])
    assert np.array_equal(again["label"], once["label"]) and again["n_components"] == once["n_components"]
    # merging the result with its own inputs, or the inputs twice, changes nothing
    for more in (np.concatenate([stack, once["label"][None, :]]), np.concatenate([stack, stack[::-1]])):
        got = capi.components_merge(more)
        assert np.array_equal(got["label"], once["label"]) and got["n_components"] == once["n_components"]
    # in place: the output may be one of the inputs
    work = stack.copy()
    got = capi.components_merge(work, out=work[2])
    assert np.array_equal(work[2], once["label"]) and got["n_components"] == once["n_components"]


def test_invalid_inputs_leave_the_output_untouched():
    stack = _stack(5, 600, 3)
    sentinel = 0xdeadbeef
    # label[i] > i
    bad = stack.copy()
    bad[1, 40] = 41
    # label[label[i]] != label[i]: a label that is not a root (a forest deeper than one level)
    deep = stack.copy()
    i = int(np.nonzero(deep[2] != np.arange(600))[0][0])       # a vertex that is not a root ...
    j = int(np.nonzero(np.arange(600) > i)[0][0])
    deep[2, j] = i                                              # ... named as the label of a later one
    assert deep[2, deep[2, j]] != deep[2, j] and deep[2, j] <= j
    for case in (bad, deep, bad[1:2], deep[::-1]):
        out = np.full(600, sentinel, dtype=np.uint32)
        with pytest.raises(capi.HsError) as e:
            capi.components_merge(case, out=out)
        assert e.value.status == capi.HS_ERR_INVALID
        assert (out == sentinel).all()
        nc = C.c_uint64(99)
        st = capi.load().hs_components_merge(capi._vp(np.ascontiguousarray(case)), len(case), 600, capi._vp(out), C.byref(nc))
        assert st == capi.HS_ERR_INVALID and nc.value == 0 and (out == sentinel).all()
    # null pointers where something is announced
    nc = C.c_uint64(0)
    lib = capi.load()
    assert lib.hs_components_merge(None, 2, 600, capi._vp(np.empty(600, dtype=np.uint32)), C.byref(nc)) == capi.HS_ERR_INVALID
    assert lib.hs_components_merge(capi._vp(stack), 3, 600, None, C.byref(nc)) == capi.HS_ERR_INVALID
    assert lib.hs_components_merge(capi._vp(stack), 3, 600, capi._vp(np.empty(600, dtype=np.uint32)), None) == capi.HS_ERR_INVALID


def test_nothing_to_merge():
    for m in (0, 1, 4):  # n = 0
        got = capi.components_merge(np.empty((m, 0), dtype=np.uint32))
        assert len(got["label"]) == 0 and got["n_components"] == 0
    nc = C.c_uint64(7)
    assert capi.load().hs_components_merge(None, 0, 0, None, C.byref(nc)) == capi.HS_OK and nc.value == 0
    got = capi.components_merge(np.empty((0, 9), dtype=np.uint32))  # m = 0: every vertex by itself
    assert np.array_equal(got["label"], np.arange(9)) and got["n_components"] == 9


def test_header_declares_and_library_exports():
    import hsearch_amd
    text = open(os.path.join(ROOT, "include", "hsearch.h")).read()
    lib = capi.load()
    for name in ("hs_components", "hs_components_dev", "hs_components_range", "hs_components_range_dev",
                 "hs_components_merge"):
        assert re.search(r"HS_API\s+hs_status\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
    assert hsearch_amd.components_merge is capi.components_merge
    for name in ("components", "components_dev"):
        assert callable(getattr(capi.Engine, name))
