"""hs_index_table_remove on the host (no GPU): one table without a set of its ids must equal, array for array, the
table built over the surviving rows (tests/indexfile.build_tables of the oracle's bucket ints) -- the rule
hs_index_remove applies on the device."""
import os
import subprocess

import numpy as np
import pytest

import hsearch_amd
from hsearch_amd import HsError, capi, synth

import indexfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0


@pytest.fixture(scope="module")
def db(oracle):
    """400 k-mers, mutated copies of them (many share their buckets) and copies: hashed once, all together."""
    k, K, L, W = 9, 3, 3, 12.0
    a, b = synth.make_planes(k, K, L, W, seed=3)
    A = synth.make_db(400, k, seed=4)
    near, _ = synth.make_query_codes(A, 300, max_subst=2, seed=5)
    codes = np.concatenate([A, near, A[:150]])
    ints = oracle.hash_all(a, b, W, oracle.embed_codes(codes))
    return dict(K=K, L=L, ints=ints, tables=indexfile.build_tables(ints, SEED))


def _remove(tables, dead, ints):
    return [capi.index_table_remove(*t, dead, None if ints is None else ints[:, l], seed=SEED)
            for l, t in enumerate(tables)]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for x, y in zip(g, w):
            assert x.dtype == y.dtype and np.array_equal(x, y.reshape(x.shape))


def _survivors(n, dead):
    keep = np.ones(n, dtype=bool)
    keep[np.asarray(dead, dtype=np.int64)] = False
    return keep


def _check(ints, tables, dead):
    got = _remove(tables, dead, ints)
    _same(got, indexfile.build_tables(ints[_survivors(len(ints), dead)], SEED))
    return got


def test_random_removals(db):
    rng = np.random.default_rng(1)
    n = len(db["ints"])
    for m in (1, 63, 64, 65, 400, n - 1):
        got = _check(db["ints"], db["tables"], rng.choice(n, size=m, replace=False))
        if m == 400:    # the case means something: buckets vanished, and others lost members but stayed
            assert all(len(got[l][1]) < len(db["tables"][l][1]) for l in range(db["L"]))
            assert all(len(got[l][1]) > n - 400 - 300 for l in range(db["L"]))


def test_empty_removal(db):
    _same(_check(db["ints"], db["tables"], np.zeros(0, dtype=np.uint32)), db["tables"])
    _same(_remove(db["tables"], np.zeros(0, dtype=np.uint32), None), db["tables"])     # no ints needed


def test_everything_removed(db):
    n = len(db["ints"])
    got = _check(db["ints"], db["tables"], np.arange(n))
    for ids, key, start, tup in got:
        assert len(ids) == 0 and len(key) == 0 and list(start) == [0] and tup.shape == (0, db["K"])


def test_a_bucket_emptied_and_one_beheaded(db):
    ids, key, start, tup = db["tables"][0]
    sizes = np.diff(start.astype(np.int64))
    big = int(np.argmax(sizes))
    assert sizes[big] >= 3
    members = ids[start[big]:start[big + 1]]
    got = _check(db["ints"], db["tables"], members)                 # the whole bucket goes
    assert len(got[0][1]) == len(key) - 1 and int(key[big]) not in set(got[0][1].tolist())
    got = _check(db["ints"], db["tables"], members[:-1])            # its last member stays, alone
    at = int(np.searchsorted(got[0][1], key[big]))
    assert got[0][1][at] == key[big] and got[0][2][at + 1] - got[0][2][at] == 1


def test_duplicates_in_the_id_list(db):
    rng = np.random.default_rng(2)
    dead = rng.choice(len(db["ints"]), size=200, replace=False)
    twice = np.concatenate([dead, dead[::-1], dead[:17]])
    _same(_remove(db["tables"], twice, db["ints"]), _remove(db["tables"], dead, db["ints"]))
    _check(db["ints"], db["tables"], twice)


def test_id_outside_the_table_is_refused(db):
    n = len(db["ints"])
    for bad in (n, n + 1, 0xffffffff):
        with pytest.raises(HsError) as e:
            capi.index_table_remove(*db["tables"][0], np.array([3, bad, 5], dtype=np.uint32), db["ints"][:, 0], seed=SEED)
        assert e.value.status == capi.HS_ERR_INVALID


def test_capacity_follows_the_two_call_pattern(db):
    ids, key, start, tup = db["tables"][0]
    dead = np.arange(0, len(ids), 7)
    want = indexfile.build_tables(db["ints"][_survivors(len(ids), dead)], SEED)[0]
    small = (np.zeros(len(ids), dtype=np.uint32), np.zeros(len(want[1]) - 1, dtype=np.uint64),
             np.zeros(len(want[1]), dtype=np.uint32), np.zeros((len(want[1]) - 1, db["K"]), dtype=np.int32))
    with pytest.raises(HsError) as e:
        capi.index_table_remove(ids, key, start, tup, dead, db["ints"][:, 0], seed=SEED, out=small)
    assert e.value.status == capi.HS_ERR_CAPACITY
    assert not any(x.any() for x in small)
    exact = (np.zeros(len(want[0]), dtype=np.uint32), np.zeros(len(want[1]), dtype=np.uint64),
             np.zeros(len(want[1]) + 1, dtype=np.uint32), np.zeros((len(want[1]), db["K"]), dtype=np.int32))
    _same([capi.index_table_remove(ids, key, start, tup, dead, db["ints"][:, 0], seed=SEED, out=exact)], [want])


def test_invalid_table_is_refused(db):
    ids, key, start, tup = db["tables"][0]
    dead = np.arange(10, dtype=np.uint32)

    def refused(**kw):
        arrs = dict(ids=ids.copy(), key=key.copy(), start=start.copy(), tup=tup.copy())
        for name, edit in kw.items():
            edit(arrs[name])
        with pytest.raises(HsError) as e:
            capi.index_table_remove(arrs["ids"], arrs["key"], arrs["start"], arrs["tup"], dead, db["ints"][:, 0], seed=SEED)
        assert e.value.status == capi.HS_ERR_INVALID

    def twice(x): x[1] = x[0]
    def out_of_range(x): x[5] = len(ids)
    def boundary(x): x[1] = x[0]
    def last_boundary(x): x[-1] -= 1
    def key_order(x): x[[0, 1]] = x[[1, 0]]
    def other_tuple(x): x[0, 0] += 1
    refused(ids=twice)
    refused(ids=out_of_range)
    refused(start=boundary)
    refused(start=last_boundary)
    refused(key=key_order)
    refused(tup=other_tuple)
    big = next(b for b in range(len(key)) if start[b + 1] - start[b] >= 2)

    def id_order(x): x[[start[big], start[big] + 1]] = x[[start[big] + 1, start[big]]]
    refused(ids=id_order)


def test_remove_of_an_appended_block_gives_the_table_back(db):
    ints = db["ints"]
    nA = 400
    T = indexfile.build_tables(ints[:nA], SEED)
    grown = [capi.index_table_append(*t, ints[nA:, l], seed=SEED) for l, t in enumerate(T)]
    _same(grown, db["tables"])
    _same(_remove(grown, np.arange(nA, len(ints)), ints), T)


def test_aliased_first_members(oracle):
    """K = 2 at W = 1: members of one bucket share the HashKey string, not always the ints ((1,23) and (12,3)).  The
    first member of every bucket whose second member carries other ints is removed: the bucket's tuple must become the
    second member's.  (Counted with the oracle: 87 such buckets in table 0 and 93 in table 1.)"""
    k, K, L, W = 25, 2, 2, 1.0
    a, b = synth.make_planes(k, K, L, W, seed=99)
    codes = synth.make_db(8000, k, seed=8)
    ints = oracle.hash_all(a, b, W, oracle.embed_codes(codes))
    tables = indexfile.build_tables(ints, SEED)
    dead, found = [], []
    for l, (ids, key, start, tup) in enumerate(tables):
        two = np.nonzero(np.diff(start.astype(np.int64)) >= 2)[0]
        first, second = ids[start[two]], ids[start[two] + 1]
        other = np.any(ints[first, l] != ints[second, l], axis=1)
        found.append(int(other.sum()))
        dead.append(first[other])
    assert all(f > 0 for f in found), found
    dead = np.unique(np.concatenate(dead))
    got = _check(ints, tables, dead)
    # ... and the tuples did change: copying the old one would not have passed
    for l, (ids, key, start, tup) in enumerate(tables):
        old = {int(f): tuple(t) for f, t in zip(key, tup)}
        changed = sum(1 for f, t in zip(got[l][1], got[l][3]) if old[int(f)] != tuple(t))
        assert changed >= found[l]


def test_host_remove_under_asan_and_ubsan(tmp_path):
    """The host function with a stand-alone main (tests/index_table_remove_san.cpp), compiled and run under
    AddressSanitizer + UndefinedBehaviorSanitizer with the host programs' sanitizer flags (the runtimes linked
    statically: the program does not depend on what else the process preloads); nothing is loaded into python."""
    exe = tmp_path / "index_table_remove_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe),
                    os.path.join(ROOT, "tests", "index_table_remove_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "index_table_remove_san ok" in res.stdout
