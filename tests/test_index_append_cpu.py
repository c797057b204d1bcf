"""hs_index_table_append on the host (no GPU): one table merged with the bucket ints of an appended block must
equal, array for array, the table built over the concatenation (tests/indexfile.build_tables of the oracle's
bucket ints) -- the rule hs_index_append applies on the device."""
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
    """A (400 k-mers) and three kinds of further k-mers hashed once, all together: mutated copies of A's (many
    land in A's buckets), copies of A's, and unrelated ones (new buckets)."""
    k, K, L, W = 9, 3, 3, 12.0
    a, b = synth.make_planes(k, K, L, W, seed=3)
    A = synth.make_db(400, k, seed=4)
    near, _ = synth.make_query_codes(A, 300, max_subst=2, seed=5)
    far = synth.make_db(200, k, seed=6)
    codes = np.concatenate([A, near, A[:150], far])
    ints = oracle.hash_all(a, b, W, oracle.embed_codes(codes))
    nA = len(A)
    return dict(K=K, L=L, A=ints[:nA], near=ints[nA:nA + 300], dup=ints[nA + 300:nA + 450], far=ints[nA + 450:])


def _append(tables, block):
    return [capi.index_table_append(*t, block[:, l], seed=SEED) for l, t in enumerate(tables)]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g is not None
        for x, y in zip(g, w):
            assert x.dtype == y.dtype and np.array_equal(x, y.reshape(x.shape))


def _check(A, B):
    got = _append(indexfile.build_tables(A, SEED), B)
    _same(got, indexfile.build_tables(np.concatenate([A, B]), SEED))
    return got


def test_mutated_copies_and_new_kmers(db):
    got = _check(db["A"], np.concatenate([db["near"], db["far"]]))
    old = indexfile.build_tables(db["A"], SEED)
    # the case means something: some block k-mers joined old buckets, some made new ones
    assert all(len(old[l][1]) < len(got[l][1]) < len(old[l][1]) + 500 for l in range(db["L"]))


def test_empty_block(db):
    _check(db["A"], db["A"][:0])


def test_empty_table(db):
    _check(db["A"][:0], db["near"])


def test_block_of_duplicates_makes_no_bucket(db):
    got = _check(db["A"], db["dup"])
    old = indexfile.build_tables(db["A"], SEED)
    assert [len(t[1]) for t in got] == [len(t[1]) for t in old]


def test_block_of_new_buckets_below_and_above_every_old_fingerprint(db):
    K, l = db["K"], 0
    old_keys = {int(x) for x in indexfile.build_tables(db["A"], SEED)[l][1]}
    lo, hi = min(old_keys), max(old_keys)
    # tuples far from A's, until one fingerprint lies below A's smallest and one above its largest
    block, below, above = [], False, False
    for v in range(1000, 200000):
        t = np.array([v, -v, 7], dtype=np.int32)
        f = capi.key_fingerprint(t, SEED)
        if f in old_keys:
            continue
        if f < lo and not below:
            below = True
            block.append(t)
        elif f > hi and not above:
            above = True
            block.append(t)
        elif len(block) < 40:
            block.append(t)
        if below and above and len(block) >= 40:
            break
    assert below and above
    B = np.repeat(np.array(block, dtype=np.int32)[:, None, :], db["L"], axis=1)
    got = _check(db["A"], B)
    assert len(got[l][1]) == len(old_keys) + len(block)


def test_three_appends_equal_one_build(db):
    parts = [db["near"][:100], db["far"][:77], db["near"][100:]]
    tables = indexfile.build_tables(db["A"], SEED)
    for p in parts:
        tables = _append(tables, p)
    _same(tables, indexfile.build_tables(np.concatenate([db["A"]] + parts), SEED))


def test_forged_collision_writes_nothing(db):
    K = db["K"]
    ids, key, start, tup = indexfile.build_tables(db["A"], SEED)[0]
    t = np.array([[31337, -5, 12]], dtype=np.int32)
    f = capi.key_fingerprint(t[0], SEED)
    r = int(np.searchsorted(key, np.uint64(f)))
    key = key.copy()
    key[min(r, len(key) - 1)] = f   # an old bucket now carries the block tuple's fingerprint, under other ints
    assert np.all(key[1:] > key[:-1])
    out = (np.full(len(ids) + 1, 0xabababab, dtype=np.uint32), np.full(len(key) + 1, 0xabababab, dtype=np.uint64),
           np.full(len(key) + 2, 0xabababab, dtype=np.uint32), np.full((len(key) + 1, K), 0x2b2b2b2b, dtype=np.int32))
    before = [x.copy() for x in out]
    assert capi.index_table_append(ids, key, start, tup, t, seed=SEED, out=out) is None
    for x, y in zip(out, before):
        assert np.array_equal(x, y)
    # ... and inside the block: two tuples cannot be forged to share a fingerprint, but the same block against the
    # untouched table merges
    assert capi.index_table_append(*indexfile.build_tables(db["A"], SEED)[0], t, seed=SEED) is not None


def test_invalid_table_is_refused(db):
    ids, key, start, tup = indexfile.build_tables(db["A"], SEED)[0]
    B = db["near"][:10, 0]

    def refused(**kw):
        arrs = dict(ids=ids.copy(), key=key.copy(), start=start.copy(), tup=tup.copy())
        for name, edit in kw.items():
            edit(arrs[name])
        with pytest.raises(HsError) as e:
            capi.index_table_append(arrs["ids"], arrs["key"], arrs["start"], arrs["tup"], B, seed=SEED)
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


def test_capacity_follows_the_two_call_pattern(db):
    ids, key, start, tup = indexfile.build_tables(db["A"], SEED)[0]
    B = db["far"][:50, 0]
    want = indexfile.build_tables(np.concatenate([db["A"], db["far"][:50]]), SEED)[0]
    small = (np.zeros(len(ids) + 50, dtype=np.uint32), np.zeros(len(want[1]) - 1, dtype=np.uint64),
             np.zeros(len(want[1]), dtype=np.uint32), np.zeros((len(want[1]) - 1, db["K"]), dtype=np.int32))
    with pytest.raises(HsError) as e:
        capi.index_table_append(ids, key, start, tup, B, seed=SEED, out=small)
    assert e.value.status == capi.HS_ERR_CAPACITY
    assert not any(x.any() for x in small)


def test_host_merge_under_asan_and_ubsan(tmp_path):
    """The host function with a stand-alone main (tests/index_table_append_san.cpp), compiled and run under
    AddressSanitizer + UndefinedBehaviorSanitizer with the host programs' sanitizer flags (the runtimes linked statically: the program
    does not depend on what else the process preloads); nothing is loaded into python."""
    exe = tmp_path / "index_table_append_san"
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-o", str(exe),
                    os.path.join(ROOT, "tests", "index_table_append_san.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "index_table_append_san ok" in res.stdout
