"""hs_index_append: a handle built over A and grown by B must be indistinguishable from a fresh handle built over
A ++ B -- the file hs_index_save writes byte for byte, hs_index_info_get but device_bytes, and every search hit for
hit with the distance's bits.  Databases are mutated copies of a few hundred random k-mers (synth.make_query_codes),
so that most appended k-mers land in occupied buckets, plus unrelated ones that make new buckets."""
import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth

pytestmark = pytest.mark.gpu

K25 = dict(k=25, K=6, L=3, W=60.0, R=40.0)    # 3000 of _codes: ~ 1400 buckets a table, the largest of ~ 20


def _codes(n, k, seed, base_seed=11):
    """n k-mers: 7 in 8 mutated copies of 1 + n // 6 base k-mers (about five to a bucket), the rest unrelated."""
    if not n:
        return np.zeros((0, k), dtype=np.uint8)
    base = synth.make_db(1 + n // 6, k, seed=base_seed)
    near, _ = synth.make_query_codes(base, n, max_subst=3, seed=seed)
    far = synth.make_db(n, k, seed=seed + 1000)
    pick = np.arange(n) % 8 == 7
    near[pick] = far[pick]
    return near


def _engine(shape, **options):
    a, b = synth.make_planes(shape["k"], shape["K"], shape["L"], shape["W"], seed=3)
    return Engine(shape["k"], shape["K"], shape["L"], shape["W"], a, b, options=options or None)


def _info(eng):
    info = eng.index_info()
    info.pop("device_bytes")
    return info


def _same(x, y, what):
    assert x.keys() == y.keys(), what
    for f in x:
        if isinstance(x[f], np.ndarray):
            assert x[f].dtype == y[f].dtype and x[f].shape == y[f].shape, (what, f)
            assert x[f].tobytes() == y[f].tobytes(), (what, f)      # (bytes: the distances' bits)
        else:
            assert x[f] == y[f], (what, f)


def _searches(eng, all_codes, R, seed=5):
    """code queries, general centres, the self-join"""
    if not len(all_codes):
        return {}
    qc, _ = synth.make_query_codes(all_codes, 200, max_subst=3, seed=seed)
    centers, _ = synth.make_queries(all_codes, 150, max_subst=3, seed=seed + 1, jitter=0.05)
    return dict(codes=eng.query_codes(qc, R), centres=eng.query(centers, R), self_join=eng.self_join(R))


def _assert_equal_handles(grown, fresh, all_codes, R, tmp_path, what):
    assert _info(grown) == _info(fresh), what
    assert _info(grown)["n"] == len(all_codes)
    pg, pf = tmp_path / "grown.hsidx", tmp_path / "fresh.hsidx"
    grown.index_save(pg)
    fresh.index_save(pf)
    assert pg.read_bytes() == pf.read_bytes(), what
    got, want = _searches(grown, all_codes, R), _searches(fresh, all_codes, R)
    for name in want:
        _same(got[name], want[name], (what, name))
    return want


def _grow_and_compare(shape, A, blocks, tmp_path, what, **options):
    grown, fresh = _engine(shape, **options), _engine(shape, **options)
    grown.index_build(A)
    new_buckets = 0
    for B in blocks:
        grown.index_append(B)
        p = grown.profile()
        assert p["append_rebuilds"] == 0, what
        new_buckets += p["append_new_buckets"]
    everything = np.concatenate([A] + list(blocks))
    info = fresh.index_build(everything)
    want = _assert_equal_handles(grown, fresh, everything, shape["R"], tmp_path, what)
    grown.close()
    fresh.close()
    return want, info, new_buckets


@pytest.mark.parametrize("n,m", [(3000, 1), (3000, 63), (3000, 64), (3000, 65), (3000, 5000), (0, 500), (500, 0), (1, 1)])
def test_append_equals_build(n, m, tmp_path):
    k = K25["k"]
    A, B = _codes(n, k, seed=21), _codes(m, k, seed=22)
    want, info, new_buckets = _grow_and_compare(K25, A, [B], tmp_path, (n, m))
    if n == 3000 and m >= 63:
        old = _engine(K25)
        nb_old = old.index_build(A)["n_buckets"]
        old.close()
        # the case means something: the block made new buckets AND filled old ones, and the searches found pairs
        assert new_buckets == sum(info["n_buckets"]) - sum(nb_old)
        assert 0 < new_buckets < m * K25["L"]
        assert len(want["codes"]["q"]) > 100 and len(want["self_join"]["i"]) > 1000


def test_three_appends_equal_one_build(tmp_path):
    k = K25["k"]
    _grow_and_compare(K25, _codes(1000, k, seed=31), [_codes(700, k, seed=32 + i) for i in range(3)], tmp_path, "3 x 700")


def test_block_equal_to_the_index_doubles_every_bucket(tmp_path):
    A = _codes(2000, K25["k"], seed=41)
    _, info, new_buckets = _grow_and_compare(K25, A, [A], tmp_path, "B = A")
    assert new_buckets == 0
    old = _engine(K25)
    before = old.index_build(A)
    old.close()
    assert info["n_buckets"] == before["n_buckets"] and info["max_bucket"] == [2 * x for x in before["max_bucket"]]


def test_one_large_bucket_split_across_index_and_block(tmp_path):
    k = K25["k"]
    one = synth.make_db(1, k, seed=51)
    A = np.concatenate([_codes(300, k, seed=52), np.repeat(one, 1200, axis=0)])
    B = np.concatenate([np.repeat(one, 800, axis=0), _codes(100, k, seed=53)])
    rng = np.random.default_rng(54)
    A, B = A[rng.permutation(len(A))], B[rng.permutation(len(B))]
    shape = dict(K25, R=1.0)    # (the copies alone: 2000 x 1999 pairs per table would be the self-join at R = 40 too)
    _, info, _ = _grow_and_compare(shape, A, [B], tmp_path, "one bucket of 2000")
    assert min(info["max_bucket"]) >= 2000


def test_short_kmers_wide_rows_sorted_grouping(tmp_path):
    shape = dict(k=15, K=6, L=3, W=45.0, R=30.0)
    A, B = _codes(3000, 15, seed=61), _codes(1500, 15, seed=62)
    _grow_and_compare(shape, A, [B], tmp_path, "k = 15", build_grouping=1)


def test_tables_without_directory_records(tmp_path):
    shape = dict(k=25, K=28, L=3, W=250.0, R=40.0)
    A, B = _codes(3000, 25, seed=71), _codes(1500, 25, seed=72)
    want, _, _ = _grow_and_compare(shape, A, [B], tmp_path, "K = 28")
    assert len(want["codes"]["q"]) > 50


def test_loaded_index_grows(tmp_path):
    k = K25["k"]
    A, B = _codes(2500, k, seed=81), _codes(900, k, seed=82)
    saved = tmp_path / "a.hsidx"
    first = _engine(K25)
    first.index_build(A)
    first.index_save(saved)
    first.close()
    grown, fresh = _engine(K25), _engine(K25)
    grown.index_load(saved)
    grown.index_append(B)
    fresh.index_build(np.concatenate([A, B]))
    _assert_equal_handles(grown, fresh, np.concatenate([A, B]), K25["R"], tmp_path, "loaded")
    grown.close()
    fresh.close()


def test_append_dev_equals_append(tmp_path):
    import torch
    k = K25["k"]
    A, B = _codes(2000, k, seed=91), _codes(777, k, seed=92)
    grown, fresh = _engine(K25), _engine(K25)
    grown.index_build(A)
    grown.index_append_dev(torch.from_numpy(B).cuda())
    fresh.index_build(np.concatenate([A, B]))
    _assert_equal_handles(grown, fresh, np.concatenate([A, B]), K25["R"], tmp_path, "_dev")
    grown.close()
    fresh.close()


def test_append_windows_equals_build_windows(tmp_path):
    k = K25["k"]
    rng = np.random.default_rng(101)
    motif = rng.integers(0, 20, size=60, dtype=np.uint8)

    def proteins(lengths):
        seqs = []
        for n in lengths:
            s = rng.integers(0, 20, size=n, dtype=np.uint8)
            if n >= 90:     # a shared stretch: windows of different proteins in one bucket
                s[10:70] = motif
                s[rng.integers(10, 70, size=3)] = rng.integers(0, 20, size=3, dtype=np.uint8)
            seqs.append(s)
        start = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        return np.concatenate(seqs), start

    r1, s1 = proteins([300, 120, 25, 200, 95])
    r2, s2 = proteins([150, 24, 0, 400, 25, 110])           # 24 and 0: shorter than k, no windows
    grown, fresh = _engine(K25), _engine(K25)
    _, pos1 = grown.index_build_windows(r1, s1)
    _, pos2 = grown.index_append_windows(r2, s2)
    both = np.concatenate([r1, r2])
    _, pos = fresh.index_build_windows(both, np.concatenate([s1, s2[1:] + np.uint64(len(r1))]))
    assert len(pos2) == 126 + 376 + 1 + 86
    assert np.array_equal(pos[:len(pos1)], pos1) and np.array_equal(pos[len(pos1):], pos2 + np.uint32(len(r1)))
    windows = np.stack([both[p:p + k] for p in pos])
    _assert_equal_handles(grown, fresh, windows, K25["R"], tmp_path, "windows")
    with pytest.raises(HsError) as e:
        grown.index_append_windows(r2, np.array([0, 200, 100, len(r2)], dtype=np.uint64))
    assert e.value.status == capi.HS_ERR_INVALID
    _assert_equal_handles(grown, fresh, windows, K25["R"], tmp_path, "windows, after a refused call")
    grown.close()
    fresh.close()


def _sinks(eng, codes, R):
    """the calls that leave state sized by n, or built lazily, in a handle"""
    qc, _ = synth.make_query_codes(codes, 300, max_subst=3, seed=7)
    out = dict(codes=eng.query_codes(qc, R))
    assert eng.profile()["join_f6_batches"] > 0        # the FP6 member records exist from here on
    out["annotate"] = eng.annotate(qc, R=R, codes=True)
    out["components"] = eng.components(R)
    out["self_knn"] = eng.self_knn(R, 5)
    out["profile"] = eng.cluster_profile(out["components"]["label"], min_size=2, want_counts=True)
    return out


def test_state_of_the_old_index_does_not_survive(tmp_path):
    k, R = K25["k"], K25["R"]
    A, B = _codes(3000, k, seed=111), _codes(2100, k, seed=112)
    grown, fresh = _engine(K25), _engine(K25)
    for eng in (grown, fresh):
        eng.set_verify_mode("join")
    grown.index_build(A)
    _sinks(grown, A, R)                                # FP6 records, annotation slots, forests ... of 3000 k-mers
    grown.index_append(B)
    everything = np.concatenate([A, B])
    fresh.index_build(everything)
    got, want = _sinks(grown, everything, R), _sinks(fresh, everything, R)
    for name in want:
        _same(got[name], want[name], name)
    assert len(want["annotate"]["id"]) > 100 and want["components"]["n_edges"] > 1000
    grown.close()
    fresh.close()


def test_refused_calls_leave_the_index_alone():
    k, R = K25["k"], K25["R"]
    A = _codes(2000, k, seed=121)
    qc, _ = synth.make_query_codes(A, 200, max_subst=3, seed=8)
    eng = _engine(K25)
    with pytest.raises(HsError) as e:
        eng.index_append(A[:10])
    assert e.value.status == capi.HS_ERR_STATE          # unbuilt
    info = eng.index_build(A)
    before = eng.query_codes(qc, R)

    def refused(call, status):
        with pytest.raises(HsError) as e:
            call()
        assert e.value.status == status
        assert eng.index_info() == info
        _same(eng.query_codes(qc, R), before, status)

    bad = _codes(100, k, seed=122)
    bad[57, 3] = 20                                     # one code outside the alphabet
    refused(lambda: eng.index_append(bad), capi.HS_ERR_INVALID)
    import torch
    refused(lambda: eng.index_append_dev(torch.from_numpy(bad).cuda()), capi.HS_ERR_INVALID)
    # n + m too large: from the arguments alone (the pointer is never read, nothing of that size is allocated)
    lib, one = capi.load(), np.zeros((1, k), dtype=np.uint8)
    for m in ((1 << 31) - 2000, (1 << 31), (1 << 40)):
        refused(lambda: eng._check(lib.hs_index_append(eng._h, one.ctypes.data, m)), capi.HS_ERR_INVALID)
        refused(lambda: eng._check(lib.hs_index_append_dev(eng._h, one.ctypes.data, m)), capi.HS_ERR_INVALID)
    eng.index_append(_codes(100, k, seed=122))          # ... and the handle still grows
    assert eng.index_info()["n"] == 2100
    eng.close()


def test_forced_collision_rebuilds(monkeypatch, tmp_path):
    """The test build's HS_TEST_APPEND_COLLISION: the match step of the last table reports one fingerprint under two
    HashKey strings; the call then runs the build loop over the concatenated codes and ends with the same index."""
    k = K25["k"]
    A, B = _codes(2000, k, seed=131), _codes(800, k, seed=132)
    a, b = synth.make_planes(k, K25["K"], K25["L"], K25["W"], seed=3)
    monkeypatch.setenv("HS_TEST_APPEND_COLLISION", "1")
    grown = Engine(k, K25["K"], K25["L"], K25["W"], a, b, hooks=True)
    monkeypatch.delenv("HS_TEST_APPEND_COLLISION")
    grown.index_build(A)
    grown.index_append(B)
    assert grown.profile()["append_rebuilds"] == 1
    fresh = _engine(K25)
    fresh.index_build(np.concatenate([A, B]))
    _assert_equal_handles(grown, fresh, np.concatenate([A, B]), K25["R"], tmp_path, "rebuild")
    grown.close()
    fresh.close()
    # the shipped library has no such switch
    monkeypatch.setenv("HS_TEST_APPEND_COLLISION", "1")
    plain = _engine(K25)
    plain.index_build(A)
    plain.index_append(B)
    assert plain.profile()["append_rebuilds"] == 0
    plain.close()
