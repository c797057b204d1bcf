"""hs_index_remove: a handle built over A and shrunk by a set of ids must be indistinguishable from a fresh handle
built over the surviving rows -- the file hs_index_save writes byte for byte, hs_index_info_get but device_bytes, and
every search hit for hit with the distance's bits.  Databases are mutated copies of a few hundred random k-mers
(synth.make_query_codes), about five to a bucket, so that a removal empties some buckets, beheads others and leaves
the rest alone."""
import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth

pytestmark = pytest.mark.gpu

K25 = dict(k=25, K=6, L=3, W=60.0, R=40.0)    # 3000 of _codes: ~ 1400 buckets a table, the largest of ~ 20
GONE = np.uint32(0xffffffff)


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


def _engine(shape, planes_seed=3, **options):
    a, b = synth.make_planes(shape["k"], shape["K"], shape["L"], shape["W"], seed=planes_seed)
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
        elif isinstance(x[f], dict):
            _same(x[f], y[f], (what, f))
        else:
            assert x[f] == y[f], (what, f)


def _searches(eng, all_codes, R, seed=5):
    """code queries, general centres, the self-join"""
    if not len(all_codes):
        return {}
    qc, _ = synth.make_query_codes(all_codes, 200, max_subst=3, seed=seed)
    centers, _ = synth.make_queries(all_codes, 150, max_subst=3, seed=seed + 1, jitter=0.05)
    return dict(codes=eng.query_codes(qc, R), centres=eng.query(centers, R), self_join=eng.self_join(R))


def _assert_equal_handles(shrunk, fresh, rest, R, tmp_path, what):
    assert _info(shrunk) == _info(fresh), what
    assert _info(shrunk)["n"] == len(rest)
    ps, pf = tmp_path / "shrunk.hsidx", tmp_path / "fresh.hsidx"
    shrunk.index_save(ps)
    fresh.index_save(pf)
    assert ps.read_bytes() == pf.read_bytes(), what
    got, want = _searches(shrunk, rest, R), _searches(fresh, rest, R)
    for name in want:
        _same(got[name], want[name], (what, name))
    return want


def _keep(n, ids):
    keep = np.ones(n, dtype=bool)
    keep[np.asarray(ids, dtype=np.int64)] = False
    return keep


def _new_id(keep):
    """what new_id must be: the cumulative sum of the keep flags"""
    want = (np.cumsum(keep) - 1).astype(np.uint32)
    want[~keep] = GONE
    return want


def _shrink_and_compare(shape, A, removals, tmp_path, what, planes_seed=3, **options):
    """removals: id arrays applied one after the other, each in the ids of its time"""
    shrunk, fresh = _engine(shape, planes_seed, **options), _engine(shape, planes_seed, **options)
    shrunk.index_build(A)
    rest, dead_buckets, retupled = A, 0, 0
    for ids in removals:
        before = shrunk.index_info()
        new_id = shrunk.index_remove(ids)
        keep = _keep(len(rest), ids)
        assert np.array_equal(new_id, _new_id(keep)), what
        if len(ids):
            p = shrunk.profile()
            assert p["remove_rebuilds"] == 0, what
            dead_buckets += p["remove_dead_buckets"]
            retupled += p["remove_retupled"]
            assert p["remove_dead_buckets"] == sum(before["n_buckets"]) - sum(shrunk.index_info()["n_buckets"])
        rest = rest[keep]
    info = fresh.index_build(rest)
    want = _assert_equal_handles(shrunk, fresh, rest, shape["R"], tmp_path, what)
    shrunk.close()
    fresh.close()
    return want, info, dead_buckets, retupled


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 1500, 2999, 3000])
def test_random_removal_equals_build(m, tmp_path):
    n = 3000
    A = _codes(n, K25["k"], seed=21)
    ids = np.random.default_rng(100 + m).choice(n, size=m, replace=False).astype(np.uint32)
    want, info, dead_buckets, retupled = _shrink_and_compare(K25, A, [ids], tmp_path, m)
    if m == 1500:
        # the case means something: buckets vanished, buckets lost their first member and kept others (with ~ 2
        # members to a bucket and every second k-mer gone, both happen hundreds of times), the searches found pairs
        assert dead_buckets > 0 and retupled > 0
        assert len(want["codes"]["q"]) > 100 and len(want["self_join"]["i"]) > 1000
    if m == 3000:
        assert info["n"] == 0 and sum(info["n_buckets"]) == 0 and dead_buckets > 0


@pytest.mark.parametrize("lo,hi", [(0, 64), (64, 128), (2936, 3000)])
def test_wave_edges_of_the_id_order(lo, hi, tmp_path):
    A = _codes(3000, K25["k"], seed=21)
    want, _, dead_buckets, retupled = _shrink_and_compare(K25, A, [np.arange(lo, hi, dtype=np.uint32)], tmp_path, (lo, hi))
    assert dead_buckets > 0 and retupled >= 0
    assert len(want["codes"]["q"]) > 100 and len(want["self_join"]["i"]) > 1000


def test_one_large_bucket_loses_most_and_then_all_of_its_members(tmp_path):
    k = K25["k"]
    one = synth.make_db(1, k, seed=51)
    A = np.concatenate([_codes(400, k, seed=52), np.repeat(one, 2000, axis=0)])
    rng = np.random.default_rng(54)
    A = A[rng.permutation(len(A))]
    copies = np.nonzero(np.all(A == one[0], axis=1))[0]
    assert len(copies) == 2000
    shape = dict(K25, R=1.0)    # (the copies alone: 800 x 799 pairs per table would be the self-join at R = 40 too)
    first = rng.permutation(copies)[:1200].astype(np.uint32)
    _, info, _, _ = _shrink_and_compare(shape, A, [first], tmp_path, "1200 of 2000")
    assert min(info["max_bucket"]) == 800
    _, info, dead_buckets, _ = _shrink_and_compare(shape, A, [copies.astype(np.uint32)], tmp_path, "2000 of 2000")
    assert max(info["max_bucket"]) < 100 and dead_buckets == K25["L"]


def _aliased(oracle):
    k, K, L, W = 25, 2, 2, 1.0
    a, b = synth.make_planes(k, K, L, W, seed=99)
    codes = synth.make_db(8000, k, seed=8)
    ints = oracle.hash_all(a, b, W, oracle.embed_codes(codes))
    dead = []
    for l in range(L):
        fp = np.array([capi.key_fingerprint(t, 0) for t in ints[:, l]], dtype=np.uint64)
        order = np.lexsort((np.arange(len(fp)), fp))
        same = np.nonzero((fp[order][1:] == fp[order][:-1]) &
                          np.concatenate([[True], fp[order][1:-1] != fp[order][:-2]]))[0]   # first and second member
        first, second = order[same], order[same + 1]
        other = np.any(ints[first, l] != ints[second, l], axis=1)
        assert other.sum() > 0
        dead.append(first[other])
    return dict(k=k, K=K, L=L, W=W, R=45.0), codes, np.unique(np.concatenate(dead)).astype(np.uint32)


def test_aliased_first_members_change_the_tuple(oracle, tmp_path):
    """K = 2 at W = 1: (1,23) and (12,3) are one bucket.  The first member of every bucket whose second member carries
    other ints goes: the tuple must become the second member's -- it feeds the saved file, the directory records and
    the giant buckets of the bucket partition."""
    shape, codes, dead = _aliased(oracle)
    shrunk, fresh = _engine(shape, 99), _engine(shape, 99)
    shrunk.index_build(codes)
    shrunk.index_remove(dead)
    p = shrunk.profile()
    assert p["remove_retupled"] > 0 and p["remove_rebuilds"] == 0
    rest = codes[_keep(len(codes), dead)]
    fresh.index_build(rest)
    _assert_equal_handles(shrunk, fresh, rest, shape["R"], tmp_path, "aliased")
    qc, _ = synth.make_query_codes(rest, 300, max_subst=3, seed=9)
    for part in range(3):
        for eng in (shrunk, fresh):
            eng.set_bucket_partition(part, 3)
        _same(shrunk.query_codes(qc, shape["R"]), fresh.query_codes(qc, shape["R"]), ("part", part))
    shrunk.close()
    fresh.close()


@pytest.mark.parametrize("shape,options", [
    (dict(k=15, K=6, L=3, W=45.0, R=30.0), dict(build_grouping=1)),      # wide rows
    (dict(k=39, K=6, L=3, W=90.0, R=60.0), {}),                          # two packed words
    (dict(k=60, K=6, L=3, W=140.0, R=90.0), {}),                         # no int8 records
    (K25, dict(probe_records=0)),
], ids=["k15", "k39", "k60", "no_probe_records"])
def test_other_shapes(shape, options, tmp_path):
    A = _codes(3000, shape["k"], seed=61)
    ids = np.random.default_rng(62).choice(3000, size=1100, replace=False).astype(np.uint32)
    want, _, dead_buckets, _ = _shrink_and_compare(shape, A, [ids], tmp_path, shape["k"], **options)
    assert dead_buckets > 0 and len(want["self_join"]["i"]) > 100


def test_loaded_index_shrinks(tmp_path):
    k = K25["k"]
    A = _codes(2500, k, seed=81)
    ids = np.random.default_rng(82).choice(2500, size=900, replace=False).astype(np.uint32)
    saved = tmp_path / "a.hsidx"
    first = _engine(K25)
    first.index_build(A)
    first.index_save(saved)
    first.close()
    shrunk, fresh = _engine(K25), _engine(K25)
    shrunk.index_load(saved)
    shrunk.index_remove(ids)
    rest = A[_keep(len(A), ids)]
    fresh.index_build(rest)
    _assert_equal_handles(shrunk, fresh, rest, K25["R"], tmp_path, "loaded")
    shrunk.close()
    fresh.close()


def test_call_forms_agree_and_new_id_is_the_cumulative_sum(tmp_path):
    import torch
    k, n = K25["k"], 3000
    A = _codes(n, k, seed=91)
    rng = np.random.default_rng(92)
    # overlapping ranges, one of no ids, one up to the last id; as ids: shuffled, with duplicates
    first = np.array([10, 40, 700, 1234, 2000, 2990], dtype=np.uint64)
    count = np.array([50, 100, 1, 0, 130, 10], dtype=np.uint64)
    ids = np.concatenate([np.arange(f, f + c) for f, c in zip(first, count)]).astype(np.uint32)
    ids = rng.permutation(np.concatenate([ids, ids[:40]]))
    keep = _keep(n, ids)
    rest = A[keep]
    fresh = _engine(K25)
    fresh.index_build(rest)
    by_ids, by_dev, by_ranges = _engine(K25), _engine(K25), _engine(K25)
    for eng in (by_ids, by_dev, by_ranges):
        eng.index_build(A)
    assert np.array_equal(by_ids.index_remove(ids), _new_id(keep))
    d_new = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    by_dev.index_remove_dev(torch.from_numpy(ids.astype(np.int32)).cuda(), new_id=d_new)
    assert np.array_equal(d_new.cpu().numpy().view(np.uint32), _new_id(keep))
    assert np.array_equal(by_ranges.index_remove_ranges(first, count), _new_id(keep))
    for eng, what in ((by_ids, "ids"), (by_dev, "_dev"), (by_ranges, "ranges")):
        _assert_equal_handles(eng, fresh, rest, K25["R"], tmp_path, what)
    # nothing to remove: a no-op, new_id the identity
    info = _info(by_ids)
    assert np.array_equal(by_ids.index_remove(np.zeros(0, dtype=np.uint32)), np.arange(len(rest), dtype=np.uint32))
    assert np.array_equal(by_ids.index_remove_ranges([5], [0]), np.arange(len(rest), dtype=np.uint32))
    d_new = torch.zeros(len(rest), dtype=torch.int32, device="cuda")
    by_ids.index_remove_dev((0, 0), new_id=d_new)
    assert np.array_equal(d_new.cpu().numpy(), np.arange(len(rest), dtype=np.int32))
    assert _info(by_ids) == info
    for eng in (by_ids, by_dev, by_ranges, fresh):
        eng.close()


def test_append_then_remove_gives_the_original_file_back(tmp_path):
    k = K25["k"]
    A, B = _codes(2000, k, seed=101), _codes(777, k, seed=102)
    eng, fresh = _engine(K25), _engine(K25)
    eng.index_build(A)
    original = tmp_path / "original.hsidx"
    eng.index_save(original)
    eng.index_append(B)
    eng.index_remove(np.arange(2000, 2777, dtype=np.uint32))
    again = tmp_path / "again.hsidx"
    eng.index_save(again)
    assert again.read_bytes() == original.read_bytes()
    fresh.index_build(A)
    _assert_equal_handles(eng, fresh, A, K25["R"], tmp_path, "append, remove")
    eng.close()
    fresh.close()


def test_remove_then_append_replaces(tmp_path):
    k = K25["k"]
    A, B = _codes(2500, k, seed=111), _codes(600, k, seed=112)
    ids = np.random.default_rng(113).choice(2500, size=600, replace=False).astype(np.uint32)
    eng, fresh = _engine(K25), _engine(K25)
    eng.index_build(A)
    eng.index_remove(ids)
    eng.index_append(B)
    everything = np.concatenate([A[_keep(2500, ids)], B])
    fresh.index_build(everything)
    _assert_equal_handles(eng, fresh, everything, K25["R"], tmp_path, "replace")
    eng.close()
    fresh.close()


def test_whole_sequences_of_a_windows_index(tmp_path):
    k = K25["k"]
    rng = np.random.default_rng(121)
    motif = rng.integers(0, 20, size=60, dtype=np.uint8)
    seqs = []
    for n in [300, 120, 25, 200, 24, 95, 400, 0, 110]:           # 24 and 0: shorter than k, no windows
        s = rng.integers(0, 20, size=n, dtype=np.uint8)
        if n >= 90:     # a shared stretch: windows of different proteins in one bucket
            s[10:70] = motif
            s[rng.integers(10, 70, size=3)] = rng.integers(0, 20, size=3, dtype=np.uint8)
        seqs.append(s)

    def joined(which):
        start = np.concatenate([[0], np.cumsum([len(seqs[i]) for i in which])]).astype(np.uint64)
        return np.concatenate([seqs[i] for i in which]), start

    residues, seq_start = joined(range(len(seqs)))
    gone = [1, 6]
    id_start = capi.window_id_start(seq_start, k)
    shrunk, fresh = _engine(K25), _engine(K25)
    info, _ = shrunk.index_build_windows(residues, seq_start)
    new_id = shrunk.index_remove_ranges([id_start[s] for s in gone], [id_start[s + 1] - id_start[s] for s in gone])
    keep = np.ones(info["n"], dtype=bool)
    for s in gone:
        keep[int(id_start[s]):int(id_start[s + 1])] = False
    assert np.array_equal(new_id, _new_id(keep))
    rest_res, rest_start = joined([i for i in range(len(seqs)) if i not in gone])
    _, pos = fresh.index_build_windows(rest_res, rest_start)
    windows = np.stack([rest_res[p:p + k] for p in pos])
    assert len(windows) == int(keep.sum()) == info["n"] - 96 - 376
    _assert_equal_handles(shrunk, fresh, windows, K25["R"], tmp_path, "windows")
    shrunk.close()
    fresh.close()


def _sinks(eng, codes, R, id_start):
    """the calls that leave state sized by n, or built lazily, in a handle"""
    qc, _ = synth.make_query_codes(codes, 300, max_subst=3, seed=7)
    out = dict(codes=eng.query_codes(qc, R))
    assert eng.profile()["join_f6_batches"] > 0        # the FP6 member records exist from here on
    out["annotate"] = eng.annotate(qc, R=R, codes=True)
    out["components"] = eng.components(R)
    out["dbscan"] = eng.dbscan(R, 3)
    out["msf"] = eng.msf(R)
    out["topk"] = eng.query_topk(qc, 5, R=R, codes=True)
    out["self_knn"] = eng.self_knn(R, 5)
    out["seq_match"] = eng.seq_match(qc, id_start, R=R, codes=True)
    out["profile"] = eng.cluster_profile(out["components"]["label"], min_size=2, want_counts=True)
    return out


def test_state_of_the_old_index_does_not_survive_and_settings_do(tmp_path):
    k, R = K25["k"], K25["R"]
    A = _codes(5100, k, seed=131)
    ids = np.random.default_rng(132).choice(5100, size=2100, replace=False).astype(np.uint32)
    id_start = np.arange(0, 5101, 100, dtype=np.uint64)          # 51 "sequences" of 100 ids
    shrunk, fresh = _engine(K25), _engine(K25)
    for eng in (shrunk, fresh):
        eng.set_verify_mode("join")
        eng.set_multiprobe(2)
    shrunk.index_build(A)
    _sinks(shrunk, A, R, id_start)                     # FP6 records, annotation slots, forests ... of 5100 k-mers
    new_id = shrunk.index_remove(ids)
    keep = new_id != GONE
    new_start = np.concatenate([[0], np.cumsum(keep)])[id_start.astype(np.int64)].astype(np.uint64)
    rest = A[keep]
    fresh.index_build(rest)
    got, want = _sinks(shrunk, rest, R, new_start), _sinks(fresh, rest, R, new_start)
    for name in want:
        _same(got[name], want[name], name)
    assert len(want["annotate"]["id"]) > 100 and want["components"]["n_edges"] > 1000
    assert want["seq_match"]["n_hits"] > 100
    # multi-probe survived: one probe per table finds fewer candidates
    with_T = shrunk.query_codes(rest[:200], R)
    shrunk.set_multiprobe(0)
    fresh.set_multiprobe(0)
    without = shrunk.query_codes(rest[:200], R)
    _same(without, fresh.query_codes(rest[:200], R), "T = 0")
    assert with_T["cand"].sum() > without["cand"].sum()
    shrunk.close()
    fresh.close()


def test_refused_calls_leave_the_index_alone():
    k, R = K25["k"], K25["R"]
    A = _codes(2000, k, seed=141)
    qc, _ = synth.make_query_codes(A, 200, max_subst=3, seed=8)
    eng = _engine(K25)
    import torch
    for call in (lambda: eng.index_remove([1, 2]), lambda: eng.index_remove_ranges([0], [2]),
                 lambda: eng.index_remove_dev(torch.tensor([1, 2], dtype=torch.int32).cuda()),
                 lambda: eng.index_remove([])):
        with pytest.raises(HsError) as e:
            call()
        assert e.value.status == capi.HS_ERR_STATE          # unbuilt
    info = eng.index_build(A)
    before = eng.query_codes(qc, R)

    def refused(call):
        with pytest.raises(HsError) as e:
            call()
        assert e.value.status == capi.HS_ERR_INVALID
        assert eng.index_info() == info
        _same(eng.query_codes(qc, R), before, "refused")

    refused(lambda: eng.index_remove([5, 2000, 7]))                                   # id == n
    refused(lambda: eng.index_remove([0xffffffff]))
    refused(lambda: eng.index_remove_dev(torch.tensor([5, 2000, 7], dtype=torch.int32).cuda()))
    refused(lambda: eng.index_remove_ranges([10, 1990], [5, 11]))                     # a range past n
    refused(lambda: eng.index_remove_ranges([2001], [0]))
    refused(lambda: eng.index_remove_ranges([5], [1 << 63]))
    refused(lambda: eng.index_remove_ranges([(1 << 64) - 1], [2]))
    eng.index_remove([5, 1999, 7])                          # ... and the handle still shrinks
    assert eng.index_info()["n"] == 1997
    eng.close()


def test_seed_above_zero_rebuilds(monkeypatch, tmp_path):
    """The test build's HS_TEST_REMOVE_RESEED: the call treats the index's seed as non-zero and runs the build loop
    over the compacted codes from seed 0; it ends with the same index."""
    k = K25["k"]
    A = _codes(2800, k, seed=151)
    ids = np.random.default_rng(152).choice(2800, size=800, replace=False).astype(np.uint32)
    keep = _keep(2800, ids)
    a, b = synth.make_planes(k, K25["K"], K25["L"], K25["W"], seed=3)
    monkeypatch.setenv("HS_TEST_REMOVE_RESEED", "1")
    shrunk = Engine(k, K25["K"], K25["L"], K25["W"], a, b, hooks=True)
    monkeypatch.delenv("HS_TEST_REMOVE_RESEED")
    shrunk.index_build(A)
    assert np.array_equal(shrunk.index_remove(ids), _new_id(keep))
    p = shrunk.profile()
    assert p["remove_rebuilds"] == 1 and p["remove_dead_buckets"] > 0
    fresh = _engine(K25)
    fresh.index_build(A[keep])
    _assert_equal_handles(shrunk, fresh, A[keep], K25["R"], tmp_path, "rebuild")
    shrunk.close()
    fresh.close()
    # the shipped library has no such switch
    monkeypatch.setenv("HS_TEST_REMOVE_RESEED", "1")
    plain = _engine(K25)
    plain.index_build(A)
    plain.index_remove(ids)
    assert plain.profile()["remove_rebuilds"] == 0
    plain.close()
