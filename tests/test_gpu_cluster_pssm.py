"""hs_cluster_weighted_profile / hs_cluster_pssm_cover on the GPU: the device forms against the host rules
(capi.cluster_weights_codes, capi.cluster_cover_codes; tests/test_cluster_pssm_cpu.py pins those to the Python-integer
reference without a GPU) bit for bit -- every shape up to the LDS limit, n = 1, 65, 4097, rows whole inside an item, cut
by one and by many edges, items of 1, 4, 5 and 9 rows, row batches, one row of everything, host and device pointers,
counts given and not, after an append and a removal, among the handle's other calls, the refusals -- and the chain
dbscan -> cluster_pssm -> pssm_scan on a planted-family database."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import cluster_pssm_ref as ref
from tests import summary_ref as sr
from tests.test_gpu_clustering import _families

pytestmark = pytest.mark.gpu

SHAPES = [(1, 20), (25, 20), (26, 20), (4, 32), (75, 32)]
NOISE = capi.NOISE
# (summary_chunk, summary_rows): the defaults; one slot per item; chunks that the planted rows fit and do not fit; one
# row and three rows per batch
OPTIONS = [(0, 0), (1, 0), (64, 0), (100, 0), (0, 1), (64, 3)]


def _engine(codes, alphabet, options=None):
    k = codes.shape[1]
    a, b = synth.make_planes(k, 2, 1, 200.0, seed=3)
    coords = None if alphabet == 20 else np.ascontiguousarray(np.random.default_rng(77).normal(0, 3, size=(alphabet, 8)))
    eng = Engine(k, 2, 1, 200.0, a, b, coords=coords, options=options)
    eng.index_build(codes)
    return eng


def _planted_sizes(n):
    """Row sizes, in label order, that at 64 slots per item give items of 1, 4, 5 and 9 rows (one round and more than
    one round of the four waves), a row cut by many edges, rows cut by one, and rows of one member"""
    if n < 4097:
        return [n // 3, 1, n - n // 3 - 1] if n >= 3 else [n]
    sizes = [64] + [16] * 4 + [13, 13, 13, 13, 12] + [7] * 8 + [4, 4] + [1000] + [30, 50] + [1] * 70
    return sizes + [n - sum(sizes) - 300]          # 300 k-mers stay noise


def _labels(rng, n):
    """dict of label arrays: 'planted' (the sizes above, members scattered over the ids, label values that are no
    member's id order), 'one' (one row of all n), 'mixed' (random small clusters and noise)"""
    perm = rng.permutation(n)
    planted = np.full(n, NOISE, np.uint32)
    at = 0
    for r, s in enumerate(_planted_sizes(n)):
        planted[perm[at:at + s]] = min(n - 1, 2 * r) if n >= 4097 else r % n
        at += s
    mixed = rng.integers(0, max(1, n // 5), size=n).astype(np.uint32)
    mixed[rng.random(n) < 0.15] = NOISE
    return dict(planted=planted, one=np.full(n, n - 1, np.uint32), mixed=mixed)


def _profiles(rng, rows, k, A):
    S = rng.integers(-6, 7, size=(rows, k, A)) / 2.0        # coarse: the minimum of a row is often tied
    if rows:
        S[0, :, 0] = -1e30                                   # a forbidden residue: scores are negative as well
    return S


def _same(got, want, what):
    ref.assert_same(got, want, what)
    assert set(got) == set(want), (what, set(got), set(want))


@pytest.mark.parametrize("k,alphabet", SHAPES)
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_device_equals_host_rule(k, alphabet, n):
    rng = np.random.default_rng(1000 * k + 10 * alphabet + n)
    codes = rng.integers(0, alphabet, size=(n, k)).astype(np.uint8)
    codes[rng.random(n) < 0.3] = codes[0]                    # repeats: unequal weights, tied scores
    labels = _labels(rng, n)
    cases = []
    for name, label in labels.items():
        for min_size in ((1, 5) if name != "one" else (1,)):
            want = capi.cluster_weights_codes(codes, alphabet, label, min_size, want_counts=True)
            rows = len(want["label"])
            S = _profiles(rng, rows, k, alphabet)
            cases.append((name, label, min_size, want, S, capi.cluster_cover_codes(codes, alphabet, label, S, min_size)))
            if n == 65:                                      # the second witness: the Python-integer reference
                ref.assert_same(want, ref.weighted_profile(codes, alphabet, label, min_size), name)
                ref.assert_same(cases[-1][5], ref.cover(codes, label, min_size, S), name)
    if n == 4097:
        sizes = dict(zip(*np.unique(labels["planted"][labels["planted"] != NOISE], return_counts=True)))
        assert sorted(sizes.values())[-2:] == [1000, n - sum(_planted_sizes(n)[:-1]) - 300] and min(sizes.values()) == 1
    eng = _engine(codes, alphabet)
    try:
        for chunk, rows_per_batch in OPTIONS:
            eng.set_option("summary_chunk", chunk)
            eng.set_option("summary_rows", rows_per_batch)
            for name, label, min_size, want, S, want_cover in cases:
                what = (k, alphabet, n, chunk, rows_per_batch, name, min_size)
                _same(eng.cluster_weighted_profile(label, min_size, want_counts=True), want, what)
                bare = eng.cluster_weighted_profile(label, min_size)
                assert "counts" not in bare
                ref.assert_same(bare, want, what)
                prof = eng.profile()
                assert prof["summary_weight_rows"] == len(want["label"])
                if not rows_per_batch:
                    ch = chunk if chunk else 512
                    assert prof["summary_weight_items"] == (int(want["size"].sum()) + ch - 1) // ch
                _same(eng.cluster_pssm_cover(label, S, min_size), want_cover, what)
        # the counts are hs_cluster_profile's
        name, label, min_size, want, _, _ = cases[0]
        assert np.array_equal(eng.cluster_profile(label, min_size, want_counts=True)["counts"], want["counts"])
    finally:
        eng.close()


@pytest.fixture(scope="module")
def handle():
    rng = np.random.default_rng(41)
    k, A, n = 25, 20, 1500
    codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
    codes[rng.random(n) < 0.3] = codes[7]
    eng = _engine(codes, A)
    yield eng, codes, rng
    eng.close()


def test_device_pointers_counts_null_and_given_and_refusals(handle):
    import torch
    eng, codes, rng = handle
    n, k = codes.shape
    A, min_size = 20, 3
    label = _labels(rng, n)["mixed"]
    want = capi.cluster_weights_codes(codes, A, label, min_size, want_counts=True)
    rows, cap = len(want["label"]), n // min_size
    assert 2 <= rows < cap
    dev = "cuda"
    d_label = torch.from_numpy(label.view(np.int32)).to(dev)
    P32, P64 = 0x7ffffffe, 0x7ffffffffffffffe

    def poisoned():
        return dict(label=torch.full((cap,), P32, dtype=torch.int32, device=dev),
                    size=torch.full((cap,), P32, dtype=torch.int32, device=dev),
                    counts=torch.full((cap, k, A), P32, dtype=torch.int32, device=dev),
                    wcounts=torch.full((cap, k, A), P64, dtype=torch.int64, device=dev),
                    wsum=torch.full((cap,), P64, dtype=torch.int64, device=dev),
                    distinct=torch.full((cap,), P32, dtype=torch.int32, device=dev))

    def call(o, lab=d_label, c=cap, counts=True, ws=True, ms=min_size):
        torch.cuda.synchronize()
        return eng.cluster_weighted_profile_dev(lab.data_ptr(), ms, o["label"].data_ptr(), o["size"].data_ptr(),
                                                o["counts"].data_ptr() if counts else None, o["wcounts"].data_ptr(),
                                                o["wsum"].data_ptr() if ws else None,
                                                o["distinct"].data_ptr() if ws else None, c)

    def host(o, fields):
        u = {torch.int32: np.uint32, torch.int64: np.uint64}
        return {f: o[f][:rows].cpu().numpy().view(u[o[f].dtype]) for f in fields}

    o = poisoned()
    assert call(o) == rows
    ref.assert_same(host(o, list(o)), want, "dev")
    for f, t in o.items():
        assert (t[rows:] == (P64 if t.dtype == torch.int64 else P32)).all(), f      # nothing behind the rows
    o2 = poisoned()
    assert call(o2, counts=False, ws=False) == rows
    assert torch.equal(o2["wcounts"][:rows], o["wcounts"][:rows]) and (o2["counts"] == P32).all()
    assert (o2["wsum"] == P64).all() and (o2["distinct"] == P32).all()
    # the cover, device pointers
    S = _profiles(rng, rows, k, A)
    want_cover = capi.cluster_cover_codes(codes, A, label, S, min_size)
    d_S = torch.from_numpy(S).to(dev)
    ms = torch.full((rows,), -7.5, dtype=torch.float64, device=dev)
    am = torch.full((rows,), P32, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.cluster_pssm_cover_dev(d_label.data_ptr(), min_size, d_S.data_ptr(), rows, ms.data_ptr(), am.data_ptr())
    ref.assert_same(dict(min_score=ms.cpu().numpy(), argmin=am.cpu().numpy().view(np.uint32)), want_cover, "dev cover")
    # refusals, every output still poisoned: capacity, a label at n in the last k-mer, min_size 0, a bad entry found on
    # the device, a row count the labels do not give
    o3 = poisoned()
    with pytest.raises(capi.HsError) as e:
        call(o3, c=rows - 1)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == rows
    bad = label.copy()
    bad[n - 1] = n
    d_bad = torch.from_numpy(bad.view(np.int32)).to(dev)
    ms3 = torch.full((rows,), -7.5, dtype=torch.float64, device=dev)
    am3 = torch.full((rows,), P32, dtype=torch.int32, device=dev)

    def cover3(lab=d_label, SS=d_S, r=rows, m=min_size):
        torch.cuda.synchronize()
        eng.cluster_pssm_cover_dev(lab.data_ptr(), m, SS.data_ptr(), r, ms3.data_ptr(), am3.data_ptr())

    refused = [lambda: call(o3, lab=d_bad), lambda: call(o3, ms=0), lambda: cover3(lab=d_bad), lambda: cover3(m=0),
               lambda: cover3(r=rows - 1), lambda: cover3(m=min_size + 1)]
    for v in (np.nan, np.inf, -2.0 ** 101):
        T = S.copy()
        T[rows - 1, k - 1, A - 1] = v
        d_T = torch.from_numpy(T).to(dev)
        refused.append(lambda d_T=d_T: cover3(SS=d_T))
        refused.append(lambda T=T: eng.cluster_pssm_cover(label, T, min_size))
    refused += [lambda: eng.cluster_weighted_profile(bad, min_size), lambda: eng.cluster_weighted_profile(label, 0),
                lambda: eng.cluster_pssm_cover(bad, S, min_size), lambda: eng.cluster_pssm_cover(label, S[:-1], min_size)]
    for i, f in enumerate(refused):
        with pytest.raises(capi.HsError) as e:
            f()
        assert e.value.status == capi.HS_ERR_INVALID, i
    for f, t in o3.items():
        assert (t == (P64 if t.dtype == torch.int64 else P32)).all(), f
    assert (ms3 == -7.5).all() and (am3 == P32).all()
    with pytest.raises(capi.HsError) as e:
        eng.cluster_weighted_profile(label, min_size, cap=rows - 1)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == rows
    # no rows at all, and an unbuilt index
    none = eng.cluster_weighted_profile(np.full(n, NOISE, np.uint32), 1, want_counts=True)
    assert all(len(v) == 0 for v in none.values())
    assert all(len(v) == 0 for v in eng.cluster_pssm_cover(np.full(n, NOISE, np.uint32), S[:0], 1).values())
    a, b = synth.make_planes(k, 2, 1, 200.0, seed=3)
    fresh = Engine(k, 2, 1, 200.0, a, b)
    n_out = C.c_uint64(5)
    st = fresh._lib.hs_cluster_weighted_profile(fresh._h, capi._vp(label), 1, None, None, None, None, None, None, 0,
                                                C.byref(n_out))
    assert st == capi.HS_ERR_STATE and n_out.value == 0
    assert fresh._lib.hs_cluster_pssm_cover(fresh._h, capi._vp(label), 1, None, 0, None, None) == capi.HS_ERR_STATE
    fresh.close()


def test_shared_state_among_the_handles_other_calls(handle):
    """hs_cluster_profile and hs_cluster_radii before, between and after: the grouping state and the scratch are shared"""
    eng, codes, rng = handle
    n, k = codes.shape
    labels = _labels(rng, n)
    la, lb = labels["mixed"], labels["planted"]
    want_a = capi.cluster_weights_codes(codes, 20, la, 2, want_counts=True)
    want_b = capi.cluster_weights_codes(codes, 20, lb, 1, want_counts=True)
    Sa = _profiles(rng, len(want_a["label"]), k, 20)
    cover_a = capi.cluster_cover_codes(codes, 20, la, Sa, 2)
    summary_b = eng.cluster_summary(lb, 1, want_counts=True)
    sr.assert_same(summary_b, sr.summary(codes, lb, 1, synth.coords()), "before")
    _same(eng.cluster_weighted_profile(la, 2, want_counts=True), want_a, "a")
    _same(eng.cluster_pssm_cover(la, Sa, 2), cover_a, "cover a")
    sr.assert_same(eng.cluster_summary(lb, 1, want_counts=True), summary_b, "between")   # its d2 scratch held score keys
    _same(eng.cluster_pssm_cover(la, Sa, 2), cover_a, "cover a again")
    eng.cluster_profile(lb, 1)                                                          # its counts scratch in between
    _same(eng.cluster_weighted_profile(lb, 1, want_counts=True), want_b, "b")
    hits = eng.pssm_weighted_counts(Sa[:2], np.array([0.0, 0.0]))                       # the u tables are shared too
    _same(eng.cluster_weighted_profile(la, 2, want_counts=True), want_a, "a again")
    again = eng.pssm_weighted_counts(Sa[:2], np.array([0.0, 0.0]))
    assert all(np.array_equal(hits[f], again[f]) for f in hits)
    sr.assert_same(eng.cluster_summary(lb, 1, want_counts=True), summary_b, "after")


def test_after_append_and_remove():
    rng = np.random.default_rng(58)
    k, A = 25, 20
    codes = rng.integers(0, A, size=(900, k)).astype(np.uint8)
    more = rng.integers(0, A, size=(333, k)).astype(np.uint8)
    eng = _engine(codes, A)
    try:
        for step in ("built", "appended", "removed"):
            if step == "appended":
                eng.index_append(more)
                codes = np.concatenate([codes, more])
            if step == "removed":
                gone = rng.choice(len(codes), size=200, replace=False)
                eng.index_remove(gone)
                codes = np.delete(codes, gone, axis=0)
            n = len(codes)
            label = _labels(rng, n)["mixed"]
            want = capi.cluster_weights_codes(codes, A, label, 2, want_counts=True)
            _same(eng.cluster_weighted_profile(label, 2, want_counts=True), want, step)
            S = _profiles(rng, len(want["label"]), k, A)
            _same(eng.cluster_pssm_cover(label, S, 2), capi.cluster_cover_codes(codes, A, label, S, 2), step)
    finally:
        eng.close()


def test_discover_profile_search_on_planted_families():
    """families of 20 x 30 plus 400 random 25-mers: dbscan labels -> cluster_pssm -> pssm_scan finds every member of
    every row under its own profile at the covering threshold; at the rank threshold cnt_ge >= size"""
    k, K, L, W, R, min_pts, min_size = 25, 4, 3, 120.0, 50.0, 5, 10
    rng = np.random.default_rng(3)
    codes = np.concatenate([_families(rng, k, 20, 30), synth.make_db(400, k, seed=8)])
    rng.shuffle(codes)
    a, b = synth.make_planes(k, K, L, W, seed=19)
    eng = Engine(k, K, L, W, a, b)
    try:
        eng.index_build(codes)
        label = eng.dbscan(R, min_pts)["label"]
        bg = eng.index_composition()
        all_counts = capi.cluster_weights_codes(codes, 20, np.zeros(len(codes), np.uint32), 1, want_counts=True)["counts"]
        assert np.array_equal(bg.view(np.uint64), capi.pssm_background(all_counts[0]).view(np.uint64))
        host = capi.cluster_weights_codes(codes, 20, label, min_size, want_counts=True)
        rows = len(host["label"])
        assert rows >= 2
        for weights in ("sites", "columns", "none"):
            got = eng.cluster_pssm(label, min_size, weights=weights)
            assert set(got) == {"label", "size", "S", "t", "counts"} | (
                set() if weights == "none" else {"wcounts", "wsum", "distinct"})
            ref.assert_same(got, host, weights)
            if weights == "none":
                S = capi.pssm_log_odds_exact(host["counts"], bg, 1.0)
            else:
                n_eff = host["size"].astype(np.float64) if weights == "sites" else host["distinct"] / np.float64(k)
                S = capi.pssm_log_odds_weighted(host["wcounts"], host["wsum"], n_eff, bg, 1.0)
            assert np.array_equal(got["S"].view(np.uint64), S.view(np.uint64)), weights
            cover = capi.cluster_cover_codes(codes, 20, label, S, min_size)
            assert np.array_equal(got["t"].view(np.uint64), cover["min_score"].view(np.uint64)), weights
            hits = eng.pssm_scan(got["S"], got["t"])
            for r, lab in enumerate(got["label"]):
                members = np.nonzero(label == lab)[0]
                found = hits["id"][hits["m"] == r]
                assert len(members) == got["size"][r] >= min_size and np.isin(members, found).all(), (weights, r)
                at = cover["argmin"][r]
                assert label[at] == lab and hits["score"][(hits["m"] == r) & (hits["id"] == at)] == got["t"][r]
        ranked = eng.cluster_pssm(label, min_size, threshold="rank")
        rank = eng.pssm_rank(ranked["S"], ranked["size"].astype(np.uint64))
        assert np.array_equal(ranked["t"], rank["t"]) and (rank["cnt_ge"] >= ranked["size"]).all()
        assert (eng.pssm_scan(ranked["S"], ranked["t"])["cnt"] >= ranked["size"]).all()
        assert "t" not in eng.cluster_pssm(label, min_size, threshold=None)
        other = eng.cluster_pssm(label, min_size, bg=np.full(20, 0.05), pseudo=0.5)
        assert np.array_equal(other["S"].view(np.uint64), capi.pssm_log_odds_weighted(
            host["wcounts"], host["wsum"], host["size"].astype(np.float64), np.full(20, 0.05), 0.5).view(np.uint64))
    finally:
        eng.close()
