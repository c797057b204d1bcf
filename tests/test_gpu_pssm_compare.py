"""hs_pssm_compare on the GPU against the host rule (capi.pssm_compare_host, itself held to the numpy contract by
tests/test_pssm_compare_cpu.py): hits, offsets, scores bit for bit, counts -- with the int8 MFMA filter and without it,
at both tile edges, in self mode, under every batch size, through host and device pointers, under the capacity
protocol and a forced survivor split; element probes that pin the lane map, the shift and the padding; the pairs
that attain the filter's bound; the survivor count predicted from the host tables; refusals; the handle's other calls
around it; and clusters -> profiles -> columns -> compare end to end."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import pssm_compare_ref as ref

pytestmark = pytest.mark.gpu

# the CPU file's shapes; the filter's shape boundary (k * 32 = 1024 and just above); alphabets at and around a stride
SHAPES = [(1, 20), (3, 4), (25, 20), (26, 21), (75, 32), (32, 32), (33, 32), (5, 16), (5, 17), (64, 16), (65, 16)]
SIZES = [(15, 33), (16, 17), (17, 16), (33, 15)]


def _coords(A):
    if A == 20:
        return None
    rng = np.random.default_rng(77)
    c = np.concatenate([synth.coords(), rng.normal(0, 3, size=(max(0, A - 20), 8))])[:A]
    return np.ascontiguousarray(c)


def _engine(k, A, codes=None, hooks=False, options=None):
    a, b = synth.make_planes(k, 2, 1, 200.0, seed=3)
    eng = Engine(k, 2, 1, 200.0, a, b, coords=_coords(A), hooks=hooks, options=options)
    if codes is not None:
        eng.index_build(codes)
    return eng


def _same(got, want, what):
    for f in ("x", "y", "d"):
        assert np.array_equal(got[f], want[f]), (what, f, len(got[f]), len(want[f]))
    assert ref.same_bits(got["score"], want["score"]), (what, "score")
    assert np.array_equal(got["cnt"], want["cnt"]), (what, "cnt")


def _profiles(rng, n, k, A):
    """dyadic entries with empty columns (equal scores and ties between offsets are common), one real-valued profile,
    one with a forbidden residue"""
    P = rng.integers(-8, 9, size=(n, k, A)).astype(np.float64) / 4.0 * rng.integers(0, 2, size=(n, k, 1))
    if n > 2:
        P[1] = rng.normal(0, 1, size=(k, A))
        P[2, 0, 0] = -1e30
    return P


def _thresholds(X, Y, v):
    """about a third of the pairs hit, every other profile with an attained score as its threshold"""
    host = capi.pssm_compare_host(X, -1e300, Y, v)
    ny = len(Y) if Y is not None else len(X)
    t = np.zeros(len(X))
    for x in range(len(X)):
        sc = np.sort(host["score"][host["x"] == x])
        t[x] = sc[(2 * len(sc)) // 3] if len(sc) else 0.0
    assert len(host["x"]) == (len(X) * ny if Y is not None else len(X) * (len(X) - 1) // 2)
    return t


@pytest.mark.parametrize("k,A", SHAPES)
def test_device_equals_host_rule(k, A):
    rng = np.random.default_rng(1000 * k + A)
    X_all, Y_all = _profiles(rng, 33, k, A), _profiles(rng, 33, k, A)
    filtered = k * ((A + 15) // 16 * 16) <= 1024
    eng = _engine(k, A)                                  # no index: none is needed
    try:
        for v in sorted({1, (k + 1) // 2, k}):
            for nx, ny in SIZES if v == 1 else SIZES[:1]:
                X, Y = X_all[:nx], Y_all[:ny]
                t = _thresholds(X, Y, v)
                want = capi.pssm_compare_host(X, t, Y, v)
                assert 0 < len(want["x"]) < nx * ny
                _same(eng.pssm_compare(X, t, Y, v), want, (k, A, v, nx, ny))
                p = eng.profile()
                assert p["pssm_cmp_pairs"] == nx * ny and p["hits"] == len(want["x"])
                assert (p["pssm_cmp_steps"] > 0) == filtered and len(want["x"]) <= p["pssm_cmp_survivors"] <= nx * ny
                if not filtered:
                    assert p["pssm_cmp_survivors"] == nx * ny
            X = X_all[:33]
            t = _thresholds(X, None, v) if k > 1 or v == 1 else np.zeros(33)
            want = capi.pssm_compare_host(X, t, None, v)
            assert np.all(want["x"] < want["y"]) and len(want["x"]) > 0
            _same(eng.pssm_compare(X, t, None, v), want, (k, A, v, "self"))
            assert eng.profile()["pssm_cmp_pairs"] == 33 * 32 // 2
            eng.set_option("pssm_cmp_filter", 0)
            _same(eng.pssm_compare(X, t, None, v), want, (k, A, v, "self, no filter"))
            p = eng.profile()
            assert p["pssm_cmp_steps"] == 0 and p["pssm_cmp_survivors"] == 33 * 32 // 2
            _same(eng.pssm_compare(X, t, Y_all[:17], v), capi.pssm_compare_host(X, t, Y_all[:17], v), (k, A, v, "no filter"))
            eng.set_option("pssm_cmp_filter", 1)
        assert len(eng.pssm_compare(np.zeros((0, k, A)), 0.0)["x"]) == 0          # nothing asked
        assert len(eng.pssm_compare(X_all[:1], -1e300)["x"]) == 0                   # one profile: no pair x < y
    finally:
        eng.close()


@pytest.mark.parametrize("batch", [1, 16, 0])
def test_batches(batch):
    k, A, v = 25, 20, 13
    rng = np.random.default_rng(5)
    X, Y = _profiles(rng, 37, k, A), _profiles(rng, 33, k, A)
    t = _thresholds(X, Y, v)
    eng = _engine(k, A, options={"query_batch": batch})
    try:
        _same(eng.pssm_compare(X, t, Y, v), capi.pssm_compare_host(X, t, Y, v), batch)
        assert eng.profile()["verify_launches"] == (37 if batch == 1 else 3 if batch == 16 else 1)
        ts = _thresholds(X, None, v)
        _same(eng.pssm_compare(X, ts, None, v), capi.pssm_compare_host(X, ts, None, v), (batch, "self"))
        assert eng.profile()["pssm_cmp_pairs"] == 37 * 36 // 2
    finally:
        eng.close()


def test_capacity_protocol_and_forced_split(monkeypatch):
    k, A, v = 25, 20, 13
    rng = np.random.default_rng(6)
    X, Y = _profiles(rng, 17, k, A), _profiles(rng, 33, k, A)
    t = _thresholds(X, Y, v)
    want = capi.pssm_compare_host(X, t, Y, v)
    nh = len(want["x"])
    monkeypatch.setenv("HS_TEST_SPLIT_ABOVE", "4")       # the TEST build: every batch above 4 profiles "overflows"
    eng = _engine(k, A, hooks=True)
    try:
        _same(eng.pssm_compare(X, t, Y, v), want, "split")
        assert eng.profile()["verify_launches"] >= 5 and eng.profile()["pssm_cmp_pairs"] == 17 * 33
        lib, h, vp = eng._lib, eng._h, capi._vp
        for cap in (0, nh - 1, nh):
            hx, hy = np.full(nh + 1, 7, np.uint32), np.full(nh + 1, 7, np.uint32)
            hd, hs, cnt = np.full(nh + 1, 7, np.int32), np.full(nh + 1, 7.0), np.full(17, 7, np.uint64)
            n = C.c_uint64(0)
            st = lib.hs_pssm_compare(h, vp(X), C.c_uint64(17), vp(Y), C.c_uint64(33), vp(t), C.c_uint32(v),
                                     None if cap == 0 else vp(hx), None if cap == 0 else vp(hy),
                                     None if cap == 0 else vp(hd), None if cap == 0 else vp(hs), C.c_uint64(cap),
                                     C.byref(n), vp(cnt))
            assert st == (capi.HS_OK if cap == nh else capi.HS_ERR_CAPACITY) and n.value == nh, cap
            assert np.array_equal(cnt, want["cnt"])
            if cap == nh:
                _same(dict(x=hx[:nh], y=hy[:nh], d=hd[:nh], score=hs[:nh], cnt=cnt), want, "exact cap")
            assert hx[nh] == 7 and hs[nh] == 7.0
    finally:
        eng.close()


@pytest.mark.parametrize("A", [20, 21])
def test_element_probes(A):
    """X profile (i, r) holds a single 1.0 at column i, residue r; Y profile (j, r') likewise; t = 1.  A hit iff
    r == r' and i - j is an allowed offset, with d = i - j: every (i, j, r, r') at k = 5, which pins the lane map,
    the shift and the padding element by element.  The filter passes exactly the hits."""
    k = 5
    P = np.zeros((k * A, k, A))
    for i in range(k):
        for r in range(A):
            P[i * A + r, i, r] = 1.0
    eng = _engine(k, A)
    try:
        for v in (1, 3, 5):
            got = eng.pssm_compare(P, 1.0, P.copy(), v)
            i, r = got["x"] // A, got["x"] % A
            j, r2 = got["y"] // A, got["y"] % A
            assert np.array_equal(r, r2) and np.array_equal(got["d"], (i.astype(np.int64) - j).astype(np.int32))
            assert np.all(got["score"] == 1.0)
            n_pairs = sum(1 for a in range(k) for b in range(k) if abs(a - b) <= k - v)
            assert len(got["x"]) == n_pairs * A
            p = eng.profile()
            assert p["pssm_cmp_survivors"] == len(got["x"]) and p["pssm_cmp_steps"] > 0
            _same(got, capi.pssm_compare_host(P, 1.0, P.copy(), v), (A, v))
    finally:
        eng.close()


def test_worst_case_pairs_are_returned():
    k, A = 25, 20
    eng = _engine(k, A)
    try:
        for sign in (1, -1):
            for mixed, kw in ((False, {}), (True, dict(q_hi=2, frac=0.499))):
                X, Y = ref.lined_up_pair(k, A, sign, mixed=mixed, **kw)
                for a, b in ((X, Y), (Y, X)):
                    want = capi.pssm_compare_host(a, -1e300, b, k)
                    t = float(want["score"][0])               # the attained score as the threshold
                    got = eng.pssm_compare(a, t, b, k)
                    _same(got, capi.pssm_compare_host(a, t, b, k), (sign, mixed))
                    assert list(got["d"]) == [0] and eng.profile()["pssm_cmp_survivors"] == 1
                    assert len(eng.pssm_compare(a, np.nextafter(t, np.inf), b, k)["x"]) == 0
    finally:
        eng.close()


def test_survivors_predicted_from_the_tables():
    """pssm_cmp_survivors equals the count predicted from hs_pssm_compare_tables on the planted-family set: this
    holds the device's tables and the operand order."""
    P, fam, shift = ref.planted_families()
    k, A, v = P.shape[1], P.shape[2], 13
    eng = _engine(k, A)
    try:
        for frac in (0.5, 0.6):
            t = frac * k
            pred = ref.predicted_survivors(P, t, None, v)
            got = eng.pssm_compare(P, t, None, v)
            p = eng.profile()
            assert p["pssm_cmp_survivors"] == pred.sum() and p["pssm_cmp_pairs"] == 69006
            assert pred[got["x"], got["y"]].all() and 0 < len(got["x"]) <= pred.sum() <= 2 * len(got["x"])
            _same(got, capi.pssm_compare_host(P, t, None, v), frac)
        # X against Y with per-profile thresholds: the first 100 against the rest
        t = np.linspace(0.3 * k, 0.6 * k, 100)
        pred = ref.predicted_survivors(P[:100], t, P[100:], v)
        got = eng.pssm_compare(P[:100], t, P[100:], v)
        assert eng.profile()["pssm_cmp_survivors"] == pred.sum()
        _same(got, capi.pssm_compare_host(P[:100], t, P[100:], v), "x against y")
    finally:
        eng.close()


def test_device_pointers_and_refusals():
    import torch
    k, A, v = 25, 20, 13
    rng = np.random.default_rng(8)
    X, Y = _profiles(rng, 33, k, A), _profiles(rng, 17, k, A)
    t = _thresholds(X, Y, v)
    eng = _engine(k, A)
    try:
        for Yh in (Y, None):
            th = t if Yh is not None else _thresholds(X, None, v)
            want = capi.pssm_compare_host(X, th, Yh, v)
            nh = len(want["x"])
            dX, dt = torch.from_numpy(X).cuda(), torch.from_numpy(th).cuda()
            dY = torch.from_numpy(Yh).cuda() if Yh is not None else None
            cap = nh + 5
            dx = torch.full((cap,), 7, dtype=torch.int32, device="cuda")
            dy = torch.full((cap,), 7, dtype=torch.int32, device="cuda")
            dd = torch.full((cap,), 7, dtype=torch.int32, device="cuda")
            ds = torch.full((cap,), 7.0, dtype=torch.float64, device="cuda")
            dc = torch.full((33,), 7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            args = (dx.data_ptr(), dy.data_ptr(), dd.data_ptr(), ds.data_ptr(), cap, dc.data_ptr())
            yp, ny = (dY.data_ptr(), 17) if dY is not None else (0, 0)
            n = eng.pssm_compare_dev(dX.data_ptr(), 33, yp, ny, dt.data_ptr(), v, *args)
            assert n == nh
            got = dict(x=dx[:n].cpu().numpy().astype(np.uint32), y=dy[:n].cpu().numpy().astype(np.uint32),
                       d=dd[:n].cpu().numpy(), score=ds[:n].cpu().numpy(), cnt=dc.cpu().numpy().astype(np.uint64))
            _same(got, want, "dev")
            assert int(dx[n]) == 7 and float(ds[n]) == 7.0
            # the value errors are found on the device, before anything is written
            dx.fill_(9), dy.fill_(9), dd.fill_(9), ds.fill_(9.0), dc.fill_(9)
            for where, bad in (("X", float("nan")), ("X", float("-inf")), ("X", 2.0 ** 101), ("Y", float("nan")),
                               ("Y", -2.0 ** 101), ("t", float("nan")), ("t", float("inf"))):
                if where == "Y" and dY is None:
                    continue
                dX2, dt2, dY2 = dX.clone(), dt.clone(), dY.clone() if dY is not None else None
                if where == "X":
                    dX2[32, 24, 19] = bad
                elif where == "Y":
                    dY2[16, 0, 0] = bad
                else:
                    dt2[32] = bad
                torch.cuda.synchronize()
                with pytest.raises(HsError) as e:
                    eng.pssm_compare_dev(dX2.data_ptr(), 33, dY2.data_ptr() if dY2 is not None else 0, ny, dt2.data_ptr(),
                                         v, *args)
                assert e.value.status == capi.HS_ERR_INVALID and e.value.n_hits == 0, (where, bad)
                assert bool((dx == 9).all()) and bool((dd == 9).all()) and bool((ds == 9.0).all()) and bool((dc == 9).all())
            with pytest.raises(HsError) as e:                  # capacity through device pointers
                eng.pssm_compare_dev(dX.data_ptr(), 33, yp, ny, dt.data_ptr(), v, dx.data_ptr(), dy.data_ptr(),
                                     dd.data_ptr(), ds.data_ptr(), nh - 1, dc.data_ptr())
            assert e.value.status == capi.HS_ERR_CAPACITY and e.value.n_hits == nh
            assert np.array_equal(dc.cpu().numpy().astype(np.uint64), want["cnt"])
    finally:
        eng.close()


def test_host_pointer_refusals_write_nothing():
    k, A = 3, 4
    X, Y, t = np.full((2, k, A), 0.5), np.full((3, k, A), 0.25), np.zeros(2)
    eng = _engine(k, A)
    vp = capi._vp
    try:
        def call(X_=X, nx=2, Y_=Y, ny=3, t_=t, v=1, cap=8, null_out=False):
            hx, hy = np.full(8, 9, np.uint32), np.full(8, 9, np.uint32)
            hd, hs, cnt = np.full(8, 9, np.int32), np.full(8, 9.0), np.full(2, 9, np.uint64)
            n = C.c_uint64(77)
            st = eng._lib.hs_pssm_compare(eng._h, vp(X_) if X_ is not None else None, C.c_uint64(nx),
                                          vp(Y_) if Y_ is not None else None, C.c_uint64(ny),
                                          vp(t_) if t_ is not None else None, C.c_uint32(v), None if null_out else vp(hx),
                                          vp(hy), vp(hd), vp(hs), C.c_uint64(cap), C.byref(n), vp(cnt))
            clean = (hx == 9).all() and (hy == 9).all() and (hd == 9).all() and (hs == 9.0).all() and (cnt == 9).all()
            return st, clean, n.value

        st, _, n = call()
        assert st == capi.HS_OK and n == 6
        nan_x, big_x, nan_y, inf_y = X.copy(), X.copy(), Y.copy(), Y.copy()
        nan_x[1, 2, 3], big_x[0, 0, 0], nan_y[2, 0, 1], inf_y[0, 0, 0] = np.nan, 2.6e30, np.nan, -np.inf
        cases = dict(v0=dict(v=0), v_above_k=dict(v=k + 1), nx_huge=dict(nx=1 << 27), ny_huge=dict(ny=1 << 27),
                     nx0_with_y=dict(nx=0), ny0_with_x=dict(ny=0), nan_x=dict(X_=nan_x), big_x=dict(X_=big_x),
                     nan_x_self=dict(X_=nan_x, Y_=None, ny=0), nan_y=dict(Y_=nan_y), inf_y=dict(Y_=inf_y),
                     nan_t=dict(t_=np.array([0.0, np.nan])), inf_t=dict(t_=np.array([np.inf, 0.0])),
                     null_out=dict(null_out=True), null_x=dict(X_=None), null_t=dict(t_=None))
        for name, kw in cases.items():
            st, clean, n = call(**kw)
            assert st == capi.HS_ERR_INVALID and clean and n == 0, name
        st, _, n = call(cap=0, null_out=True)
        assert st == capi.HS_ERR_CAPACITY and n == 6
        for name, value in (("pssm_cmp_filter", 2), ("pssm_cmp_filter", -1)):
            with pytest.raises(HsError):
                eng.set_option(name, value)
    finally:
        eng.close()


def test_a_handle_with_an_index_and_its_other_calls():
    from tests import pssm_ref
    k, A, v = 25, 20, 13
    rng = np.random.default_rng(12)
    codes = rng.integers(0, A, size=(3000, k)).astype(np.uint8)
    S = rng.integers(-16, 17, size=(9, k, A)) / 4.0
    ts = np.sort(pssm_ref.scores(S, codes), axis=1)[:, -40].copy()
    X, Y = _profiles(rng, 33, k, A), _profiles(rng, 17, k, A)
    t = _thresholds(X, Y, v)
    want = capi.pssm_compare_host(X, t, Y, v)
    eng = _engine(k, A, codes)
    try:
        before = eng.pssm_scan(S, ts)
        _same(eng.pssm_compare(X, t, Y, v), want, "indexed handle")
        after = eng.pssm_scan(S, ts)
        for f in ("m", "id", "cnt"):
            assert np.array_equal(before[f], after[f]), f
        assert ref.same_bits(before["score"], after["score"]) and len(before["m"]) >= 9 * 40
        _same(eng.pssm_compare(X, t, Y, v), want, "after a scan")
        assert eng.profile()["pssm_pairs"] == 0 and eng.profile()["pssm_cmp_pairs"] == 33 * 17
    finally:
        eng.close()


def test_clusters_to_profiles_to_compare():
    """dbscan -> cluster_pssm -> pssm_compare_columns -> pssm_compare in self mode, on a database with two planted
    motifs of 30 columns cut into 25-mer windows (6 shifts each, 6 copies per window) among random k-mers.  Column c of
    a motif is column c - s of the window at shift s, and column p of Y meets column p + d of X: the clusters of shifts
    s_x and s_y come back as one hit with d = s_y - s_x; no pair of distinct motifs does."""
    k, A, v = 25, 20, 13
    rng = np.random.default_rng(31)
    motifs = rng.integers(0, A, size=(2, 30)).astype(np.uint8)
    rows, tag = [], []
    for m in range(2):
        for s in range(6):
            for _ in range(6):
                rows.append(motifs[m, s:s + k])
                tag.append((m, s))
    noise = rng.integers(0, A, size=(500, k)).astype(np.uint8)
    order = rng.permutation(len(rows) + len(noise))
    codes = np.ascontiguousarray(np.concatenate([np.array(rows), noise])[order])
    tags = np.array(tag + [(-1, -1)] * len(noise))[order]
    eng = _engine(k, A, codes)
    try:
        lab = eng.dbscan(0.5, 4)
        assert lab["n_clusters"] == 12
        cp = eng.cluster_pssm(lab["label"], min_size=4, weights="none", bg=np.full(A, 1.0 / A), threshold=None)
        assert len(cp["label"]) == 12
        row_tag = tags[cp["label"]]                           # a cluster's label is the id of one of its members
        P = capi.pssm_compare_columns(cp["S"], "pearson")
        got = eng.pssm_compare(P, 0.5 * k, None, v)
        _same(got, capi.pssm_compare_host(P, 0.5 * k, None, v), "end to end")
        mx, sx = row_tag[got["x"]].T
        my, sy = row_tag[got["y"]].T
        assert np.array_equal(mx, my) and np.array_equal(got["d"], (sy - sx).astype(np.int32))
        assert len(got["x"]) == 2 * 15                        # every pair of shifts of a motif: |s_x - s_y| <= 5 <= k - v
    finally:
        eng.close()
