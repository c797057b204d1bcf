"""hs_pssm_pvalue / hs_pssm_pvalue_threshold on the GPU against the host rule (capi.pssm_pvalue_host,
capi.pssm_threshold_host), bit for bit: both cdf tables through a lookup in every bin, p_hi, p_lo, t_p and flag at every
shape and at more profiles than CUs; hit scores at and beyond the grid's ends in any order; batches, device pointers,
the upper side alone and the index's own background, none of which may show; the scan at t_p composed with the
p-values of its hits; the hit count on a database drawn from the null model; refusals; the handle's other calls around
a call."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, HsError, capi, synth
from tests import pssm_null_ref as ref
from tests import pssm_ref

pytestmark = pytest.mark.gpu


def _coords(A):
    if A == 20:
        return None
    rng = np.random.default_rng(77)
    base = synth.coords()
    if A < 20:
        return np.ascontiguousarray(base[:A])
    return np.ascontiguousarray(np.concatenate([base, rng.normal(0, 3, size=(A - 20, 8))]))


def _engine(k, A, codes=None, options=None):
    a, b = synth.make_planes(k, 2, 1, 200.0, seed=3)
    eng = Engine(k, 2, 1, 200.0, a, b, coords=_coords(A), options=options)
    if codes is not None:
        eng.index_build(codes)
    return eng


def _profiles(k, A, nm, seed=0):
    """nm profiles, their null and floors: log-odds, a plain one with a forbidden residue, a floor of its own each"""
    rng = np.random.default_rng(1000 * k + 10 * A + nm + seed)
    bg = rng.dirichlet(np.full(A, 2.0))
    S = ref.log_odds_profiles(rng, nm, k, A, bg)
    if nm > 1:
        S[1] = rng.normal(0, 2, size=(k, A))
        if k > 1:
            S[1, 1:, 0] = -1e30
    top = S.max(axis=2).sum(axis=1)
    t_lo = np.where(np.arange(nm) % 2 == 0, 0.0, top - 9.0)
    return S, bg, t_lo


def _every_bin(S, bg, t_lo, B, rng):
    """hits that look into every bin of every profile's tables, the ends of the grid and beyond, shuffled"""
    nm = S.shape[0]
    delta = capi.pssm_null_tables(S, bg, t_lo, B, want_lower=False)["delta"] if B <= 256 or nm <= 3 else None
    top = S.max(axis=2).sum(axis=1)
    hit_m, hit_s = [], []
    for m in range(nm):
        s = [t_lo[m], top[m], top[m] + 1.0, t_lo[m] - 1.0, np.inf, -np.inf, np.nextafter(t_lo[m], -np.inf)]
        if delta is not None:
            s += list(top[m] - (np.arange(B) + 0.5) * delta[m])
        else:
            s += list(np.linspace(t_lo[m], top[m], 40))
        hit_m += [m] * len(s)
        hit_s += s
    order = rng.permutation(len(hit_m))
    return np.array(hit_m, np.uint32)[order], np.array(hit_s)[order]


def _same(got, want, fields, what):
    for f in fields:
        assert ref.same_bits(got[f], want[f]), (what, f)


def _check(eng, S, bg, t_lo, B, what, ps=(1.0, 1e-2, 1e-5, 1e-300)):
    rng = np.random.default_rng(5)
    hit_m, hit_s = _every_bin(S, bg, t_lo, B, rng)
    want = capi.pssm_pvalue_host(S, bg, hit_m, hit_s, t_lo, B)
    got = eng.pssm_pvalue(S, hit_m, hit_s, bg=bg, t_lo=t_lo)
    _same(got, want, ("p_hi", "p_lo"), what)
    p = eng.profile()
    assert p["pssm_null_bins"] == B and p["pssm_null_profiles"] == S.shape[0], what
    # descending profile order
    order = np.argsort(-hit_m.astype(np.int64), kind="stable")
    got = eng.pssm_pvalue(S, hit_m[order], hit_s[order], bg=bg, t_lo=t_lo)
    assert ref.same_bits(got["p_hi"], want["p_hi"][order]) and ref.same_bits(got["p_lo"], want["p_lo"][order]), what
    for pv in ps:
        pp = np.full(S.shape[0], pv)
        pp[::3] = min(1.0, pv * 7)
        th = eng.pssm_pvalue_threshold(S, pp, bg=bg, t_lo=t_lo)
        wt = capi.pssm_threshold_host(S, bg, pp, t_lo, B)
        _same(th, wt, ("t", "p_hi", "p_lo"), (what, pv))
        assert np.array_equal(th["flag"], wt["flag"]), (what, pv)
    return want


@pytest.mark.parametrize("k,A,B", [(1, 20, 64), (3, 4, 64), (25, 20, 100), (25, 20, 4096), (75, 32, 8192)])
def test_outputs_equal_host_rule(k, A, B):
    S, bg, t_lo = _profiles(k, A, 3)
    eng = _engine(k, A, options={"pssm_null_bins": B})        # no index: the background is given
    try:
        _check(eng, S, bg, t_lo, B, (k, A, B))
        e = eng.pssm_pvalue_threshold(np.zeros((0, k, A)), 0.5, bg=bg)   # nm = 0 is an empty, successful call
        assert len(e["t"]) == 0
        e = eng.pssm_pvalue(S, np.zeros(0, np.uint32), np.zeros(0), bg=bg)
        assert len(e["p_hi"]) == 0
    finally:
        eng.close()


@pytest.mark.parametrize("nm", [1, 17, 33, 300])
def test_profile_counts(nm):
    k, A, B = 25, 20, 256
    S, bg, t_lo = _profiles(k, A, nm)
    eng = _engine(k, A, options={"pssm_null_bins": B})
    try:
        _check(eng, S, bg, t_lo, B, nm, ps=(1e-3,))
    finally:
        eng.close()


def _handmade():
    rng = np.random.default_rng(77)
    k, A = 3, 4
    base = rng.normal(0, 2, size=(k, A))
    top = float(base.max(axis=1).sum())
    S, t_lo = [], []
    S.append(np.full((k, A), 0.75)), t_lo.append(-1.0)                       # constant
    forb = base.copy()
    forb[1:, 2] = -1e30
    S.append(forb), t_lo.append(-5.0)                                        # a forbidden residue
    huge = base.copy()
    huge[0, 0], huge[1, 1], huge[2, 3] = 2.0 ** 100, -2.0 ** 100, 2.0 ** 100
    S.append(huge), t_lo.append(0.0)                                         # entries at +-2^100
    S.append(base), t_lo.append(top + 1.0)                                   # dead
    S.append(base), t_lo.append(top - 1e6)                                   # t_lo far below
    S.append(base), t_lo.append(top)                                         # t_lo exactly the maximum
    bg = rng.dirichlet(np.full(A, 2.0))
    return np.array(S), bg, np.array(t_lo)


@pytest.mark.parametrize("B", [64, 4096])
def test_handmade_profiles(B):
    S, bg, t_lo = _handmade()
    eng = _engine(3, 4, options={"pssm_null_bins": B})
    try:
        for zeros in (False, True):
            b = bg.copy()
            if zeros:
                b[1] = 0.0                                                   # bg with zeros
            _check(eng, S, b, t_lo, B, (B, zeros), ps=(1.0, 0.3, 1e-2, 1e-12))
    finally:
        eng.close()


def test_batches_pointers_and_sides_do_not_show():
    import torch
    k, A, B, nm = 25, 20, 256, 33
    S, bg, t_lo = _profiles(k, A, nm)
    hit_m, hit_s = _every_bin(S, bg, t_lo, B, np.random.default_rng(6))
    n = len(hit_m)
    pp = np.full(nm, 1e-3)
    want = capi.pssm_pvalue_host(S, bg, hit_m, hit_s, t_lo, B)
    wt = capi.pssm_threshold_host(S, bg, pp, t_lo, B)
    eng = _engine(k, A, options={"pssm_null_bins": B})
    try:
        for batch in (1, 16, 0):
            eng.set_option("query_batch", batch)
            _same(eng.pssm_pvalue(S, hit_m, hit_s, bg=bg, t_lo=t_lo), want, ("p_hi", "p_lo"), batch)
            th = eng.pssm_pvalue_threshold(S, pp, bg=bg, t_lo=t_lo)
            _same(th, wt, ("t", "p_hi", "p_lo"), batch)
            assert np.array_equal(th["flag"], wt["flag"])
            # the upper side alone
            up = eng.pssm_pvalue(S, hit_m, hit_s, bg=bg, t_lo=t_lo, want_lower=False)
            assert ref.same_bits(up["p_hi"], want["p_hi"]) and "p_lo" not in up
            up = eng.pssm_pvalue_threshold(S, pp, bg=bg, t_lo=t_lo, want_lower=False)
            assert ref.same_bits(up["t"], wt["t"]) and ref.same_bits(up["p_hi"], wt["p_hi"])
            # device pointers
            dS, dbg, dtl = torch.from_numpy(S).cuda(), torch.from_numpy(bg).cuda(), torch.from_numpy(t_lo).cuda()
            dm = torch.from_numpy(hit_m.astype(np.int32)).cuda()
            ds, dp = torch.from_numpy(hit_s).cuda(), torch.from_numpy(pp).cuda()
            dhi = torch.full((n + 1,), 7.0, dtype=torch.float64, device="cuda")
            dlo = torch.full((n + 1,), 7.0, dtype=torch.float64, device="cuda")
            dt, dth, dtl2 = (torch.full((nm + 1,), 7.0, dtype=torch.float64, device="cuda") for _ in range(3))
            dfl = torch.full((nm + 1,), 7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            eng.pssm_pvalue_dev(dS.data_ptr(), nm, dm.data_ptr(), ds.data_ptr(), n, dhi.data_ptr(), dlo.data_ptr(),
                                d_bg=dbg.data_ptr(), d_t_lo=dtl.data_ptr())
            assert ref.same_bits(dhi[:n].cpu().numpy(), want["p_hi"]) and ref.same_bits(dlo[:n].cpu().numpy(), want["p_lo"])
            assert float(dhi[n]) == 7.0 and float(dlo[n]) == 7.0
            dlo.fill_(7.0)
            torch.cuda.synchronize()
            eng.pssm_pvalue_dev(dS.data_ptr(), nm, dm.data_ptr(), ds.data_ptr(), n, dhi.data_ptr(), None,
                                d_bg=dbg.data_ptr(), d_t_lo=dtl.data_ptr())
            assert ref.same_bits(dhi[:n].cpu().numpy(), want["p_hi"]) and bool((dlo == 7.0).all())
            eng.pssm_pvalue_threshold_dev(dS.data_ptr(), dp.data_ptr(), nm, dt.data_ptr(), dth.data_ptr(), dfl.data_ptr(),
                                          d_p_lo=dtl2.data_ptr(), d_bg=dbg.data_ptr(), d_t_lo=dtl.data_ptr())
            assert ref.same_bits(dt[:nm].cpu().numpy(), wt["t"]) and ref.same_bits(dth[:nm].cpu().numpy(), wt["p_hi"])
            assert ref.same_bits(dtl2[:nm].cpu().numpy(), wt["p_lo"])
            assert np.array_equal(dfl[:nm].cpu().numpy().astype(np.uint32), wt["flag"])
            assert float(dt[nm]) == 7.0 and float(dth[nm]) == 7.0 and float(dtl2[nm]) == 7.0 and int(dfl[nm]) == 7
        # t_lo = None is 0 for every profile
        _same(eng.pssm_pvalue_threshold(S, pp, bg=bg), capi.pssm_threshold_host(S, bg, pp, None, B), ("t", "p_hi", "p_lo"),
              "t_lo None")
    finally:
        eng.close()


def test_index_background():
    """bg=None is hs_pssm_background of the index's residue counts: the explicit route, before and after an append."""
    k, A, B = 25, 20, 256
    rng = np.random.default_rng(12)
    codes = rng.choice(A, size=(6000, k), p=rng.dirichlet(np.full(A, 3.0))).astype(np.uint8)
    codes[5000:] = rng.integers(0, A, size=(1000, k))                  # the appended block moves the composition
    S, _, t_lo = _profiles(k, A, 5)
    eng = _engine(k, A, codes[:5000], options={"pssm_null_bins": B})
    try:
        for n in (5000, 6000):
            if n == 6000:
                eng.index_append(codes[5000:])
            counts = eng.pssm_hit_counts(np.zeros((1, k, A)), np.zeros(1))["counts"][0]
            assert counts.sum() == n * k
            bg = capi.pssm_background(counts)
            wt = capi.pssm_threshold_host(S, bg, 1e-3, t_lo, B)
            th = eng.pssm_pvalue_threshold(S, 1e-3, t_lo=t_lo)
            _same(th, wt, ("t", "p_hi", "p_lo"), n)
            _same(eng.pssm_pvalue_threshold(S, 1e-3, bg=bg, t_lo=t_lo), wt, ("t", "p_hi", "p_lo"), n)
            hit_m, hit_s = np.arange(5, dtype=np.uint32), wt["t"] + 0.25
            _same(eng.pssm_pvalue(S, hit_m, hit_s, t_lo=t_lo), capi.pssm_pvalue_host(S, bg, hit_m, hit_s, t_lo, B),
                  ("p_hi", "p_lo"), n)
            if n == 5000:
                first = wt["p_hi"].copy()
        assert not np.array_equal(first, wt["p_hi"])        # the composition moved, and the p-values with it
    finally:
        eng.close()


# The database of the null check: 20 000 iid 25-mers from a non-uniform bg, seed 2026.  Checked first on the CPU with
# numpy scores (tests/pssm_ref.py) at the host rule's thresholds, B = 4096: the four profiles' hit counts were
# 187, 195, 153, 184 inside [88 .. 90, 284] at p = 10^-2 and 22, 24, 18, 11 inside [-10, 47] at p = 10^-3.
def _null_db():
    k, A, n = 25, 20, 20000
    rng = np.random.default_rng(2026)
    bg = rng.dirichlet(np.full(A, 3.0))
    codes = rng.choice(A, size=(n, k), p=bg).astype(np.uint8)
    S = ref.log_odds_profiles(rng, 4, k, A, bg, conc=2.0)
    return k, A, n, bg, codes, S


def test_scan_at_the_threshold_and_the_null_database():
    import torch
    k, A, n, bg, codes, S = _null_db()
    nm = S.shape[0]
    eng = _engine(k, A, codes)
    try:
        dS, dbg = torch.from_numpy(S).cuda(), torch.from_numpy(bg).cuda()
        for p in (1e-2, 1e-3):
            dp = torch.full((nm,), p, dtype=torch.float64, device="cuda")
            dt, dhi, dlo = (torch.zeros(nm, dtype=torch.float64, device="cuda") for _ in range(3))
            dfl = torch.zeros(nm, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            eng.pssm_pvalue_threshold_dev(dS.data_ptr(), dp.data_ptr(), nm, dt.data_ptr(), dhi.data_ptr(), dfl.data_ptr(),
                                          d_p_lo=dlo.data_ptr(), d_bg=dbg.data_ptr())
            wt = capi.pssm_threshold_host(S, bg, p, None, 4096)
            assert ref.same_bits(dt.cpu().numpy(), wt["t"]) and not wt["flag"].any()
            # composition: the scan at t_p, then the p-values of its hits, all on the device
            cap = 4096
            dm, did = (torch.zeros(cap, dtype=torch.int32, device="cuda") for _ in range(2))
            dsc, dph = (torch.zeros(cap, dtype=torch.float64, device="cuda") for _ in range(2))
            dcnt = torch.zeros(nm, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            nh = eng.pssm_scan_dev(dS.data_ptr(), dt.data_ptr(), nm, dm.data_ptr(), did.data_ptr(), dsc.data_ptr(), cap,
                                   dcnt.data_ptr())
            eng.pssm_pvalue_dev(dS.data_ptr(), nm, dm.data_ptr(), dsc.data_ptr(), nh, dph.data_ptr(), None,
                                d_bg=dbg.data_ptr())
            ph = dph[:nh].cpu().numpy()
            assert nh > 0 and np.all(ph <= p) and np.all(ph > 0), p
            want = capi.pssm_pvalue_host(S, bg, dm[:nh].cpu().numpy().astype(np.uint32), dsc[:nh].cpu().numpy(), None, 4096)
            assert ref.same_bits(ph, want["p_hi"])
            # the null check
            cnt = dcnt.cpu().numpy()
            sc = pssm_ref.scores(S, codes)
            assert np.array_equal(cnt, (sc >= wt["t"][:, None]).sum(axis=1))
            lo = n * wt["p_lo"] - 6 * np.sqrt(n * wt["p_hi"])
            hi = n * wt["p_hi"] + 6 * np.sqrt(n * wt["p_hi"])
            assert np.all(lo <= cnt) and np.all(cnt <= hi), (p, cnt, lo, hi)
    finally:
        eng.close()


def test_refusals_write_nothing():
    import torch
    k, A, B, nm, n = 25, 20, 64, 3, 4
    S, bg, t_lo = _profiles(k, A, nm)
    hit_m, hit_s = np.array([0, 1, 2, 1], np.uint32), np.array([1.0, 2.0, 3.0, 4.0])
    pp = np.full(nm, 0.01)
    eng = _engine(k, A, options={"pssm_null_bins": B})
    try:
        lib, h = eng._lib, eng._h
        out = dict(hi=np.full(n, 7.0), lo=np.full(n, 7.0), t=np.full(nm, 7.0), thi=np.full(nm, 7.0), tlo=np.full(nm, 7.0),
                   fl=np.full(nm, 7, np.uint32))

        def v(a):
            return None if a is None else capi._vp(a)

        def pv(S_=S, b=bg, tl=t_lo, m=nm, hm=hit_m, hs=hit_s, nn=n, hi=out["hi"], lo=out["lo"]):
            return lib.hs_pssm_pvalue(h, v(S_), v(b), v(tl), C.c_uint64(m), v(hm), v(hs), C.c_uint64(nn), v(hi), v(lo))

        def th(S_=S, b=bg, tl=t_lo, p=pp, m=nm, t=out["t"], hi=out["thi"], lo=out["tlo"], fl=out["fl"]):
            return lib.hs_pssm_pvalue_threshold(h, v(S_), v(b), v(tl), v(p), C.c_uint64(m), v(t), v(hi), v(lo), v(fl))

        bad = capi.HS_ERR_INVALID
        for call in (pv, th):
            assert call(S_=None) == bad and call(m=1 << 27) == bad
            assert call(b=None) == capi.HS_ERR_STATE                       # no index to take the composition from
            for x in (np.nan, np.inf, 2.0 ** 101):
                S2 = S.copy()
                S2[2, 7, 5] = x
                assert call(S_=S2) == bad
            for x in (-0.01, 1.01, np.nan):
                b2 = bg.copy()
                b2[3] = x
                assert call(b=b2) == bad
            assert call(b=np.zeros(A)) == bad
            for x in (np.nan, -np.inf):
                assert call(tl=np.array([0.0, x, 0.0])) == bad
        assert pv(hm=np.array([0, 3, 2, 1], np.uint32)) == bad and pv(hs=np.array([1.0, np.nan, 3.0, 4.0])) == bad
        assert pv(hm=None) == bad and pv(hs=None) == bad and pv(hi=None) == bad and pv(m=0) == bad
        for x in (0.0, -1.0, 1.5, np.nan):
            assert th(p=np.array([0.5, x, 0.5])) == bad
        assert th(p=None) == bad and th(t=None) == bad and th(hi=None) == bad and th(fl=None) == bad
        assert pv(nn=0) == capi.HS_OK and th(m=0) == capi.HS_OK            # nothing to do: nothing written
        for name, a in out.items():
            assert np.all(a == 7), name
        assert pv() == capi.HS_OK and th() == capi.HS_OK

        # the _dev forms find the value errors on the device
        dS, dbg, dtl = torch.from_numpy(S).cuda(), torch.from_numpy(bg).cuda(), torch.from_numpy(t_lo).cuda()
        dm, ds = torch.from_numpy(hit_m.astype(np.int32)).cuda(), torch.from_numpy(hit_s).cuda()
        dp = torch.from_numpy(pp).cuda()
        outs = [torch.full((max(n, nm),), 9.0, dtype=torch.float64, device="cuda") for _ in range(5)]
        dfl = torch.full((nm,), 9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def untouched():
            torch.cuda.synchronize()
            return all(bool((o == 9.0).all()) for o in outs) and bool((dfl == 9).all())

        def dpv(S_=dS, b=dbg, tl=dtl, m_=dm, s_=ds):
            eng.pssm_pvalue_dev(S_.data_ptr(), nm, m_.data_ptr(), s_.data_ptr(), n, outs[0].data_ptr(), outs[1].data_ptr(),
                                d_bg=b.data_ptr(), d_t_lo=tl.data_ptr())

        def dth(S_=dS, b=dbg, tl=dtl, p_=dp):
            eng.pssm_pvalue_threshold_dev(S_.data_ptr(), p_.data_ptr(), nm, outs[2].data_ptr(), outs[3].data_ptr(),
                                          dfl.data_ptr(), d_p_lo=outs[4].data_ptr(), d_bg=b.data_ptr(),
                                          d_t_lo=tl.data_ptr())

        def mod(t, i, x):
            c = t.clone()
            c.view(-1)[i] = x
            torch.cuda.synchronize()
            return c

        for call in (dpv, dth):
            for kw in (dict(S_=mod(dS, 50, float("nan"))), dict(S_=mod(dS, 50, 2.0 ** 101)), dict(b=mod(dbg, 3, -0.5)),
                       dict(b=mod(dbg, 3, float("nan"))), dict(b=torch.zeros(A, dtype=torch.float64, device="cuda")),
                       dict(tl=mod(dtl, 1, float("inf")))):
                with pytest.raises(HsError) as e:
                    call(**kw)
                assert e.value.status == bad and untouched(), kw
        for kw in (dict(m_=mod(dm, 2, 3)), dict(s_=mod(ds, 0, float("nan")))):
            with pytest.raises(HsError) as e:
                dpv(**kw)
            assert e.value.status == bad and untouched()
        for x in (0.0, 1.5, float("nan")):
            with pytest.raises(HsError) as e:
                dth(p_=mod(dp, 2, x))
            assert e.value.status == bad and untouched()
        with pytest.raises(HsError) as e:                                  # bg = None without an index
            eng.pssm_pvalue_threshold_dev(dS.data_ptr(), dp.data_ptr(), nm, outs[2].data_ptr(), outs[3].data_ptr(),
                                          dfl.data_ptr())
        assert e.value.status == capi.HS_ERR_STATE and untouched()
        for name, value in (("pssm_null_bins", 63), ("pssm_null_bins", 8193)):
            with pytest.raises(HsError):
                eng.set_option(name, value)
        # an empty index has no composition
        info, _ = eng.index_build_windows(np.zeros(10, dtype=np.uint8), np.array([0, 4, 10], dtype=np.uint64))
        assert info["n"] == 0
        for a in out.values():
            a.fill(7)
        assert th(b=None) == bad and pv(b=None) == bad
        for name, a in out.items():
            assert np.all(a == 7), name
    finally:
        eng.close()


def test_other_calls_around_a_call():
    """hs_pssm_scan, hs_pssm_rank and hs_query_codes on the same handle give what they gave, before and after."""
    k = 25
    codes = synth.make_db(3000, k, seed=31)
    qcodes = codes[:40].copy()
    a, b = synth.make_planes(k, 4, 3, 120.0, seed=3)
    rng = np.random.default_rng(34)
    S = rng.integers(-12, 13, size=(17, k, 20)) / 4.0
    sc = pssm_ref.scores(S, codes)
    t = np.sort(sc, axis=1)[:, -40].copy()
    eng = Engine(k, 4, 3, 120.0, a, b)
    try:
        eng.index_build(codes)

        def others():
            return eng.pssm_scan(S, t), eng.pssm_rank(S, 40), eng.query_codes(qcodes, 45.0)

        before = others()
        got = eng.pssm_pvalue_threshold(S, 1e-4, t_lo=-10.0)
        p = eng.profile()
        assert p["pssm_null_bins"] == 4096 and p["pssm_null_profiles"] == 17 and p["ms_total"] > 0
        pv = eng.pssm_pvalue(S, before[0]["m"], before[0]["score"], t_lo=-10.0)
        assert np.all(pv["p_lo"] <= pv["p_hi"]) and np.all(pv["p_hi"] > 0)
        after = others()
        for x, y in zip(before, after):
            assert sorted(x) == sorted(y)
            for f in x:
                assert np.array_equal(x[f], y[f]), f
        assert eng.profile()["pssm_null_profiles"] == 0                  # another call's profile
        again = eng.pssm_pvalue_threshold(S, 1e-4, t_lo=-10.0)
        _same(again, got, ("t", "p_hi", "p_lo"), "again")
    finally:
        eng.close()
