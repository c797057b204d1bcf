"""Multi-probe search on the GPU (hs_set_multiprobe / hs_probe_buckets) against the numpy restatement
(tests/multiprobe_ref.py): the probe sequence bit for bit, the hits exactly, across the filter and grouping paths."""
import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import multiprobe_ref as mp

pytestmark = pytest.mark.gpu

_FIELDS = ("q", "id", "table", "dist", "cand")


def _assert_same(got, want, what=""):
    for f in _FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)


@pytest.mark.parametrize("k,K,L,W", [(25, 16, 8, 200.0), (25, 20, 3, 37.5), (15, 6, 5, 7.0), (39, 5, 2, 0.9),
                                     (25, 32, 2, 100.0)])
def test_probe_sequence_matches_restatement(oracle, k, K, L, W):
    a, b = synth.make_planes(k, K, L, W)
    codes = synth.make_db(150, k, seed=21)
    kmers = oracle.embed_codes(codes)
    rng = np.random.default_rng(8)
    jittered = kmers + rng.normal(0, 0.4, size=kmers.shape)
    eng = Engine(k, K, L, W, a, b)
    for pts in (kmers, jittered):
        b0, v0 = eng.probe_buckets(pts)
        assert v0.all() and np.array_equal(b0[:, :, 0, :], eng.hash_points(pts))
        for T in (1, 7, 63):
            if T > 3 ** K - 1:
                continue
            eng.set_multiprobe(T)
            got_b, got_v = eng.probe_buckets(pts)
            want_b, want_v = mp.probe_buckets(oracle, a, b, W, pts, T)
            assert np.array_equal(got_v, want_v), T
            assert np.array_equal(got_b, want_b), T
        eng.set_multiprobe(0)
    eng.close()


def _case(k, n=24000, nq=500, K=8, L=4, W=120.0):
    a, b = synth.make_planes(k, K, L, W)
    codes = synth.make_db(n, k)
    qcodes, _ = synth.make_query_codes(codes, nq, seed=7)
    centers, _ = synth.make_queries(codes, nq, jitter=0.25, seed=9)
    return a, b, W, codes, qcodes, centers


@pytest.mark.parametrize("k,R", [(15, 30.0), (25, 40.0), (39, 50.0)])
def test_hits_match_restatement_across_paths(oracle, k, R):
    T = 6
    a, b, W, codes, qcodes, centers = _case(k)
    K, L = a.shape[1], a.shape[0]
    db = oracle.embed_codes(codes)
    want = mp.search(oracle, a, b, W, db, centers, R, T)
    want_c = mp.search(oracle, a, b, W, db, synth.embed(qcodes), R, T)
    assert len(want["q"]) > 0 and len(want_c["q"]) > 0
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    eng.set_multiprobe(T)
    runs = [("verify", m, {}) for m in ("auto", "stream", "join", "join16")]
    runs += [("hash", m, {}) for m in ("auto", "exact", "mfma")]
    runs += [("opt", None, dict(seg_mode=1)), ("opt", None, dict(seg_mode=2)),
             ("opt", None, dict(join_resident=1)), ("opt", None, dict(join_resident=2)),
             ("opt", None, dict(wide_rows=1)), ("opt", None, dict(query_batch=37))]
    for what, mode, opts in runs:
        if what == "verify":
            eng.set_verify_mode(mode)
        elif what == "hash":
            eng.set_hash_mode(mode)
        for name, value in opts.items():
            eng.set_option(name, value)
        _assert_same(eng.query(centers, R), want, (what, mode, opts))
        _assert_same(eng.query_codes(qcodes, R), want_c, (what, mode, opts, "codes"))
        assert eng.profile()["candidates"] == int(want_c["cand"].sum())
        for name in opts:
            eng.set_option(name, {"seg_mode": 0, "join_resident": 0, "wide_rows": 0, "query_batch": 0}[name])
        eng.set_verify_mode("auto")
        eng.set_hash_mode("auto")
    eng.close()


def test_properties(oracle):
    k, R = 25, 40.0
    a, b, W, codes, _, centers = _case(k)
    K, L = a.shape[1], a.shape[0]
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    fresh = Engine(k, K, L, W, a, b)
    fresh.index_build(codes)
    base = fresh.query(centers, R)
    eng.set_multiprobe(5)
    eng.query(centers, R)
    eng.set_multiprobe(0)
    _assert_same(eng.query(centers, R), base, "back to 0")
    prev = base
    for T in (4, 8, 12):
        eng.set_multiprobe(T)
        cur = eng.query(centers, R)
        before = dict(zip(zip(prev["q"], prev["id"]), prev["table"]))
        after = dict(zip(zip(cur["q"], cur["id"]), cur["table"]))
        assert set(before) <= set(after), T
        assert all(after[p] <= before[p] for p in before), T
        prev = cur
    # the setting survives a rebuild
    eng.index_build(codes)
    _assert_same(eng.query(centers, R), prev, "after rebuild")
    with pytest.raises(capi.HsError):
        eng.set_multiprobe(64)
    one = Engine(k, 1, 2, W, a[:2, :1], b[:2, :1])
    one.set_multiprobe(2)
    with pytest.raises(capi.HsError):
        one.set_multiprobe(3)
    one.close()
    fresh.close()
    eng.close()


def test_bucket_partition_with_extra_probes():
    import torch
    k, R, T = 25, 40.0, 8
    a, b, W, codes, _, centers = _case(k)
    K, L = a.shape[1], a.shape[0]
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    eng.set_multiprobe(T)
    full = eng.query(centers, R)
    for n_parts in (2, 3):
        lists = []
        for part in range(n_parts):
            eng.set_bucket_partition(part, n_parts)
            lists.append(eng.query(centers, R))
        eng.set_bucket_partition(0, 1)
        cat = {f: np.concatenate([x[f] for x in lists]) for f in ("q", "id", "table", "dist")}
        dev = {f: torch.from_numpy(cat[f].astype(np.int32) if f != "dist" else cat[f]).cuda()
               for f in cat}
        torch.cuda.synchronize()
        n = eng.merge_first_table_dev(dev["q"].data_ptr(), dev["id"].data_ptr(), dev["table"].data_ptr(),
                                      dev["dist"].data_ptr(), len(cat["q"]))
        for f in ("q", "id", "table", "dist"):
            got = dev[f][:n].cpu().numpy()
            assert np.array_equal(got.astype(full[f].dtype), full[f]), (n_parts, f)
    eng.close()


def test_larger_index_recall(oracle):
    """configs[1]'s index size (10^6 k-mers here, L = 4): T = 8 finds a superset of T = 0, all within R."""
    k, K, L, W, R = 25, 16, 4, 160.0, 40.0
    a, b = synth.make_planes(k, K, L, W)
    codes = synth.make_db(1_000_000, k)
    centers, _ = synth.make_queries(codes, 500, jitter=0.25, seed=12)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    h0 = eng.query(centers, R)
    eng.set_multiprobe(8)
    h8 = eng.query(centers, R)
    assert (h8["dist"] <= R).all()
    p0, p8 = set(zip(h0["q"], h0["id"])), set(zip(h8["q"], h8["id"]))
    assert p0 <= p8 and len(p8) > len(p0)
    truth = eng.bruteforce(centers, R)
    pt = set(zip(truth["q"], truth["id"]))
    assert p8 <= pt
    assert len(p8 & pt) >= len(p0 & pt)
    eng.close()


def test_cli_probes_flag(tmp_path, oracle):
    """hs_motif_both_points -M: 0 writes what the run without the flag writes; 6 writes the restatement's hits in the
    reference's format, plain and over two loopback ranks sharing the buckets (and the tables)."""
    import subprocess
    from tests.test_host_cli import _bin, _write_points
    k, K, L, W, R, seed = 25, 6, 5, 140.0, 40.0, 81
    rng = np.random.default_rng(13)
    codes = rng.integers(0, 20, size=(3000, k), dtype=np.uint8)
    pts = oracle.embed_codes(codes)
    qcodes = codes[rng.choice(len(codes), 90, replace=False)].copy()
    for row in qcodes:
        for _ in range(int(rng.integers(0, 4))):
            row[rng.integers(0, k)] = rng.integers(0, 20)
    centers = oracle.embed_codes(qcodes)
    db, cen, planes = [str(tmp_path / n) for n in ("db.points", "cen.points", "planes.bin")]
    _write_points(db, pts)
    with open(cen, "w") as f:
        for i, row in enumerate(centers):
            f.write("c%d\n" % i + " ".join("%.17g" % v for v in row) + "\n")
    common = ["-d", db, "-c", cen, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "-T", repr(R),
              "--seed", str(seed)]

    def run(out, *extra):
        r = subprocess.run([_bin(), "-o", str(tmp_path / out)] + common + list(extra), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return open(tmp_path / out).read()
    plain = run("plain", "--planes-out", planes)
    assert run("m0", "-M", "0") == plain
    raw = np.fromfile(planes, dtype=np.float64)
    a = raw[:L * K * 8 * k].reshape(L, K, 8 * k)
    b = raw[L * K * 8 * k:].reshape(L, K)
    want = mp.search(oracle, a, b, W, pts, centers, R, 6)
    m6 = run("m6", "-M", "6")
    rows = [ln.split() for ln in m6.splitlines()]
    assert [r[:2] for r in rows] == [["c%d" % q, "p%d" % i] for q, i in zip(want["q"], want["id"])]
    assert len(rows) > len(plain.splitlines())
    for part in ("buckets", "tables", "queries"):
        got = run("m6_" + part, "-M", "6", "--gpus", "2", "--transport", "loopback", "--partition", part)
        assert got == m6, part
