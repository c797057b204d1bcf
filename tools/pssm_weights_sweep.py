"""hs_pssm_weighted_counts and hs_pssm_refine_weighted on one MI355X against the raw count sink and against the host
route, and the unchanged paths against the parent commit's library.

Shape (the protocol of tools/pssm_counts_sweep.py): 10^7 synthetic 25-mers (hsearch_amd/synth.py) in sequences of 300
windows (33 334 of them); the profiles are the Euclidean equivalents of search centres; nm = 16, 256, 4096.  Two
thresholds:
  bench   t = -R^2 at R = 40: about one hit per profile
  heavy   one value for all profiles, the median over the first 16 profiles of the 0.999 quantile of their scores over
          the first 200 000 k-mers: a profile hits of the order of 10^4 windows
Medians of --reps warm repetitions with [min, max], every worker a fresh process, the builds taking turns:
  (a) weighted_dev / weighted_one_dev   hs_pssm_weighted_counts_dev, every site / one site per sequence
  (b) counts_dev / counts_one_dev       hs_pssm_hit_counts_dev on the same handle: (a) - (b) is what the weights cost
  (c) host       hs_pssm_scan with host pointers + hs_pssm_weight_hits, PCIe and the host rule in it (skipped where the
                 host rule would sort more than --host-max-hits tuples)
  (d) refine     one hs_pssm_refine_weighted of 3 iterations (host pointers, every site, n_eff = the sites, the index's
                 composition as the background), from the log-odds of the heavy scan's raw counts at one threshold in
                 bits, as tools/pssm_counts_sweep.py starts its loop.  Recorded: ms, the scans run, the last one's hits.
  unchanged      with --parent-lib: hs_pssm_scan at the largest nm (bench threshold, host pointers),
                 hs_pssm_hit_counts_dev (heavy threshold, nm = --unchanged-counts-nm) and one bench step (hs_query_dev
                 at the bench shape), parent against this build; this build's median is to lie inside the parent's spread

Usage (GPU box): python tools/pssm_weights_sweep.py --out profiles/pssm_weights_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--nm", type=str, default="16,256,4096")
ap.add_argument("--seq-windows", type=int, default=300)
ap.add_argument("--heavy-quantile", type=float, default=0.999)
ap.add_argument("--host-max-hits", type=int, default=100_000_000)
ap.add_argument("--refine-iters", type=int, default=3)
ap.add_argument("--unchanged-counts-nm", type=int, default=256)
ap.add_argument("--bench-nq", type=int, default=100_000)
ap.add_argument("--bench-K", type=int, default=16)
ap.add_argument("--bench-L", type=int, default=8)
ap.add_argument("--bench-W", type=float, default=212.0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--turns", type=int, default=2, help="processes per arm and build, taking turns")
ap.add_argument("--worker-timeout", type=int, default=900)
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) weights | unchanged")
args = ap.parse_args()
NM = [int(x) for x in args.nm.split(",")]
ARMS = ("a_weighted_dev", "a_weighted_one_dev", "b_counts_dev", "b_counts_one_dev", "c_host", "d_refine")


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, capi, synth
    res = {"mode": mode, "gpu": torch.cuda.get_device_name(0)}
    state = {}

    def timed(call, reps=args.reps, warmup=args.warmup):
        for _ in range(warmup):
            call()
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        return summary(ms)

    codes = synth.make_db(args.n, args.k)
    centers, _ = synth.make_queries(codes, max(NM), jitter=0.05)
    coords = synth.coords()
    A = coords.shape[0]
    res["n"] = args.n
    dev = torch.device("cuda", 0)
    id_start = np.append(np.arange(0, args.n, args.seq_windows), args.n).astype(np.uint64)
    n_seq = len(id_start) - 1

    def profiles(nm):
        c = centers[:nm].reshape(nm, args.k, 1, 8)
        return np.ascontiguousarray(-((coords[None, None, :, :] - c) ** 2).sum(axis=3))

    def quantile_threshold(S16):
        """the contract's left-to-right sum over a sample, the median of the profiles' quantiles"""
        sample = codes[:200_000]
        acc = np.zeros((S16.shape[0], len(sample)))
        for p in range(args.k):
            acc = acc + S16[:, p, :][:, sample[:, p]]
        return float(np.median(np.quantile(acc, args.heavy_quantile, axis=1)))

    def scan_engine():   # the tables play no part in a scan: one small table
        a, b = synth.make_planes(args.k, 2, 1, args.bench_W)
        eng = Engine(args.k, 2, 1, args.bench_W, a, b)
        eng.index_build(codes)
        return eng

    t_heavy = quantile_threshold(profiles(min(16, max(NM))))
    res.update(n_seq=n_seq, t_heavy=t_heavy, t_bench=-args.R * args.R)
    d_ids = torch.from_numpy(id_start.astype(np.int64)).to(dev)
    if mode == "weights":
        eng = scan_engine()
        bg = capi.pssm_background(eng.pssm_hit_counts(np.zeros((1, args.k, A)), np.zeros(1))["counts"][0])
        for nm in NM:
            S = profiles(nm)
            d_S = torch.from_numpy(S).to(dev)
            d_counts = torch.empty((nm, args.k, A), dtype=torch.int32, device=dev)
            d_wc = torch.empty((nm, args.k, A), dtype=torch.int64, device=dev)
            d_ws, d_cnt, d_used = (torch.empty(nm, dtype=torch.int64, device=dev) for _ in range(3))
            d_dis = torch.empty(nm, dtype=torch.int32, device=dev)
            for name, tv in (("bench", -args.R * args.R), ("heavy", t_heavy)):
                t = np.full(nm, tv)
                d_t = torch.from_numpy(t).to(dev)
                torch.cuda.synchronize()
                row = {"t": tv}
                for arm, ids, ns in (("a_weighted_dev", None, 0), ("a_weighted_one_dev", d_ids.data_ptr(), n_seq)):
                    def weighted_dev():
                        state["a"] = eng.pssm_weighted_counts_dev(d_S.data_ptr(), d_t.data_ptr(), nm, d_wc.data_ptr(), ids,
                                                                  ns, d_counts.data_ptr(), d_ws.data_ptr(),
                                                                  d_dis.data_ptr(), d_cnt.data_ptr(), d_used.data_ptr())
                    row[arm] = timed(weighted_dev)
                    p = eng.profile()
                    row[arm].update(device_ms=p["ms_total"], finalize_ms=p["ms_finalize"], sites=p["pssm_weight_sites"],
                                    items=p["pssm_weight_items"])
                    assert int(d_used.sum()) == p["pssm_weight_sites"] and int(d_cnt.sum()) == state["a"]
                    if ids is None:
                        state["wcounts"] = d_wc.cpu().numpy().view(np.uint64)
                        state["counts"] = d_counts.cpu().numpy().astype(np.uint32)
                n_hits = state["a"]
                for arm, ids, ns in (("b_counts_dev", None, 0), ("b_counts_one_dev", d_ids.data_ptr(), n_seq)):
                    def counts_dev():
                        state["b"] = eng.pssm_hit_counts_dev(d_S.data_ptr(), d_t.data_ptr(), nm, d_counts.data_ptr(), ids,
                                                             ns, d_cnt.data_ptr(), d_used.data_ptr())
                    row[arm] = timed(counts_dev)
                    p = eng.profile()
                    row[arm].update(device_ms=p["ms_total"], finalize_ms=p["ms_finalize"])
                    assert state["b"] == n_hits
                if n_hits <= args.host_max_hits:
                    def host():
                        r = eng.pssm_scan(S, t, cap=n_hits + 1, want_counts=False)
                        state["c"] = capi.pssm_weight_hits(codes, A, r["m"], r["id"], r["score"], nm)
                    row["c_host"] = timed(host)
                    assert np.array_equal(state["c"]["wcounts"], state["wcounts"])
                else:
                    row["c_host_skipped"] = "the host rule would sort %d tuples" % n_hits
                row.update(hits=n_hits, survivors=p["pssm_survivors"])
                if name == "heavy":   # (d): from the log-odds of the raw counts, at a threshold in bits
                    S1 = capi.pssm_log_odds_exact(state["counts"], bg, 1.0)
                    t1 = np.full(nm, quantile_threshold(S1[:16]))

                    def refine():
                        state["d"] = eng.pssm_refine_weighted(S1, args.refine_iters, t=t1, background=bg)
                    row["d_refine"] = timed(refine)
                    row["d_refine"].update(t_bits=float(t1[0]), iters=state["d"]["iters"],
                                           converged=state["d"]["converged"], last_hits=eng.profile()["hits"],
                                           sites=int(state["d"]["used"].sum()))
                res["%s_%d" % (name, nm)] = row
            del d_S, d_counts, d_wc
        eng.close()
    else:
        eng = scan_engine()
        nm = max(NM)
        S, t = profiles(nm), np.full(nm, -args.R * args.R)
        cap = len(eng.pssm_scan(S, t, want_counts=False)["m"]) + 1
        res["scan_%d" % nm] = timed(lambda: eng.pssm_scan(S, t, cap=cap, want_counts=False))
        nm = min(args.unchanged_counts_nm, max(NM))
        d_S = torch.from_numpy(profiles(nm)).to(dev)
        d_t = torch.from_numpy(np.full(nm, t_heavy)).to(dev)
        d_counts = torch.empty((nm, args.k, A), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        res["hit_counts_dev_%d" % nm] = timed(lambda: eng.pssm_hit_counts_dev(d_S.data_ptr(), d_t.data_ptr(), nm,
                                                                              d_counts.data_ptr()))
        eng.close()
        a, b = synth.make_planes(args.k, args.bench_K, args.bench_L, args.bench_W)
        q, _ = synth.make_queries(codes, args.bench_nq, jitter=0.05)
        eng = Engine(args.k, args.bench_K, args.bench_L, args.bench_W, a, b)
        eng.index_build(codes)
        d_c = torch.from_numpy(q).to(dev)
        cap = 64 * args.bench_nq
        d_q, d_id, d_tb = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
        d_d = torch.empty(cap, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def step():
            state["hits"] = eng.query_dev(d_c.data_ptr(), args.bench_nq, args.R, d_q.data_ptr(), d_id.data_ptr(),
                                          d_tb.data_ptr(), d_d.data_ptr(), cap)
        res["search_step"] = timed(step)
        res["n_hits"] = state["hits"]
        eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(mode, lib):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--nm", args.nm]
    for name in ("n", "k", "R", "seq_windows", "heavy_quantile", "host_max_hits", "refine_iters", "unchanged_counts_nm",
                 "bench_nq", "bench_K", "bench_L", "bench_W", "warmup", "reps"):
        argv += ["--" + name.replace("_", "-"), repr(getattr(args, name))]
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=args.worker_timeout)
    if r.returncode != 0:   # a failed measurement ends the sweep: nothing else is started
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("worker failed with status %d" % r.returncode)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


if args.worker:
    worker(args.worker)
    sys.exit(0)
res = {"shape": {k: v for k, v in vars(args).items() if k not in ("worker", "out")},
       "taken": time.strftime("%Y-%m-%d"), "runs": [], "summary": {}}
order = []
for _ in range(args.turns):
    order.append(("weights", "here"))
    if args.parent_lib:
        order += [("unchanged", "parent"), ("unchanged", "here")]
for mode, which in order:
    row = run_worker(mode, args.parent_lib if which == "parent" else None)
    row.update(build=which)
    print(json.dumps(row), file=sys.stderr, flush=True)
    res["runs"].append(row)
    if args.out:   # what was measured so far survives a later worker's failure
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

s = res["summary"]


def pooled(rows):
    if not rows:
        return None
    return {"median_ms": statistics.median(r["median_ms"] for r in rows), "min_ms": min(r["min_ms"] for r in rows),
            "max_ms": max(r["max_ms"] for r in rows), "turns": len(rows)}


runs = [r for r in res["runs"] if r["mode"] == "weights"]
if runs:
    s["t_heavy"], s["n_seq"] = runs[-1]["t_heavy"], runs[-1]["n_seq"]
for nm in NM:
    for name in ("bench", "heavy"):
        cases = [r["%s_%d" % (name, nm)] for r in runs if "%s_%d" % (name, nm) in r]
        if not cases:
            continue
        out = {f: cases[-1][f] for f in ("t", "hits", "survivors", "c_host_skipped") if f in cases[-1]}
        for arm in ARMS:
            p = pooled([c[arm] for c in cases if arm in c])
            if p:
                for f in ("finalize_ms", "sites", "items", "iters", "converged", "last_hits", "t_bits"):
                    if f in cases[-1][arm]:
                        p[f] = cases[-1][arm][f]
                out[arm] = p
        out["a_minus_b_ms"] = out["a_weighted_dev"]["median_ms"] - out["b_counts_dev"]["median_ms"]
        out["a_one_minus_b_one_ms"] = out["a_weighted_one_dev"]["median_ms"] - out["b_counts_one_dev"]["median_ms"]
        out["sink_ms"] = {"weighted": out["a_weighted_dev"]["finalize_ms"], "counts": out["b_counts_dev"]["finalize_ms"]}
        if "c_host" in out:
            out["c_over_a"] = out["c_host"]["median_ms"] / out["a_weighted_dev"]["median_ms"]
        s["%s_%d" % (name, nm)] = out
unchanged = sorted({w for r in res["runs"] if r["mode"] == "unchanged" for w in r
                    if w == "search_step" or w.startswith("scan_") or w.startswith("hit_counts_dev_")})
for what in unchanged:
    p = pooled([r[what] for r in res["runs"] if r["mode"] == "unchanged" and r["build"] == "parent" and what in r])
    h = pooled([r[what] for r in res["runs"] if r["mode"] == "unchanged" and r["build"] == "here" and what in r])
    if p and h:
        s["unchanged_%s_parent" % what], s["unchanged_%s_here" % what] = p, h
        s["unchanged_%s_verdict" % what] = ("inside" if p["min_ms"] <= h["median_ms"] <= p["max_ms"] else
                                               "faster" if h["median_ms"] < p["min_ms"] else "slower")
if res["runs"]:
    res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
