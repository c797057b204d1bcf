"""hs_pssm_pvalue / hs_pssm_pvalue_threshold on one MI355X against the route without them, and the unchanged paths
against the parent commit's library.  The protocol of tools/pssm_rank_sweep.py: medians of --reps warm repetitions with
[min, max], every worker a fresh process, the builds taking turns.  Profiles: Dirichlet(0.5) columns as log-odds in
bits against the database's residue composition, k = 25, alphabet 20, t_lo = 0.

  (a) threshold  hs_pssm_pvalue_threshold_dev, nm x B, both sides, with its phases (ms_hash: tables + convolution,
                 ms_finalize: the threshold search); the convolution's LDS read rate nm * 2 * k * alphabet * B * 8 bytes
                 over ms_hash, against the guide's aggregate figure for 8-byte reads (about 150 TB/s)
  (b) upper      the upper side alone through the lookup form: hs_pssm_pvalue_dev on one hit per profile, p_lo = NULL
  (c) host       hs_pssm_threshold_host on one CPU thread at --host-nm profiles (it is linear in nm): the route
                 without this work
  (d) scan       for scale: hs_pssm_scan_dev at t_p (p = --scan-p) over --n synthetic 25-mers, at the largest nm
  (e) hits       hs_pssm_pvalue_dev on (d)'s hit list at the p that returns about 10^6 hits of --hits-nm profiles, against copying the list
                 to the host and running hs_pssm_pvalue_host
  ratio          p_hi / p_lo at the thresholds of p = 10^-4, 10^-6, 10^-8 per B (median and range over 64 profiles)
  unchanged      with --parent-lib: hs_pssm_scan at the largest nm, hs_pssm_rank_dev at nm = 256, rank 10^4, and one
                 bench step (hs_query_dev at the bench shape), parent against this build; this build's median is to lie
                 inside the parent's own spread

Usage (GPU box): python tools/pssm_null_sweep.py --out profiles/pssm_null_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--nm", type=str, default="16,256,4096")
ap.add_argument("--bins", type=str, default="1024,4096,8192")
ap.add_argument("--p", type=float, default=1e-6)
ap.add_argument("--host-nm", type=int, default=16)
ap.add_argument("--hits-nm", type=int, default=16)
ap.add_argument("--scan-p", type=float, default=1e-4)
ap.add_argument("--bench-nq", type=int, default=100_000)
ap.add_argument("--bench-K", type=int, default=16)
ap.add_argument("--bench-L", type=int, default=8)
ap.add_argument("--bench-W", type=float, default=212.0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--turns", type=int, default=2, help="processes per arm and build, taking turns")
ap.add_argument("--worker-limit", type=int, default=420, help="seconds a worker process may run")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) null | unchanged")
args = ap.parse_args()
NM = [int(x) for x in args.nm.split(",")]
BINS = [int(x) for x in args.bins.split(",")]
A = 20
LDS_AGGREGATE_TBS = 150.0   # every CU streaming 8-byte LDS reads at about 2.4 GHz


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, HsError, capi, synth
    res = {"mode": mode, "gpu": torch.cuda.get_device_name(0), "n": args.n}
    state = {}
    dev = torch.device("cuda", 0)

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

    def scan_engine(options=None):   # the tables play no part in a scan: one small table
        a, b = synth.make_planes(args.k, 2, 1, args.bench_W)
        eng = Engine(args.k, 2, 1, args.bench_W, a, b, options=options)
        eng.index_build(codes)
        return eng

    if mode == "null":
        rng = np.random.default_rng(7)
        eng = scan_engine()
        # the null is the database's residue composition, so that (d) and (e) scan a database drawn from it
        bg = capi.pssm_background(eng.pssm_hit_counts(np.zeros((1, args.k, A)), np.zeros(1))["counts"][0])
        f = rng.dirichlet(np.full(A, 0.5), size=(max(NM), args.k))
        S_all = np.ascontiguousarray(np.log2(np.maximum(f, 1e-6) / bg))
        d_bg = torch.from_numpy(bg).to(dev)
        for B in BINS:
            eng.set_option("pssm_null_bins", B)
            for nm in NM:
                d_S = torch.from_numpy(S_all[:nm]).to(dev)
                d_p = torch.full((nm,), args.p, dtype=torch.float64, device=dev)
                d_t, d_hi, d_lo = (torch.empty(nm, dtype=torch.float64, device=dev) for _ in range(3))
                d_fl = torch.empty(nm, dtype=torch.int32, device=dev)
                d_m = torch.arange(nm, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                row = timed(lambda: eng.pssm_pvalue_threshold_dev(d_S.data_ptr(), d_p.data_ptr(), nm, d_t.data_ptr(),
                                                                  d_hi.data_ptr(), d_fl.data_ptr(), d_p_lo=d_lo.data_ptr(),
                                                                  d_bg=d_bg.data_ptr()))
                pr = eng.profile()
                tbs = nm * 2 * args.k * A * B * 8 / (pr["ms_hash"] * 1e-3) / 1e12
                row.update(tables_conv_ms=pr["ms_hash"], search_ms=pr["ms_finalize"], device_ms=pr["ms_total"],
                           lds_read_TBs=tbs, lds_share_of_aggregate=tbs / LDS_AGGREGATE_TBS,
                           flags=[int((d_fl == v).sum().item()) for v in range(3)])
                res["a_%d_%d" % (nm, B)] = row
                row = timed(lambda: eng.pssm_pvalue_dev(d_S.data_ptr(), nm, d_m.data_ptr(), d_t.data_ptr(), nm,
                                                        d_hi.data_ptr(), None, d_bg=d_bg.data_ptr()))
                pr = eng.profile()
                row.update(tables_conv_ms=pr["ms_hash"], lookup_ms=pr["ms_finalize"])
                res["b_%d_%d" % (nm, B)] = row
            hn = args.host_nm
            row = timed(lambda: capi.pssm_threshold_host(S_all[:hn], bg, args.p, None, B), reps=3, warmup=1)
            row.update(nm=hn, ms_per_profile=row["median_ms"] / hn)
            res["c_host_%d" % B] = row
            ratios = {}
            for p in (1e-4, 1e-6, 1e-8):
                th = eng.pssm_pvalue_threshold(S_all[:64], p, bg=bg)
                ok = (th["flag"] == 0) & (th["p_lo"] > 0)
                r = th["p_hi"][ok] / th["p_lo"][ok]
                ratios["%g" % p] = dict(profiles=int(ok.sum()), median=float(np.median(r)) if ok.any() else None,
                                        min=float(r.min()) if ok.any() else None, max=float(r.max()) if ok.any() else None)
            res["ratio_%d" % B] = ratios
        # (d), (e) at the default grid
        eng.set_option("pssm_null_bins", 4096)
        for name, nm, p in (("d_scan", NM[-1], args.scan_p), ("e_hits", args.hits_nm, 1e6 / (args.hits_nm * args.n))):
            S = S_all[:nm]
            d_S = torch.from_numpy(S).to(dev)
            t = eng.pssm_pvalue_threshold(S, p, bg=bg)["t"]
            d_t = torch.from_numpy(t).to(dev)
            torch.cuda.synchronize()
            try:     # capacity 0 asks for the count
                cap = eng.pssm_scan_dev(d_S.data_ptr(), d_t.data_ptr(), nm, 0, 0, 0, 0) + 1
            except HsError as e:
                cap = int(e.n_hits) + 1
            d_m, d_id = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
            d_sc, d_hi = (torch.empty(cap, dtype=torch.float64, device=dev) for _ in range(2))
            torch.cuda.synchronize()

            def scan():
                state["hits"] = eng.pssm_scan_dev(d_S.data_ptr(), d_t.data_ptr(), nm, d_m.data_ptr(), d_id.data_ptr(),
                                                  d_sc.data_ptr(), cap)
            row = timed(scan)
            row.update(hits=state["hits"], nm=nm, p=p, expected_at_most=p * nm * args.n)
            res[name + "_scan"] = row
            if name == "e_hits":
                nh = state["hits"]
                row = timed(lambda: eng.pssm_pvalue_dev(d_S.data_ptr(), nm, d_m.data_ptr(), d_sc.data_ptr(), nh,
                                                        d_hi.data_ptr(), None, d_bg=d_bg.data_ptr()))
                row.update(hits=nh)
                res["e_pvalue_dev"] = row

                def host_route():
                    m = d_m[:nh].cpu().numpy().astype(np.uint32)
                    sc = d_sc[:nh].cpu().numpy()
                    state["p_hi"] = capi.pssm_pvalue_host(S, bg, m, sc, None, 4096, want_lower=False)["p_hi"]
                row = timed(host_route, reps=3, warmup=1)
                row.update(hits=nh, same_bits=bool(np.array_equal(state["p_hi"].view(np.uint64),
                                                                  d_hi[:nh].cpu().numpy().view(np.uint64))))
                res["e_copy_and_host"] = row
        eng.close()
    else:
        eng = scan_engine()
        centers, _ = synth.make_queries(codes, max(NM + [256]), jitter=0.05)
        coords = synth.coords()

        def profiles(nm):
            c = centers[:nm].reshape(nm, args.k, 1, 8)
            return np.ascontiguousarray(-((coords[None, None, :, :] - c) ** 2).sum(axis=3))

        nm = NM[-1]
        S, t = profiles(nm), np.full(nm, -args.R * args.R)
        cap = len(eng.pssm_scan(S, t, want_counts=False)["m"]) + 1
        res["scan_%d" % nm] = timed(lambda: eng.pssm_scan(S, t, cap=cap, want_counts=False))
        d_S = torch.from_numpy(profiles(256)).to(dev)
        d_r = torch.full((256,), 10000, dtype=torch.int64, device=dev)
        d_t = torch.empty(256, dtype=torch.float64, device=dev)
        d_ge, d_gt = (torch.empty(256, dtype=torch.int64, device=dev) for _ in range(2))
        torch.cuda.synchronize()
        res["rank_256_10000"] = timed(lambda: eng.pssm_rank_dev(d_S.data_ptr(), d_r.data_ptr(), 256, d_t.data_ptr(),
                                                                d_ge.data_ptr(), d_gt.data_ptr()))
        eng.close()
        a, b = synth.make_planes(args.k, args.bench_K, args.bench_L, args.bench_W)
        q, _ = synth.make_queries(codes, args.bench_nq, jitter=0.05)
        eng = Engine(args.k, args.bench_K, args.bench_L, args.bench_W, a, b)
        eng.index_build(codes)
        d_c = torch.from_numpy(q).to(dev)
        cap = 64 * args.bench_nq
        d_q, d_id, d_tt = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
        d_d = torch.empty(cap, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def step():
            state["hits"] = eng.query_dev(d_c.data_ptr(), args.bench_nq, args.R, d_q.data_ptr(), d_id.data_ptr(),
                                          d_tt.data_ptr(), d_d.data_ptr(), cap)
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
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--nm", args.nm, "--bins", args.bins]
    for name in ("n", "k", "R", "p", "host_nm", "hits_nm", "scan_p", "bench_nq", "bench_K", "bench_L", "bench_W", "warmup",
                 "reps"):
        argv += ["--" + name.replace("_", "-"), repr(getattr(args, name))]
    # every GPU step under a time limit of its own; a failed measurement ends the sweep: nothing else is started
    r = subprocess.run(["timeout", "-k", "10", str(args.worker_limit)] + argv, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("worker %s failed with status %d" % (mode, r.returncode))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


if args.worker:
    worker(args.worker)
    sys.exit(0)
shape = {k: v for k, v in vars(args).items() if k not in ("worker", "out", "parent_lib")}
shape["parent_lib"] = "the parent commit's libhsearch_amd.so" if args.parent_lib else None
res = {"shape": shape, "taken": time.strftime("%Y-%m-%d"), "runs": [], "summary": {}}
order = []
for _ in range(args.turns):
    order.append(("null", "here"))
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


def pooled(mode, which, what):
    rows = [r[what] for r in res["runs"] if r["mode"] == mode and r["build"] == which and what in r]
    if not rows:
        return None
    out = {"median_ms": statistics.median(r["median_ms"] for r in rows), "min_ms": min(r["min_ms"] for r in rows),
           "max_ms": max(r["max_ms"] for r in rows), "turns": len(rows)}
    out.update({f: v for f, v in rows[-1].items() if f not in ("median_ms", "min_ms", "max_ms", "reps")})
    return out


names = ["%s_%d_%d" % (arm, nm, B) for arm in "ab" for nm in NM for B in BINS]
names += ["c_host_%d" % B for B in BINS] + ["d_scan_scan", "e_hits_scan", "e_pvalue_dev", "e_copy_and_host"]
for name in names:
    r = pooled("null", "here", name)
    if r:
        s[name] = r
for B in BINS:
    rows = [r["ratio_%d" % B] for r in res["runs"] if r["mode"] == "null" and "ratio_%d" % B in r]
    if rows:
        s["ratio_%d" % B] = rows[-1]
    c = s.get("c_host_%d" % B)
    for nm in NM:
        a = s.get("a_%d_%d" % (nm, B))
        if a and c:
            s["host_over_a_%d_%d" % (nm, B)] = c["ms_per_profile"] * nm / a["median_ms"]
if "e_pvalue_dev" in s and "e_copy_and_host" in s:
    s["e_host_over_dev"] = s["e_copy_and_host"]["median_ms"] / s["e_pvalue_dev"]["median_ms"]
for what in ("scan_%d" % NM[-1], "rank_256_10000", "search_step"):
    p, h = pooled("unchanged", "parent", what), pooled("unchanged", "here", what)
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
