"""hs_pssm_compare on one MI355X: the call with and without its int8 MFMA filter, the route without it (the host rule
on one CPU thread), and the unchanged paths against the parent commit's library.  The protocol of
tools/pssm_null_sweep.py: medians of --reps warm repetitions with [min, max], every worker a fresh process, the builds
taking turns.  Profiles: k = 25, alphabet 20, Pearson columns of Dirichlet(0.3) columns; a fifth of them in planted
families of 6 windows of one master, shifted by 4 columns each, each mixed 4 : 1 with columns of its own.

  (a) filter     hs_pssm_compare_dev in self mode at nm = --nm, v = 13, t = 0.5 k: ms_verify (tables + filter) and
                 ms_finalize (exact pass + ordering), survivors per hit, and the filter's rate -- 2 * 16 * 16 * 64
                 operations per issued depth step of every 16 x 16 tile of the workgroups that run -- as a share of the
                 dense int8 MFMA peak (5000 TOP/s)
  (b) no filter  the same call with pssm_cmp_filter = 0 at nm = --nm-off: what the filter buys (reported, not gated)
  (c) host       hs_pssm_compare_host on one CPU thread at --host-nm profiles; it is linear in the pairs
  unchanged      with --parent-lib: hs_pssm_scan at nm = 4096 over --n synthetic 25-mers and one bench step
                 (hs_query_dev at the bench shape), parent against this build; this build's median is to lie inside
                 the parent's own spread

Usage (GPU box): python tools/pssm_compare_sweep.py --out profiles/pssm_compare_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--nm", type=str, default="1000,10000,100000")
ap.add_argument("--nm-off", type=str, default="1000,10000")
ap.add_argument("--host-nm", type=int, default=1000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--v", type=int, default=13)
ap.add_argument("--n", type=int, default=2_000_000)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--scan-nm", type=int, default=4096)
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
ap.add_argument("--worker", type=str, default=None, help="(internal) compare | unchanged")
args = ap.parse_args()
NM = [int(x) for x in args.nm.split(",")]
NM_OFF = [int(x) for x in args.nm_off.split(",")]
A = 20
I8_PEAK_TOPS = 5000.0


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def profiles(nm, k, seed=7):
    import numpy as np
    from hsearch_amd import capi
    rng = np.random.default_rng(seed)
    P = rng.standard_gamma(0.3, size=(nm, k, A))
    fams = nm // 30                                    # 6 members each: a fifth of the profiles
    for f in range(fams):
        master = rng.standard_gamma(0.3, size=(k + 20, A))
        for j in range(6):                             # a member: its window of the master, a fifth of it its own
            P[6 * f + j] = 0.8 * master[4 * j:4 * j + k] + 0.2 * P[6 * f + j]
    P /= P.sum(axis=2, keepdims=True)
    P = P[rng.permutation(nm)]
    return capi.pssm_compare_columns(P, "pearson")


def tiles_run(nm, batch=4096):
    """16 x 16 tiles of the workgroups a self comparison runs (those with a pair x < y)"""
    total = 0
    for m0 in range(0, nm, batch):
        mb = min(batch, nm - m0)
        for x0 in range(0, mb, 32):
            first = max(0, (m0 + x0 - 31 + 31) // 32)   # tiles with y0 + 31 > x
            total += max(0, (nm + 31) // 32 - first)
    return 4 * total


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, HsError, capi, synth
    res = {"mode": mode, "gpu": torch.cuda.get_device_name(0)}
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

    k = args.k
    if mode == "compare":
        a, b = synth.make_planes(k, 2, 1, 200.0)
        eng = Engine(k, 2, 1, 200.0, a, b)             # no index
        t_val = 0.5 * k
        for filt, sizes in ((1, NM), (0, NM_OFF)):
            eng.set_option("pssm_cmp_filter", filt)
            for nm in sizes:
                P = profiles(nm, k)
                d_X = torch.from_numpy(P).to(dev)
                d_t = torch.full((nm,), t_val, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                try:     # capacity 0 asks for the count
                    cap = eng.pssm_compare_dev(d_X.data_ptr(), nm, 0, 0, d_t.data_ptr(), args.v, 0, 0, 0, 0, 0) + 1
                except HsError as e:
                    cap = int(e.n_hits) + 1
                d_x, d_y, d_d = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
                d_s = torch.empty(cap, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()

                def call():
                    state["hits"] = eng.pssm_compare_dev(d_X.data_ptr(), nm, 0, 0, d_t.data_ptr(), args.v, d_x.data_ptr(),
                                                         d_y.data_ptr(), d_d.data_ptr(), d_s.data_ptr(), cap)
                row = timed(call, reps=args.reps if nm * (2 - filt) <= 100000 else 3)
                pr = eng.profile()
                row.update(nm=nm, hits=state["hits"], pairs=pr["pssm_cmp_pairs"], survivors=pr["pssm_cmp_survivors"],
                           steps=pr["pssm_cmp_steps"], verify_ms=pr["ms_verify"], finalize_ms=pr["ms_finalize"],
                           device_ms=pr["ms_total"], survivors_per_hit=pr["pssm_cmp_survivors"] / max(1, state["hits"]))
                if filt:
                    ops = tiles_run(nm) * pr["pssm_cmp_steps"] * 2 * 16 * 16 * 64
                    tops = ops / (pr["ms_verify"] * 1e-3) / 1e12
                    row.update(filter_issued_TOPs=tops, share_of_i8_peak=tops / I8_PEAK_TOPS)
                res["%s_%d" % ("a" if filt else "b", nm)] = row
        eng.close()
        P = profiles(args.host_nm, k)
        row = timed(lambda: state.update(host=capi.pssm_compare_host(P, t_val, None, args.v)), reps=1, warmup=0)
        pairs = args.host_nm * (args.host_nm - 1) // 2
        row.update(nm=args.host_nm, pairs=pairs, hits=len(state["host"]["x"]), us_per_pair=row["median_ms"] * 1e3 / pairs)
        res["c_host"] = row
    else:
        codes = synth.make_db(args.n, k)
        a, b = synth.make_planes(k, 2, 1, args.bench_W)
        eng = Engine(k, 2, 1, args.bench_W, a, b)
        eng.index_build(codes)
        nm = args.scan_nm
        centers, _ = synth.make_queries(codes, nm, jitter=0.05)
        coords = synth.coords()
        S = np.ascontiguousarray(-((coords[None, None, :, :] - centers.reshape(nm, k, 1, 8)) ** 2).sum(axis=3))
        t = np.full(nm, -args.R * args.R)
        cap = len(eng.pssm_scan(S, t, want_counts=False)["m"]) + 1
        res["scan_%d" % nm] = timed(lambda: eng.pssm_scan(S, t, cap=cap, want_counts=False))
        eng.close()
        a, b = synth.make_planes(k, args.bench_K, args.bench_L, args.bench_W)
        q, _ = synth.make_queries(codes, args.bench_nq, jitter=0.05)
        eng = Engine(k, args.bench_K, args.bench_L, args.bench_W, a, b)
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
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--nm", args.nm, "--nm-off", args.nm_off]
    for name in ("host_nm", "k", "v", "n", "R", "scan_nm", "bench_nq", "bench_K", "bench_L", "bench_W", "warmup", "reps"):
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
    order.append(("compare", "here"))
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


for name in ["a_%d" % nm for nm in NM] + ["b_%d" % nm for nm in NM_OFF] + ["c_host"]:
    r = pooled("compare", "here", name)
    if r:
        s[name] = r
for nm in NM:
    a, bb, c = s.get("a_%d" % nm), s.get("b_%d" % nm), s.get("c_host")
    if a and bb:
        s["no_filter_over_filter_%d" % nm] = bb["median_ms"] / a["median_ms"]
    if a and c:
        s["host_over_filter_%d" % nm] = c["us_per_pair"] * 1e-3 * a["pairs"] / a["median_ms"]
for what in ("scan_%d" % args.scan_nm, "search_step"):
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
