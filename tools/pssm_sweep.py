"""hs_pssm_scan against hs_bruteforce on one MI355X, and the unchanged paths against the parent commit's library.

Shape: 10^7 synthetic 25-mers (hsearch_amd/synth.py); the profiles are the Euclidean equivalents of search centres at
R = 40 -- S[p][a] = -sum_j (coords[a][j] - c[8 p + j])^2, t = -R^2 --, so the scan and the brute-force search do the
same pairs and find the same hits.  nm = 16, 256, 4096.  Medians of --reps warm repetitions with [min, max], every
worker a fresh process, the two builds taking turns:
  (a) scan       hs_pssm_scan on this build, the MFMA filter on (host pointers: PCIe is in it)
  (b) nofilter   the same with HS_OPT_PSSM_FILTER = 0, at the smallest nm only
  (c) brute      with --parent-lib: hs_bruteforce over the same centres by THAT library (host pointers too)
  unchanged      with --parent-lib: one bench step (hs_query_dev at the bench shape) and hs_bruteforce at the smallest
                 nm, parent against this build; this build's median is to lie inside the parent's own spread
Per nm: hits, survivors / hits, ms, pairs/s, and the fraction of the FP6 MFMA peak by ISSUED depth,
pairs x steps x 128 x 2 / time / 10 PF.

Usage (GPU box): python tools/pssm_sweep.py --out profiles/pssm_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--nm", type=str, default="16,256,4096")
ap.add_argument("--bench-nq", type=int, default=100_000)
ap.add_argument("--bench-K", type=int, default=16)
ap.add_argument("--bench-L", type=int, default=8)
ap.add_argument("--bench-W", type=float, default=212.0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--turns", type=int, default=2, help="processes per arm and build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) scan | brute | unchanged")
args = ap.parse_args()
NM = [int(x) for x in args.nm.split(",")]
PEAK_FP6 = 10e15   # dense FP6 MFMA peak of the chip, flop/s


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, synth
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
    res["n"] = args.n

    def scan_engine():   # the tables play no part in a scan or in brute force: one small table
        a, b = synth.make_planes(args.k, 2, 1, args.bench_W)
        eng = Engine(args.k, 2, 1, args.bench_W, a, b)
        eng.index_build(codes)
        return eng

    if mode == "scan":
        coords = synth.coords()
        eng = scan_engine()
        steps = -(-args.k * 20 // 128)
        for nm in NM:
            c = centers[:nm].reshape(nm, args.k, 1, 8)
            S = np.ascontiguousarray(-((coords[None, None, :, :] - c) ** 2).sum(axis=3))
            t = np.full(nm, -args.R * args.R)
            cap = len(eng.pssm_scan(S, t, want_counts=False)["m"]) + 1

            def scan():
                state["r"] = eng.pssm_scan(S, t, cap=cap, want_counts=False)
            row = timed(scan)
            p = eng.profile()
            pairs = nm * args.n
            row.update(hits=len(state["r"]["m"]), survivors=p["pssm_survivors"], pairs=pairs,
                       pairs_per_s=pairs / (row["median_ms"] * 1e-3),
                       device_ms=p["ms_total"], filter_ms=p["ms_verify"], exact_ms=p["ms_finalize"],
                       peak_fraction_issued=pairs * steps * 128 * 2 / (row["median_ms"] * 1e-3) / PEAK_FP6,
                       peak_fraction_issued_filter_kernel=pairs * steps * 128 * 2 / (p["ms_verify"] * 1e-3) / PEAK_FP6)
            row["survivors_per_hit"] = row["survivors"] / max(1, row["hits"])
            res["scan_%d" % nm] = row
            if nm == NM[0]:
                eng.set_option("pssm_filter", 0)
                res["nofilter_%d" % nm] = timed(scan, reps=3, warmup=1)
                res["nofilter_%d" % nm]["hits"] = len(state["r"]["m"])
                eng.set_option("pssm_filter", 1)
        eng.close()
    elif mode == "brute":
        eng = scan_engine()
        for nm in NM:
            cap = len(eng.bruteforce(centers[:nm], args.R)["q"]) + 1

            def brute():
                state["r"] = eng.bruteforce(centers[:nm], args.R, cap=cap)
            row = timed(brute)
            row.update(hits=len(state["r"]["q"]), pairs=nm * args.n, pairs_per_s=nm * args.n / (row["median_ms"] * 1e-3))
            res["brute_%d" % nm] = row
        eng.close()
    else:
        eng = scan_engine()
        nm = NM[0]
        cap = len(eng.bruteforce(centers[:nm], args.R)["q"]) + 1
        res["brute_%d" % nm] = timed(lambda: eng.bruteforce(centers[:nm], args.R, cap=cap))
        eng.close()
        dev = torch.device("cuda", 0)
        a, b = synth.make_planes(args.k, args.bench_K, args.bench_L, args.bench_W)
        q, _ = synth.make_queries(codes, args.bench_nq, jitter=0.05)
        eng = Engine(args.k, args.bench_K, args.bench_L, args.bench_W, a, b)
        eng.index_build(codes)
        d_c = torch.from_numpy(q).to(dev)
        cap = 64 * args.bench_nq
        d_q, d_id, d_t = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
        d_d = torch.empty(cap, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def step():
            state["hits"] = eng.query_dev(d_c.data_ptr(), args.bench_nq, args.R, d_q.data_ptr(), d_id.data_ptr(),
                                          d_t.data_ptr(), d_d.data_ptr(), cap)
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
    for name in ("n", "k", "R", "bench_nq", "bench_K", "bench_L", "bench_W", "warmup", "reps"):
        argv += ["--" + name.replace("_", "-"), repr(getattr(args, name))]
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=600)
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
    order.append(("scan", "here"))
    if args.parent_lib:
        order += [("brute", "parent"), ("unchanged", "parent"), ("unchanged", "here")]
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
    return {"median_ms": statistics.median(r["median_ms"] for r in rows), "min_ms": min(r["min_ms"] for r in rows),
            "max_ms": max(r["max_ms"] for r in rows), "turns": len(rows), "last": rows[-1]}


for nm in NM:
    a = pooled("scan", "here", "scan_%d" % nm)
    if a:
        last = a.pop("last")
        a.update({f: last[f] for f in ("hits", "survivors", "survivors_per_hit", "pairs", "filter_ms", "exact_ms",
                                       "device_ms")})
        a["pairs_per_s"] = a["pairs"] / (a["median_ms"] * 1e-3)
        a["peak_fraction_issued"] = last["peak_fraction_issued"] * last["median_ms"] / a["median_ms"]
        a["peak_fraction_issued_filter_kernel"] = last["peak_fraction_issued_filter_kernel"]
        s["a_scan_%d" % nm] = a
    c = pooled("brute", "parent", "brute_%d" % nm)
    if c:
        last = c.pop("last")
        c.update(hits=last["hits"], pairs_per_s=last["pairs"] / (c["median_ms"] * 1e-3))
        s["c_brute_parent_%d" % nm] = c
        if a:
            s["c_over_a_%d" % nm] = c["median_ms"] / a["median_ms"]
            s["same_hits_%d" % nm] = c["hits"] == a["hits"]
b = pooled("scan", "here", "nofilter_%d" % NM[0])
if b:
    last = b.pop("last")
    b["hits"] = last["hits"]
    s["b_nofilter_%d" % NM[0]] = b
for what in ("search_step", "brute_%d" % NM[0]):
    p, h = pooled("unchanged", "parent", what), pooled("unchanged", "here", what)
    if p and h:
        p.pop("last"), h.pop("last")
        s["unchanged_%s_parent" % what], s["unchanged_%s_here" % what] = p, h
        s["unchanged_%s_verdict" % what] = ("inside" if p["min_ms"] <= h["median_ms"] <= p["max_ms"] else
                                               "faster" if h["median_ms"] < p["min_ms"] else "slower")
if res["runs"]:
    res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
