"""hs_pssm_topk on one MI355X against the routes the parent commit's library offers, and the unchanged paths against
that library.  The protocol of tools/pssm_sweep.py: 10^7 synthetic 25-mers, the Euclidean-equivalent profiles of search
centres, host pointers (PCIe is in every figure), medians of --reps warm repetitions with [min, max], every worker a
fresh process, the builds taking turns.

  (a) topk       hs_pssm_topk on this build, nm x topk, with its three phases (ms_hash: sample pass, ms_verify: tables
                 + filter, ms_finalize: exact pass + selection); and the sample sizes --samples at the largest shape
  (b) oracle     with --parent-lib: hs_pssm_scan by THAT library at the ORACLE threshold -- the true topk-th best score
                 per profile, taken from (a)'s rows -- plus the selection of the rows on the host (numpy lexsort).  The
                 cheapest route a user of the parent could take, and it needs the answer in advance
  (c) nofloor    with --parent-lib: that library's hs_pssm_scan at -DBL_MAX, the smallest nm only: what a user without
                 a threshold has.  The scan and its copy to the host only: the host selection is NOT in the figure
  unchanged      with --parent-lib: hs_pssm_scan at the largest nm (t = -R^2) and one bench step (hs_query_dev at the
                 bench shape), parent against this build; this build's median is to lie inside the parent's own spread

Usage (GPU box): python tools/pssm_topk_sweep.py --out profiles/pssm_topk_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, tempfile, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--nm", type=str, default="16,256,4096")
ap.add_argument("--topk", type=str, default="10,64")
ap.add_argument("--samples", type=str, default="16384,65536,262144")
ap.add_argument("--bench-nq", type=int, default=100_000)
ap.add_argument("--bench-K", type=int, default=16)
ap.add_argument("--bench-L", type=int, default=8)
ap.add_argument("--bench-W", type=float, default=212.0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--turns", type=int, default=2, help="processes per arm and build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) topk | parent | unchanged")
ap.add_argument("--oracle-file", type=str, default=None, help="(internal) the oracle thresholds, written by topk")
args = ap.parse_args()
NM = [int(x) for x in args.nm.split(",")]
TOPK = [int(x) for x in args.topk.split(",")]
SAMPLES = [int(x) for x in args.samples.split(",")]
NO_FLOOR = -1.7976931348623157e308


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, synth
    res = {"mode": mode, "gpu": torch.cuda.get_device_name(0), "n": args.n}
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

    def profiles(nm):
        c = centers[:nm].reshape(nm, args.k, 1, 8)
        return np.ascontiguousarray(-((coords[None, None, :, :] - c) ** 2).sum(axis=3))

    def scan_engine():   # the tables play no part in a scan: one small table
        a, b = synth.make_planes(args.k, 2, 1, args.bench_W)
        eng = Engine(args.k, 2, 1, args.bench_W, a, b)
        eng.index_build(codes)
        return eng

    if mode == "topk":
        eng = scan_engine()
        oracle = {}
        for nm in NM:
            S = profiles(nm)
            for topk in TOPK:
                def call():
                    state["r"] = eng.pssm_topk(S, topk)
                row = timed(call)
                p = eng.profile()
                row.update(sample_ms=p["ms_hash"], filter_ms=p["ms_verify"], exact_select_ms=p["ms_finalize"],
                           device_ms=p["ms_total"], survivors=p["pssm_survivors"], hits=p["hits"],
                           raised=p["pssm_topk_raised"], sample=p["pssm_topk_sample"],
                           hits_per_profile=p["hits"] / nm)
                res["topk_%d_%d" % (nm, topk)] = row
                oracle["t_%d_%d" % (nm, topk)] = state["r"]["score"][:, topk - 1].copy()
                oracle["id_%d_%d" % (nm, topk)] = state["r"]["id"]
        S, topk = profiles(NM[-1]), TOPK[-1]
        for sample in SAMPLES:
            eng.set_option("pssm_topk_sample", sample)
            row = timed(lambda: eng.pssm_topk(S, topk))
            p = eng.profile()
            row.update(sample_ms=p["ms_hash"], filter_ms=p["ms_verify"], exact_select_ms=p["ms_finalize"],
                       device_ms=p["ms_total"], survivors=p["pssm_survivors"], hits=p["hits"])
            res["sample_%d" % sample] = row
        eng.close()
        if args.oracle_file:
            np.savez(args.oracle_file, **oracle)
    elif mode == "parent":
        eng = scan_engine()
        oracle = np.load(args.oracle_file)
        for nm in NM:
            S = profiles(nm)
            for topk in TOPK:
                t = oracle["t_%d_%d" % (nm, topk)]
                cap = len(eng.pssm_scan(S, t, want_counts=False)["m"]) + 1

                def call():
                    h = eng.pssm_scan(S, t, cap=cap, want_counts=False)
                    order = np.lexsort((h["id"], -h["score"], h["m"]))       # (m, score descending, id)
                    m = h["m"][order]
                    rank = np.arange(len(m)) - np.searchsorted(m, m, side="left")
                    keep = order[rank < topk]
                    rows = np.full((nm, topk), 0xffffffff, dtype=np.uint32)
                    rows[h["m"][keep], rank[rank < topk]] = h["id"][keep]
                    state["rows"], state["hits"] = rows, len(m)
                row = timed(call)
                row.update(hits=state["hits"], same_rows=bool(np.array_equal(state["rows"], oracle["id_%d_%d" % (nm, topk)])))
                res["oracle_%d_%d" % (nm, topk)] = row
        nm = NM[0]
        S, t = profiles(nm), np.full(nm, NO_FLOOR)
        cap = nm * args.n

        def nofloor():
            state["hits"] = len(eng.pssm_scan(S, t, cap=cap, want_counts=False)["m"])
        res["nofloor_%d" % nm] = timed(nofloor, reps=3, warmup=1)
        res["nofloor_%d" % nm]["hits"] = state["hits"]
        eng.close()
    else:
        eng = scan_engine()
        nm = NM[-1]
        S, t = profiles(nm), np.full(nm, -args.R * args.R)
        cap = len(eng.pssm_scan(S, t, want_counts=False)["m"]) + 1
        res["scan_%d" % nm] = timed(lambda: eng.pssm_scan(S, t, cap=cap, want_counts=False))
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


def run_worker(mode, lib, oracle_file):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--nm", args.nm, "--topk", args.topk,
            "--samples", args.samples, "--oracle-file", oracle_file]
    for name in ("n", "k", "R", "bench_nq", "bench_K", "bench_L", "bench_W", "warmup", "reps"):
        argv += ["--" + name.replace("_", "-"), repr(getattr(args, name))]
    # every GPU step under a time limit of its own; a failed measurement ends the sweep: nothing else is started
    r = subprocess.run(["timeout", "-k", "10", "420"] + argv, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("worker %s failed with status %d" % (mode, r.returncode))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


if args.worker:
    worker(args.worker)
    sys.exit(0)
shape = {k: v for k, v in vars(args).items() if k not in ("worker", "out", "oracle_file", "parent_lib")}
shape["parent_lib"] = "the parent commit's libhsearch_amd.so" if args.parent_lib else None
res = {"shape": shape, "taken": time.strftime("%Y-%m-%d"), "runs": [], "summary": {}}
order = []
for _ in range(args.turns):
    order.append(("topk", "here"))
    if args.parent_lib:
        order += [("parent", "parent"), ("unchanged", "parent"), ("unchanged", "here")]
with tempfile.TemporaryDirectory() as tmp:
    oracle_file = os.path.join(tmp, "oracle.npz")
    for mode, which in order:
        row = run_worker(mode, args.parent_lib if which == "parent" else None, oracle_file)
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


for nm in NM:
    for topk in TOPK:
        a = pooled("topk", "here", "topk_%d_%d" % (nm, topk))
        b = pooled("parent", "parent", "oracle_%d_%d" % (nm, topk))
        if a:
            s["a_topk_%d_%d" % (nm, topk)] = a
        if b:
            s["b_oracle_parent_%d_%d" % (nm, topk)] = b
        if a and b:
            s["a_over_b_%d_%d" % (nm, topk)] = a["median_ms"] / b["median_ms"]
            s["a_over_b_%d_%d_spread" % (nm, topk)] = [a["min_ms"] / b["max_ms"], a["max_ms"] / b["min_ms"]]
c = pooled("parent", "parent", "nofloor_%d" % NM[0])
if c:
    s["c_nofloor_parent_%d" % NM[0]] = c
    for topk in TOPK:
        a = s.get("a_topk_%d_%d" % (NM[0], topk))
        if a:
            s["a_over_c_%d_%d" % (NM[0], topk)] = a["median_ms"] / c["median_ms"]
            s["a_over_c_%d_%d_spread" % (NM[0], topk)] = [a["min_ms"] / c["max_ms"], a["max_ms"] / c["min_ms"]]
best = None
for sample in SAMPLES:
    r = pooled("topk", "here", "sample_%d" % sample)
    if r:
        s["sample_%d" % sample] = r
        if best is None or r["median_ms"] < best[1]:
            best = (sample, r["median_ms"])
if best:
    s["fastest_sample"] = best[0]
for what in ("scan_%d" % NM[-1], "search_step"):
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
