"""What the device-side annotation (hs_annotate / hs_annotate_dev) costs against the hit list it replaces, at the
bench's default shape (10^7 25-mers, K = 16, L = 8, W = 212, R = 40, 10^5 queries given as codes) and at the
hit-heavy shape (k = 15, same sizes), every figure a median of warm repetitions with its spread, every worker a
fresh process:
  (a) scalar     hs_query_codes_dev -- with --parent-lib also for that build of the library (another commit's), the
                 two builds taking turns: the scalar path must not have changed
  (b) device     hs_annotate_dev against hs_query_codes_dev of the same build
  (c) end to end the host-pointer hs_annotate against hs_query_codes followed by the host reduction of the hit
                 list (hs_merge_best: the std::sort + first-of-run pass SearchProteinsSharded ran before), PCIe and
                 sort included
and the HBM each path holds beyond the index once its workspaces are reserved (free memory before and after).
Usage (GPU box): python tools/annotate_sweep.py --out profiles/annotate_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--queries", type=int, default=100_000)
ap.add_argument("--ks", type=str, default="25,15")
ap.add_argument("--k", type=int, default=25, help="(worker) the k-mer length measured")
ap.add_argument("--K", type=int, default=16)
ap.add_argument("--L", type=int, default=8)
ap.add_argument("--W", type=float, default=212.0)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--e2e-reps", type=int, default=15, help="repetitions of the host-pointer paths of (c)")
ap.add_argument("--turns", type=int, default=2, help="with --parent-lib: processes per build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) scalar | annotate")
args = ap.parse_args()


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1],
            "q1_ms": s[len(s) // 4], "q3_ms": s[(3 * len(s)) // 4], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, capi, synth
    dev = torch.device("cuda", 0)
    codes = synth.make_db(args.n, args.k)
    qcodes, _ = synth.make_query_codes(codes, args.queries)
    a, b = synth.make_planes(args.k, args.K, args.L, args.W)
    eng = Engine(args.k, args.K, args.L, args.W, a, b)
    eng.index_build(codes)
    nq = args.queries
    d_q = torch.from_numpy(qcodes).to(dev)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]   # the index stands, no query workspace yet
    res = {"mode": mode, "gpu": torch.cuda.get_device_name(0)}

    def timed(call, reps, warmup=None):
        for _ in range(args.warmup if warmup is None else warmup):
            n_rows = call()
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        row = summary(ms)
        p = eng.profile()
        row.update(rows=int(n_rows), hits=int(p["hits"]), ms_total_device=p["ms_total"], ms_finalize=p["ms_finalize"],
                   ms_verify=p["ms_verify"], join_async_retries=p["join_async_retries"])
        return row

    if mode == "scalar":
        try:   # the two-call pattern: the size of the hit list
            eng.query_dev(d_q.data_ptr(), nq, args.R, 0, 0, 0, 0, 0, codes=True)
            cap = 1
        except capi.HsError as e:
            cap = e.needed
        out = [torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3)] + \
              [torch.empty(cap, dtype=torch.float64, device=dev)]
        ptrs = [t.data_ptr() for t in out]
        torch.cuda.synchronize()
        res["dev"] = timed(lambda: eng.query_dev(d_q.data_ptr(), nq, args.R, *ptrs, cap, codes=True), args.reps)
        torch.cuda.synchronize()
        res["hbm_beyond_index_dev"] = free0 - torch.cuda.mem_get_info()[0]   # the caller's hit arrays included
        if hasattr(eng._lib, "hs_merge_best") and args.e2e_reps:
            hq, hid, ht = (np.empty(cap, dtype=np.uint32) for _ in range(3))
            hd = np.empty(cap, dtype=np.float64)

            def list_then_reduce():
                n = eng.query_into(qcodes, args.R, hq, hid, ht, hd, codes=True)
                return len(capi.merge_best(hid[:n], hq[:n], ht[:n], hd[:n])["id"])
            res["e2e"] = timed(list_then_reduce, args.e2e_reps, 1)
            res["e2e_list_only"] = timed(lambda: eng.query_into(qcodes, args.R, hq, hid, ht, hd, codes=True), args.e2e_reps, 1)
            torch.cuda.synchronize()
            res["hbm_beyond_index_e2e"] = free0 - torch.cuda.mem_get_info()[0]
    else:
        cap = args.n
        out = [torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3)] + \
              [torch.empty(cap, dtype=torch.float64, device=dev)]
        ptrs = [t.data_ptr() for t in out]
        torch.cuda.synchronize()
        res["dev"] = timed(lambda: eng.annotate_dev(d_q.data_ptr(), nq, args.R, None, *ptrs, cap, codes=True), args.reps)
        torch.cuda.synchronize()
        res["hbm_beyond_index_dev"] = free0 - torch.cuda.mem_get_info()[0]   # the caller's n-row arrays included
        if args.e2e_reps:
            res["e2e"] = timed(lambda: len(eng.annotate(qcodes, args.R, codes=True, cap=cap)["id"]), args.e2e_reps, 1)
            torch.cuda.synchronize()
            res["hbm_beyond_index_e2e"] = free0 - torch.cuda.mem_get_info()[0]
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(mode, k, lib):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--k", str(k)]
    for name in ("n", "queries", "K", "L", "W", "R", "warmup", "reps", "e2e_reps"):
        argv += ["--" + name.replace("_", "-"), repr(getattr(args, name))]
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:   # a failed measurement ends the sweep: nothing else is started
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("worker failed with status %d" % r.returncode)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


if args.worker:
    worker(args.worker)
    sys.exit(0)
res = {"shape": {k: v for k, v in vars(args).items() if k not in ("worker", "out", "k")},
       "taken": time.strftime("%Y-%m-%d"), "runs": [], "summary": {}}
med = lambda rows, what: statistics.median(r[what]["median_ms"] for r in rows)
spread = lambda rows, what: [min(r[what]["min_ms"] for r in rows), max(r[what]["max_ms"] for r in rows)]
for k in [int(x) for x in args.ks.split(",")]:
    order = [("scalar", "parent"), ("scalar", "here")] * args.turns if args.parent_lib else [("scalar", "here")]
    order += [("annotate", "here")] * (args.turns if args.parent_lib else 1)
    rows = []
    for mode, which in order:
        row = run_worker(mode, k, args.parent_lib if which == "parent" else None)
        row.update(build=which, k=k)
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    res["runs"] += rows
    here = [r for r in rows if r["build"] == "here" and r["mode"] == "scalar"]
    parent = [r for r in rows if r["build"] == "parent"]
    ann = [r for r in rows if r["mode"] == "annotate"]
    s = res["summary"]["k%d" % k] = {
        "hits": here[0]["dev"]["hits"], "rows": ann[0]["dev"]["rows"],
        "a_scalar_here_ms": med(here, "dev"), "a_scalar_here_spread_ms": spread(here, "dev")}
    if parent:
        s["a_scalar_parent_ms"] = med(parent, "dev")
        s["a_scalar_parent_spread_ms"] = spread(parent, "dev")
        s["a_here_over_parent"] = s["a_scalar_here_ms"] / s["a_scalar_parent_ms"]
    s["b_annotate_dev_ms"] = med(ann, "dev")
    s["b_annotate_dev_spread_ms"] = spread(ann, "dev")
    s["b_annotate_over_scalar"] = s["b_annotate_dev_ms"] / s["a_scalar_here_ms"]
    s["hbm_beyond_index_scalar_dev"] = max(r["hbm_beyond_index_dev"] for r in here)
    s["hbm_beyond_index_annotate_dev"] = max(r["hbm_beyond_index_dev"] for r in ann)
    if "e2e" in here[0] and "e2e" in ann[0]:
        s["c_list_then_host_reduce_ms"] = med(here, "e2e")
        s["c_list_then_host_reduce_spread_ms"] = spread(here, "e2e")
        s["c_list_only_ms"] = med(here, "e2e_list_only")
        s["c_annotate_host_ms"] = med(ann, "e2e")
        s["c_annotate_host_spread_ms"] = spread(ann, "e2e")
        s["c_speedup"] = s["c_list_then_host_reduce_ms"] / s["c_annotate_host_ms"]
        s["hbm_beyond_index_scalar_e2e"] = max(r["hbm_beyond_index_e2e"] for r in here)
        s["hbm_beyond_index_annotate_e2e"] = max(r["hbm_beyond_index_e2e"] for r in ann)
res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
