"""What the top-k selection (hs_self_knn_dev, hs_query_topk_dev) costs, at the C4 shape (10^6 25-mers, K = 16, L = 8,
W = 200, R = 40) on planted families of 50 (tools/sweep_dbs.py: 34 neighbours per k-mer) and, for the search, at the
bench shape (bench.py: 10^7 25-mers, W = 212, R = 40, 10^5 queries) -- every figure a median of warm repetitions with
[min, max], every worker a fresh process:
  (a) knn         hs_self_knn_dev at topk 10 and 64; hs_degrees_dev, the same self-join with the cheapest sink (the
                  difference is the selection); hs_core_distance_dev at min_pts 11, the same order statistic without ids,
                  by threshold rounds; the host route hs_self_join + selection on the host, with the bytes moved
  (b) search      hs_query_topk_dev at topk 10 against hs_query_dev, the same queries
  (c) unchanged   with --parent-lib: hs_self_join, hs_components_dev and a search step (hs_query_dev at the bench shape)
                  for that build of the library (another commit's) and this one, the two builds taking turns: none may
                  have changed -- this build's medians must lie inside the spread of the other's repeated turns; the
                  verdict is recorded as "inside" or "outside"
Usage (GPU box): python tools/knn_sweep.py --out profiles/knn_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--per-family", type=int, default=50)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--K", type=int, default=16)
ap.add_argument("--L", type=int, default=8)
ap.add_argument("--W", type=float, default=200.0)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--topk", type=str, default="10,64")
ap.add_argument("--bench-n", type=int, default=10_000_000)
ap.add_argument("--bench-nq", type=int, default=100_000)
ap.add_argument("--bench-W", type=float, default=212.0)
ap.add_argument("--bench-R", type=float, default=40.0, help="the search's radius: bench.py's own --R")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--turns", type=int, default=2, help="with --parent-lib: processes per build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--skip", type=str, default="", help="comma list of workers left out: knn, search, unchanged")
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) knn | search | unchanged")
args = ap.parse_args()
TOPK = [int(t) for t in args.topk.split(",")]


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, synth
    dev = torch.device("cuda", 0)
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

    def graph_engine():
        from tools.sweep_dbs import planted_families
        codes = planted_families(np, args.n, args.k, args.per_family)
        a, b = synth.make_planes(args.k, args.K, args.L, args.W)
        eng = Engine(args.k, args.K, args.L, args.W, a, b)
        eng.index_build(codes)
        return eng, len(codes)

    def search_engine():
        codes = synth.make_db(args.bench_n, args.k)
        a, b = synth.make_planes(args.k, args.K, args.L, args.bench_W)
        centers, _ = synth.make_queries(codes, args.bench_nq, jitter=0.05)
        eng = Engine(args.k, args.K, args.L, args.bench_W, a, b)
        eng.index_build(codes)
        return eng, torch.from_numpy(centers).to(dev)

    def search_step(eng, d_centers):
        nq = d_centers.shape[0]
        cap = 64 * nq
        d_q, d_id, d_t = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
        d_d = torch.empty(cap, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def step():
            state["hits"] = eng.query_dev(d_centers.data_ptr(), nq, args.bench_R, d_q.data_ptr(), d_id.data_ptr(),
                                          d_t.data_ptr(), d_d.data_ptr(), cap)
        return step

    if mode == "knn":
        eng, n = graph_engine()
        res["n"] = n
        d_deg = torch.empty(n, dtype=torch.int32, device=dev)
        d_core = torch.empty(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def degrees():
            state["n_edges"] = eng.degrees_dev(d_deg.data_ptr(), args.R, True)
        res["degrees_dev"] = timed(degrees)
        res["n_edges"] = state["n_edges"]
        for topk in TOPK:
            d_id, d_t = (torch.empty(n * topk, dtype=torch.int32, device=dev) for _ in range(2))
            d_d = torch.empty(n * topk, dtype=torch.float64, device=dev)
            d_c = torch.empty(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def knn():
                state["knn_edges"] = eng.self_knn_dev(d_id.data_ptr(), d_t.data_ptr(), d_d.data_ptr(), d_c.data_ptr(),
                                                      args.R, topk, True)
            res["self_knn_dev_%d" % topk] = timed(knn)
            assert state["knn_edges"] == res["n_edges"] and bool((d_c == d_deg).all())
            res["self_knn_dev_%d" % topk]["bytes_out"] = n * topk * 16 + n * 4

            def core():
                state["core"] = eng.core_distance_dev(d_core.data_ptr(), args.R, topk + 1, True)
            res["core_distance_dev_minpts_%d" % (topk + 1)] = timed(core)
            assert bool((d_d.view(torch.int64).view(n, topk)[:, topk - 1] == d_core.view(torch.int64)).all())
            del d_id, d_t, d_d, d_c
        cap = res["n_edges"]
        topk = TOPK[0]

        def host_route():
            e = eng.self_join(args.R, sqrt_test=True, cap=max(cap, 1))
            order = np.lexsort((e["j"], e["dist"].view(np.uint64), e["i"]))
            start = np.searchsorted(e["i"][order], np.arange(n))
            rank = np.arange(len(order)) - start[e["i"][order]]
            state["host_rows"] = order[rank < topk]
        res["host_route_topk_%d" % topk] = timed(host_route, reps=2, warmup=1)
        res["host_route_topk_%d" % topk]["bytes_over_pcie"] = cap * 20
        eng.close()
    elif mode == "search":
        eng, d_centers = search_engine()
        nq = d_centers.shape[0]
        res["n"], res["nq"] = args.bench_n, nq
        res["query_dev"] = timed(search_step(eng, d_centers))
        res["n_hits"] = state["hits"]
        for topk in TOPK[:1]:
            d_id, d_t = (torch.empty(nq * topk, dtype=torch.int32, device=dev) for _ in range(2))
            d_d = torch.empty(nq * topk, dtype=torch.float64, device=dev)
            d_c = torch.empty(nq, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def top():
                state["top_hits"] = eng.query_topk_dev(d_centers.data_ptr(), nq, topk, args.bench_R, None, d_id.data_ptr(),
                                                       d_t.data_ptr(), d_d.data_ptr(), d_c.data_ptr())
            res["query_topk_dev_%d" % topk] = timed(top)
            assert state["top_hits"] == res["n_hits"]
        eng.close()
    else:
        eng, n = graph_engine()
        res["n"] = n
        d_label = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        cap = len(eng.self_join(args.R, sqrt_test=True, cap=4 * n)["i"])   # the two-call pattern, once

        def join():
            state["e"] = eng.self_join(args.R, sqrt_test=True, cap=max(cap, 1))

        def components():
            state["cc"] = eng.components_dev(d_label.data_ptr(), args.R, True)
        res["join"] = timed(join, reps=5, warmup=1)
        res["components_dev"] = timed(components)
        res["n_edges"] = cap
        assert state["cc"][1] == cap
        eng.close()
        eng, d_centers = search_engine()
        res["search_step"] = timed(search_step(eng, d_centers))
        res["n_hits"] = state["hits"]
        eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(mode, lib):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--topk", args.topk]
    for name in ("n", "per_family", "k", "K", "L", "W", "R", "bench_n", "bench_nq", "bench_W", "bench_R", "warmup", "reps"):
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
res = {"shape": {k: v for k, v in vars(args).items() if k not in ("worker", "out", "skip")},
       "taken": time.strftime("%Y-%m-%d"), "runs": [], "summary": {}}
skip = set(args.skip.split(","))
order = [(m, "here") for m in ("knn", "search") if m not in skip]
if args.parent_lib and "unchanged" not in skip:
    order += [("unchanged", "parent"), ("unchanged", "here")] * args.turns
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
for row in res["runs"]:
    if row["mode"] == "unchanged":
        continue
    for what, v in row.items():
        if isinstance(v, dict):
            s[what + "_ms"] = v["median_ms"]
            s[what + "_spread_ms"] = [v["min_ms"], v["max_ms"]]
            for extra in ("bytes_out", "bytes_over_pcie"):
                if extra in v:
                    s[what + "_" + extra] = v[extra]
        elif what in ("n", "nq", "n_edges", "n_hits"):
            s[row["mode"] + "_" + what] = v
for topk in TOPK:
    if "self_knn_dev_%d_ms" % topk in s:
        s["selection_%d_ms" % topk] = s["self_knn_dev_%d_ms" % topk] - s["degrees_dev_ms"]
med = lambda rows, what: statistics.median(r[what]["median_ms"] for r in rows)
spread = lambda rows, what: [min(r[what]["min_ms"] for r in rows), max(r[what]["max_ms"] for r in rows)]
for which in ("here", "parent"):
    un = [r for r in res["runs"] if r["mode"] == "unchanged" and r["build"] == which]
    for what in ("join", "components_dev", "search_step"):
        if un:
            s["unchanged_%s_%s_ms" % (what, which)] = med(un, what)
            s["unchanged_%s_%s_spread_ms" % (what, which)] = spread(un, what)
if "unchanged_join_parent_ms" in s:   # the yardstick: the parent's own spread over its turns
    for what in ("join", "components_dev", "search_step"):
        lo, hi = s["unchanged_%s_parent_spread_ms" % what]
        s["unchanged_%s_verdict" % what] = "inside" if lo <= s["unchanged_%s_here_ms" % what] <= hi else "outside"
if res["runs"]:
    res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
