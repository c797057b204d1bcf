"""What the density tree (hs_density_tree_dev) costs on its two paths, and the core distances alone, against the ladder of
hs_dbscan_dev calls it replaces, at the C4 shape (10^6 25-mers, K = 16, L = 8, W = 200, R = 40, min_pts = 5) on two
databases of that size -- uniform random k-mers, and planted families of 50 (tools/sweep_dbs.py) -- every figure a
median of warm repetitions with [min, max], every worker a fresh process:
  (a) density     hs_density_tree_dev with the pairs kept in HBM (the default) and re-joined per pass
                  (msf_edge_budget = 0), with rounds and self_joins; hs_core_distance_dev; and, in the same process,
                  a ladder of --ladder hs_dbscan_dev calls at radii R / ladder, 2 R / ladder, ..., R
  (b) unchanged   with --parent-lib: hs_msf_dev and hs_self_join for that build of the library (another commit's) and
                  this one, the two builds taking turns: neither may have changed -- this build's medians must lie
                  inside the spread of the other's repeated turns
with the HBM held beyond the index once the workspaces are reserved (free memory before and after).
Usage (GPU box): python tools/density_sweep.py --out profiles/density_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--dbs", type=str, default="uniform,families")
ap.add_argument("--db", type=str, default="uniform", help="(worker) the database measured")
ap.add_argument("--per-family", type=int, default=50)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--K", type=int, default=16)
ap.add_argument("--L", type=int, default=8)
ap.add_argument("--W", type=float, default=200.0)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--min-pts", type=int, default=5)
ap.add_argument("--ladder", type=int, default=8, help="hs_dbscan_dev calls of the ladder the tree replaces")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--turns", type=int, default=2, help="with --parent-lib: processes per build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) density | unchanged")
args = ap.parse_args()


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def make_codes(np):
    if args.db == "uniform":
        from hsearch_amd import synth
        return synth.make_db(args.n, args.k)
    from tools.sweep_dbs import planted_families
    return planted_families(np, args.n, args.k, args.per_family)


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, synth
    dev = torch.device("cuda", 0)
    codes = make_codes(np)
    n = len(codes)
    a, b = synth.make_planes(args.k, args.K, args.L, args.W)
    eng = Engine(args.k, args.K, args.L, args.W, a, b)
    eng.index_build(codes)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]   # the index stands, no query workspace yet
    res = {"mode": mode, "db": args.db, "n": n, "gpu": torch.cuda.get_device_name(0)}

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

    d_label = torch.empty(n, dtype=torch.int32, device=dev)
    d_lo = torch.empty(n, dtype=torch.int32, device=dev)
    d_hi = torch.empty(n, dtype=torch.int32, device=dev)
    d_w = torch.empty(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    state = {}

    if mode == "density":
        d_core = torch.empty(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def tree():
            state["info"] = eng.density_tree_dev(d_lo.data_ptr(), d_hi.data_ptr(), d_w.data_ptr(), n, args.R,
                                                 args.min_pts, True, d_label_ptr=d_label.data_ptr(),
                                                 d_core_ptr=d_core.data_ptr())

        def core():
            state["core"] = eng.core_distance_dev(d_core.data_ptr(), args.R, args.min_pts, True)

        def ladder():
            state["ladder"] = [eng.dbscan_dev(d_label.data_ptr(), args.R * (s + 1) / args.ladder, args.min_pts, True)
                               for s in range(args.ladder)]

        res["dbscan_ladder"] = timed(ladder)
        res["core_distance"] = timed(core)
        for name, budget in (("resident", -1), ("rejoin", 0)):
            eng.set_option("msf_edge_budget", budget)
            res["tree_" + name] = timed(tree)
            res["tree_" + name].update(state["info"])
            assert state["info"]["resident"] == (1 if budget else 0), state["info"]
            torch.cuda.synchronize()
            res["hbm_beyond_index_" + name] = free0 - torch.cuda.mem_get_info()[0]   # the caller's arrays included
            state[name] = tuple(t.cpu().numpy() for t in (d_lo, d_hi, d_w, d_label, d_core))
        assert all(np.array_equal(x, y) for x, y in zip(state["resident"], state["rejoin"]))
        top = state["ladder"][-1]                                 # the ladder's last step is hs_dbscan at R itself
        res["n_edges"], res["n_core"], res["n_clusters"] = top["n_edges"], top["n_core"], top["n_clusters"]
        assert state["info"]["n_graph_edges"] == res["n_edges"] and state["info"]["n_core"] == res["n_core"]
        assert state["info"]["n_clusters"] == res["n_clusters"] and state["core"] == (res["n_core"], res["n_edges"])
    else:
        cap = len(eng.self_join(args.R, sqrt_test=True, cap=4 * n)["i"])   # the two-call pattern, once

        def join():
            state["e"] = eng.self_join(args.R, sqrt_test=True, cap=max(cap, 1))

        def msf():
            state["msf"] = eng.msf_dev(d_lo.data_ptr(), d_hi.data_ptr(), d_w.data_ptr(), n, args.R, True,
                                       d_label_ptr=d_label.data_ptr())
        res["join"] = timed(join)
        res["msf_dev"] = timed(msf)
        res["n_edges"] = cap
        assert state["msf"]["n_graph_edges"] == cap
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(mode, db, lib):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--db", db]
    for name in ("n", "per_family", "k", "K", "L", "W", "R", "min_pts", "ladder", "warmup", "reps"):
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
res = {"shape": {k: v for k, v in vars(args).items() if k not in ("worker", "out", "db")},
       "taken": time.strftime("%Y-%m-%d"), "runs": [], "summary": {}}
med = lambda rows, what: statistics.median(r[what]["median_ms"] for r in rows)
spread = lambda rows, what: [min(r[what]["min_ms"] for r in rows), max(r[what]["max_ms"] for r in rows)]
for db in args.dbs.split(","):
    order = [("density", "here")]
    if args.parent_lib:
        order += [("unchanged", "parent"), ("unchanged", "here")] * args.turns
    rows = []
    for mode, which in order:
        row = run_worker(mode, db, args.parent_lib if which == "parent" else None)
        row.update(build=which)
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    res["runs"] += rows
    assert all(r["n_edges"] == rows[0]["n_edges"] for r in rows), "the builds and paths disagree on the graph"
    m = rows[0]
    s = res["summary"][db] = {"n": m["n"], "min_pts": args.min_pts, "n_edges": m["n_edges"], "n_core": m["n_core"],
                              "n_clusters": m["n_clusters"], "n_tree_edges": m["tree_resident"]["n_tree_edges"],
                              "rounds": m["tree_resident"]["rounds"],
                              "self_joins_resident": m["tree_resident"]["self_joins"],
                              "self_joins_rejoin": m["tree_rejoin"]["self_joins"]}
    for what in ("dbscan_ladder", "core_distance", "tree_resident", "tree_rejoin"):
        s[what + "_ms"] = m[what]["median_ms"]
        s[what + "_spread_ms"] = [m[what]["min_ms"], m[what]["max_ms"]]
    s["ladder_over_tree_resident"] = s["dbscan_ladder_ms"] / s["tree_resident_ms"]
    s["ladder_over_tree_rejoin"] = s["dbscan_ladder_ms"] / s["tree_rejoin_ms"]
    s["hbm_beyond_index_resident"] = m["hbm_beyond_index_resident"]
    s["hbm_beyond_index_rejoin"] = m["hbm_beyond_index_rejoin"]
    for which in ("here", "parent"):
        un = [r for r in rows if r["mode"] == "unchanged" and r["build"] == which]
        for what in ("join", "msf_dev"):
            if un:
                s["unchanged_%s_%s_ms" % (what, which)] = med(un, what)
                s["unchanged_%s_%s_spread_ms" % (what, which)] = spread(un, what)
    if args.parent_lib:   # the acceptance: this build inside the spread of the other's turns
        for what in ("join", "msf_dev"):
            lo, hi = s["unchanged_%s_parent_spread_ms" % what]
            s["unchanged_%s_inside_parent_spread" % what] = lo <= s["unchanged_%s_here_ms" % what] <= hi
res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
