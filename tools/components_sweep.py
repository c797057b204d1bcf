"""What the device-side components (hs_components / hs_components_dev) cost against the edge list they replace, at the
C4 shape (10^6 25-mers, K = 16, L = 8, W = 200, R = 40) on two databases of that size -- uniform random k-mers, and
planted families of 50 (a random centre, up to 4 substitutions per member: what tests/test_gpu_clustering.py's
_families draws) -- every figure a median of warm repetitions with its spread, every worker a fresh process:
  (a) join        the host-pointer hs_self_join -- with --parent-lib also for that build of the library (another
                  commit's), the two builds taking turns: the self-join must not have changed
  (b) components  hs_components_dev (labels stay on the device) and the host-pointer hs_components, against
                  hs_self_join followed by a union-find of the edge list on the host (scipy's connected_components
                  where scipy is installed, a numpy min-label propagation otherwise; the JSON says which)
with the bytes each path moves across PCIe per call and the HBM it holds beyond the index once its workspaces are
reserved (free memory before and after).
Usage (GPU box): python tools/components_sweep.py --out profiles/components_sweep.json [--parent-lib other/libhsearch_amd.so]"""
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
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--turns", type=int, default=2, help="with --parent-lib: processes per build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) join | components")
args = ap.parse_args()


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1],
            "q1_ms": s[len(s) // 4], "q3_ms": s[(3 * len(s)) // 4], "reps": len(s)}


def make_codes(np):
    if args.db == "uniform":
        from hsearch_amd import synth
        return synth.make_db(args.n, args.k)
    from tools.sweep_dbs import planted_families
    return planted_families(np, args.n, args.k, args.per_family)


def host_labels(np, n, ei, ej):
    """(labels = the smallest id per component, the name of the method)"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        g = coo_matrix((np.ones(len(ei), dtype=np.uint8), (ei, ej)), shape=(n, n))
        _, comp = connected_components(g, directed=False)
        smallest = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
        np.minimum.at(smallest, comp, np.arange(n))
        return smallest[comp].astype(np.uint32), "scipy.sparse.csgraph.connected_components"
    except ImportError:
        label = np.arange(n, dtype=np.int64)
        ei, ej = ei.astype(np.int64), ej.astype(np.int64)
        while True:
            low = np.minimum(label[ei], label[ej])
            nxt = label.copy()
            np.minimum.at(nxt, ei, low)
            np.minimum.at(nxt, ej, low)
            nxt = nxt[nxt]
            if np.array_equal(nxt, label):
                return label.astype(np.uint32), "numpy min-label propagation"
            label = nxt


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

    def timed(call):
        for _ in range(args.warmup):
            call()
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        row = summary(ms)
        p = eng.profile()
        row.update(ms_device=p["ms_total"], ms_finalize=p["ms_finalize"], join_async_retries=p["join_async_retries"])
        return row

    if mode == "join":
        cap = len(eng.self_join(args.R, sqrt_test=True, cap=4 * n)["i"])   # the two-call pattern, once
        state = {}

        def join():
            state["e"] = eng.self_join(args.R, sqrt_test=True, cap=max(cap, 1))

        def join_then_union_find():
            join()
            state["label"], state["how"] = host_labels(np, n, state["e"]["i"], state["e"]["j"])
        res["join"] = timed(join)
        torch.cuda.synchronize()
        res["hbm_beyond_index"] = free0 - torch.cuda.mem_get_info()[0]
        if hasattr(eng._lib, "hs_components"):   # (the parent build is measured for (a) only)
            res["join_then_union_find"] = timed(join_then_union_find)
            res["union_find"] = state["how"]
            res["n_components"] = int((state["label"] == np.arange(n)).sum())
        res["n_edges"] = cap
        res["pcie_bytes"] = 20 * cap
    else:
        d_label = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        state = {}

        def on_device():
            state["dev"] = eng.components_dev(d_label.data_ptr(), args.R, True)

        def to_host():
            state["host"] = eng.components(args.R, True)
        res["components_dev"] = timed(on_device)
        torch.cuda.synchronize()
        res["hbm_beyond_index"] = free0 - torch.cuda.mem_get_info()[0]   # the caller's n labels included
        res["components_host"] = timed(to_host)
        assert np.array_equal(d_label.cpu().numpy().view(np.uint32), state["host"]["label"])
        res["n_components"], res["n_edges"] = state["dev"]
        res["pcie_bytes_dev"] = 16
        res["pcie_bytes_host"] = 4 * n + 16
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(mode, db, lib):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--db", db]
    for name in ("n", "per_family", "k", "K", "L", "W", "R", "warmup", "reps"):
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
    order = [("join", "parent"), ("join", "here")] * args.turns if args.parent_lib else [("join", "here")]
    order += [("components", "here")] * (args.turns if args.parent_lib else 1)
    rows = []
    for mode, which in order:
        row = run_worker(mode, db, args.parent_lib if which == "parent" else None)
        row.update(build=which)
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    res["runs"] += rows
    here = [r for r in rows if r["build"] == "here" and r["mode"] == "join"]
    parent = [r for r in rows if r["build"] == "parent"]
    cc = [r for r in rows if r["mode"] == "components"]
    assert all(r["n_edges"] == cc[0]["n_edges"] for r in rows), "the builds and paths disagree on the edges"
    assert all(r["n_components"] == cc[0]["n_components"] for r in here + cc)
    s = res["summary"][db] = {
        "n": cc[0]["n"], "n_edges": cc[0]["n_edges"], "n_components": cc[0]["n_components"],
        "a_self_join_here_ms": med(here, "join"), "a_self_join_here_spread_ms": spread(here, "join")}
    if parent:
        s["a_self_join_parent_ms"] = med(parent, "join")
        s["a_self_join_parent_spread_ms"] = spread(parent, "join")
        s["a_here_over_parent"] = s["a_self_join_here_ms"] / s["a_self_join_parent_ms"]
    s["b_join_then_host_union_find_ms"] = med(here, "join_then_union_find")
    s["b_join_then_host_union_find_spread_ms"] = spread(here, "join_then_union_find")
    s["b_host_union_find"] = here[0]["union_find"]
    s["b_components_dev_ms"] = med(cc, "components_dev")
    s["b_components_dev_spread_ms"] = spread(cc, "components_dev")
    s["b_components_host_ms"] = med(cc, "components_host")
    s["b_components_host_spread_ms"] = spread(cc, "components_host")
    s["b_components_dev_over_self_join"] = s["b_components_dev_ms"] / s["a_self_join_here_ms"]
    s["b_speedup_over_join_then_union_find"] = s["b_join_then_host_union_find_ms"] / s["b_components_dev_ms"]
    s["pcie_bytes_self_join"] = here[0]["pcie_bytes"]
    s["pcie_bytes_components_dev"] = cc[0]["pcie_bytes_dev"]
    s["pcie_bytes_components_host"] = cc[0]["pcie_bytes_host"]
    s["hbm_beyond_index_self_join"] = max(r["hbm_beyond_index"] for r in here)
    s["hbm_beyond_index_components_dev"] = max(r["hbm_beyond_index"] for r in cc)
res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
