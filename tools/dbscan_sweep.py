"""What the device-side density clusters (hs_dbscan_dev, hs_degrees_dev) cost against what they replace and against
single linkage, at the C4 shape of DESIGN.md section 12 (10^6 25-mers, K = 16, L = 8, W = 200, R = 40) on two databases
of that size -- uniform random k-mers, and planted families of 50 (tools/components_sweep.py's) -- every figure a
median of warm repetitions with its spread, every worker a fresh process:
  (a) join     the host-pointer hs_self_join, and hs_self_join followed by hs_dbscan_edges on the host: what a user
               had to do before
  (b) dbscan   hs_dbscan_dev and hs_degrees_dev (outputs stay on the device), the host-pointer hs_dbscan, and
               hs_components_dev in the same process: two self-joins against one
  (c) parent   with --parent-lib, hs_self_join and hs_components_dev in that build of the library (another commit's) and
               in this one, the builds taking turns: the existing calls must not have changed.  The criterion is the
               one section 12 used -- the difference of the medians lies inside the spread of repeated turns -- and
               both values are written down
with the bytes each path moves across PCIe per call.
Usage (GPU box): python tools/dbscan_sweep.py --out profiles/dbscan_sweep.json [--parent-lib other/libhsearch_amd.so]"""
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
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--turns", type=int, default=2, help="with --parent-lib: processes per build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) join | dbscan | existing")
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


def worker(mode):
    import zlib
    import numpy as np
    import torch
    from hsearch_amd import Engine, capi, synth
    dev = torch.device("cuda", 0)
    codes = make_codes(np)
    n = len(codes)
    a, b = synth.make_planes(args.k, args.K, args.L, args.W)
    eng = Engine(args.k, args.K, args.L, args.W, a, b)
    eng.index_build(codes)
    torch.cuda.synchronize()
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
        row.update(ms_device=eng.profile()["ms_total"])
        return row

    state = {}
    if mode in ("join", "existing"):
        cap = len(eng.self_join(args.R, sqrt_test=True, cap=4 * n)["i"])   # the two-call pattern, once

        def join():
            state["e"] = eng.self_join(args.R, sqrt_test=True, cap=max(cap, 1))
        res["join"] = timed(join)
        res["n_edges"] = cap
        res["pcie_bytes_self_join"] = 20 * cap
        # what the edges are, not only how many: the builds must agree on it
        res["edges_crc"] = zlib.crc32(state["e"]["j"].tobytes(), zlib.crc32(state["e"]["i"].tobytes()))
    if mode == "join":
        def join_then_host_dbscan():
            join()
            state["host"] = capi.dbscan_edges(state["e"]["i"], state["e"]["j"], n, args.min_pts)
        res["join_then_dbscan_edges"] = timed(join_then_host_dbscan)
        res["counts"] = {f: v for f, v in state["host"].items() if f != "label"}
        res["label_crc"] = zlib.crc32(state["host"]["label"].tobytes())
    if mode in ("dbscan", "existing"):
        d_label = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def components_dev():
            state["cc"] = eng.components_dev(d_label.data_ptr(), args.R, True)
        res["components_dev"] = timed(components_dev)
        res["n_components"], res["n_edges"] = state["cc"]
        res["components_crc"] = zlib.crc32(d_label.cpu().numpy().tobytes())
    if mode == "dbscan":
        d_degree = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def dbscan_dev():
            state["dev"] = eng.dbscan_dev(d_label.data_ptr(), args.R, args.min_pts, True, d_degree.data_ptr())

        def degrees_dev():
            state["ne"] = eng.degrees_dev(d_degree.data_ptr(), args.R, True)

        def dbscan_host():
            state["host"] = eng.dbscan(args.R, args.min_pts, True, want_degree=True)
        res["dbscan_dev"] = timed(dbscan_dev)
        res["degrees_dev"] = timed(degrees_dev)
        res["dbscan_host"] = timed(dbscan_host)
        dbscan_dev()
        assert np.array_equal(d_label.cpu().numpy().view(np.uint32), state["host"]["label"])
        assert np.array_equal(d_degree.cpu().numpy().view(np.uint32), state["host"]["degree"])
        res["counts"] = state["dev"]
        res["label_crc"] = zlib.crc32(state["host"]["label"].tobytes())
        res["degree_max"] = int(state["host"]["degree"].max()) if n else 0
        res["pcie_bytes_dbscan_dev"] = 40
        res["pcie_bytes_dbscan_host"] = 8 * n + 40
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(mode, db, lib):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--db", db]
    for name in ("n", "per_family", "k", "K", "L", "W", "R", "min_pts", "warmup", "reps"):
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
    order = [("join", "here"), ("dbscan", "here")]
    if args.parent_lib:
        order += [("existing", "parent"), ("existing", "here")] * args.turns
    rows = []
    for mode, which in order:
        row = run_worker(mode, db, args.parent_lib if which == "parent" else None)
        row.update(build=which)
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    res["runs"] += rows
    join, = [r for r in rows if r["mode"] == "join"]
    dbs, = [r for r in rows if r["mode"] == "dbscan"]
    assert all(r["n_edges"] == dbs["n_edges"] for r in rows), "the builds and paths disagree on the edges"
    assert join["counts"] == dbs["counts"] and join["label_crc"] == dbs["label_crc"], "device and host rule disagree"
    assert dbs["counts"]["n_edges"] == dbs["n_edges"]
    s = res["summary"][db] = {
        "n": dbs["n"], "min_pts": args.min_pts, "n_components": dbs["n_components"], "degree_max": dbs["degree_max"]}
    s.update(dbs["counts"])
    for name, row, what in (("a_self_join", join, "join"), ("a_join_then_host_dbscan_edges", join, "join_then_dbscan_edges"),
                            ("b_dbscan_dev", dbs, "dbscan_dev"), ("b_degrees_dev", dbs, "degrees_dev"),
                            ("b_dbscan_host", dbs, "dbscan_host"), ("b_components_dev", dbs, "components_dev")):
        s[name + "_ms"] = row[what]["median_ms"]
        s[name + "_spread_ms"] = [row[what]["min_ms"], row[what]["max_ms"]]
    s["b_dbscan_dev_over_components_dev"] = s["b_dbscan_dev_ms"] / s["b_components_dev_ms"]
    s["b_degrees_dev_over_components_dev"] = s["b_degrees_dev_ms"] / s["b_components_dev_ms"]
    s["b_speedup_over_join_then_host_dbscan_edges"] = s["a_join_then_host_dbscan_edges_ms"] / s["b_dbscan_dev_ms"]
    s["pcie_bytes_self_join"] = join["pcie_bytes_self_join"]
    s["pcie_bytes_dbscan_dev"] = dbs["pcie_bytes_dbscan_dev"]
    s["pcie_bytes_dbscan_host"] = dbs["pcie_bytes_dbscan_host"]
    if args.parent_lib:
        here = [r for r in rows if r["mode"] == "existing" and r["build"] == "here"]
        parent = [r for r in rows if r["build"] == "parent"]
        assert all(r["edges_crc"] == here[0]["edges_crc"] and r["components_crc"] == here[0]["components_crc"]
                   for r in here + parent), "the builds disagree on the self-join or the components"
        for what in ("join", "components_dev"):
            h, p = [r[what]["median_ms"] for r in here], [r[what]["median_ms"] for r in parent]
            s["c_%s_here_ms" % what], s["c_%s_parent_ms" % what] = med(here, what), med(parent, what)
            s["c_%s_here_spread_ms" % what], s["c_%s_parent_spread_ms" % what] = spread(here, what), spread(parent, what)
            s["c_%s_here_over_parent" % what] = med(here, what) / med(parent, what)
            # the difference of the builds' medians against how far one build's turns lie apart
            s["c_%s_difference_ms" % what] = abs(med(here, what) - med(parent, what))
            s["c_%s_turn_to_turn_ms" % what] = max(max(h) - min(h), max(p) - min(p))
            s["c_%s_inside_the_spread" % what] = s["c_%s_difference_ms" % what] <= s["c_%s_turn_to_turn_ms" % what]
res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
