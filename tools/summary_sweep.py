"""What the device-side cluster summaries (hs_cluster_profile_dev, hs_cluster_radii_dev) cost against what they replace,
at the C4 shape of DESIGN.md sections 12 / 13 (10^6 25-mers, K = 16, L = 8, W = 200, R = 40, min_pts = 5) on two
databases of that size -- planted families of 50 (labels: hs_dbscan_dev, min_size 1) and uniform random k-mers
(labels: hs_components_dev, min_size 1: 10^6 singleton rows) -- every figure a median of warm repetitions with its
spread, every worker a fresh process:
  (a) summary  hs_cluster_profile_dev, hs_cluster_radii_dev against the centroids, and what a user did before: the
               labels copied out and hs_cluster_summary_codes on the host over the host's codes
  (b) parent   with --parent-lib, hs_self_join and hs_dbscan_dev in that build of the library (another commit's) and in
               this one, the builds taking turns, and with --bench-steps the default step of bench.py likewise: the
               existing calls must not have changed.  The criterion is section 12's -- the difference of the medians
               lies inside the spread of repeated turns -- and both values are written down
with the bytes each route moves across PCIe per call.
Usage (GPU box): python tools/summary_sweep.py --out profiles/summary_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--dbs", type=str, default="families,uniform")
ap.add_argument("--db", type=str, default="families", help="(worker) the database measured")
ap.add_argument("--per-family", type=int, default=50)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--K", type=int, default=16)
ap.add_argument("--L", type=int, default=8)
ap.add_argument("--W", type=float, default=200.0)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--min-pts", type=int, default=5)
ap.add_argument("--min-size", type=int, default=1)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--turns", type=int, default=2, help="with --parent-lib: processes per build, taking turns")
ap.add_argument("--bench-steps", type=int, default=0, help="with --parent-lib: also bench.py's default step, this many")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) summary | existing")
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

    def timed(call, reps=None):
        for _ in range(args.warmup):
            call()
        ms = []
        for _ in range(reps or args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        return summary(ms)

    d_label = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    state = {}
    if mode == "existing":
        cap = len(eng.self_join(args.R, sqrt_test=True, cap=4 * n)["i"])

        def join():
            state["e"] = eng.self_join(args.R, sqrt_test=True, cap=max(cap, 1))

        def dbscan_dev():
            state["c"] = eng.dbscan_dev(d_label.data_ptr(), args.R, args.min_pts, True)
        res["join"] = timed(join)
        res["dbscan_dev"] = timed(dbscan_dev)
        res["edges_crc"] = zlib.crc32(state["e"]["j"].tobytes(), zlib.crc32(state["e"]["i"].tobytes()))
        res["label_crc"] = zlib.crc32(d_label.cpu().numpy().tobytes())
    else:
        if args.db == "uniform":
            eng.components_dev(d_label.data_ptr(), args.R, True)
        else:
            eng.dbscan_dev(d_label.data_ptr(), args.R, args.min_pts, True)
        m = args.min_size
        cap = n // m
        ol = torch.empty(cap, dtype=torch.int32, device=dev)
        osz = torch.empty(cap, dtype=torch.int32, device=dev)
        cen = torch.empty((cap, 8 * args.k), dtype=torch.float64, device=dev)
        mx = torch.empty(cap, dtype=torch.float64, device=dev)
        rad = torch.empty(cap, dtype=torch.float64, device=dev)
        med = torch.empty(cap, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def profile_dev():
            state["rows"] = eng.cluster_profile_dev(d_label.data_ptr(), m, ol.data_ptr(), osz.data_ptr(), None,
                                                    cen.data_ptr(), cap)

        def radii_dev():
            eng.cluster_radii_dev(d_label.data_ptr(), m, cen.data_ptr(), state["rows"], mx.data_ptr(), rad.data_ptr(),
                                  med.data_ptr())
        res["profile_dev"] = timed(profile_dev)
        rows = state["rows"]
        lds_crc = zlib.crc32(cen[:rows].cpu().numpy().tobytes())
        res["radii_dev"] = timed(radii_dev)

        def host_route():
            label = d_label.cpu().numpy().view(np.uint32)
            state["host"] = capi.cluster_summary_codes(codes, label, m)
        res["labels_out_then_summary_codes"] = timed(host_route, args.host_reps)
        host = state["host"]
        assert zlib.crc32(host["centroid"].tobytes()) == lds_crc, "device and host rule disagree on the centroids"
        assert np.array_equal(host["radius"], rad[:rows].cpu().numpy()), "device and host rule disagree on the radii"
        assert np.array_equal(host["medoid"], med[:rows].cpu().numpy().view(np.uint32))
        sizes = osz[:rows].cpu().numpy()
        res.update(rows=rows, kept=int(sizes.sum()), largest_row=int(sizes.max()) if rows else 0, centroid_crc=lds_crc,
                   pcie_bytes_dev=24, pcie_bytes_host_route=4 * n,
                   hbm_bytes_centroids=int(rows) * 64 * args.k)
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(mode, db, lib):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    if mode == "bench":
        argv = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps),
                "--warmup", "2"]
    else:
        argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--db", db]
        for name in ("n", "per_family", "k", "K", "L", "W", "R", "min_pts", "min_size", "warmup", "reps", "host_reps"):
            argv += ["--" + name.replace("_", "-"), repr(getattr(args, name))]
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:   # a failed measurement ends the sweep: nothing else is started
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("worker failed with status %d" % r.returncode)
    if mode == "bench":
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        return {"mode": "bench", "db": "bench", "queries_per_s": line["value"]}
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
    order = [("summary", "here")]
    if args.parent_lib:
        order += [("existing", "parent"), ("existing", "here")] * args.turns
    rows = []
    for mode, which in order:
        row = run_worker(mode, db, args.parent_lib if which == "parent" else None)
        row.update(build=which)
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    res["runs"] += rows
    sm, = [r for r in rows if r["mode"] == "summary"]
    s = res["summary"][db] = {f: sm[f] for f in ("n", "rows", "kept", "largest_row", "pcie_bytes_dev",
                                                 "pcie_bytes_host_route", "hbm_bytes_centroids")}
    for what in ("profile_dev", "radii_dev", "labels_out_then_summary_codes"):
        s["a_%s_ms" % what] = sm[what]["median_ms"]
        s["a_%s_spread_ms" % what] = [sm[what]["min_ms"], sm[what]["max_ms"]]
    s["a_host_route_over_device"] = s["a_labels_out_then_summary_codes_ms"] / (s["a_profile_dev_ms"] + s["a_radii_dev_ms"])
    if args.parent_lib:
        here = [r for r in rows if r["mode"] == "existing" and r["build"] == "here"]
        parent = [r for r in rows if r["build"] == "parent"]
        assert all(r["edges_crc"] == here[0]["edges_crc"] and r["label_crc"] == here[0]["label_crc"]
                   for r in here + parent), "the builds disagree on the self-join or the clusters"
        for what in ("join", "dbscan_dev"):
            h, p = [r[what]["median_ms"] for r in here], [r[what]["median_ms"] for r in parent]
            s["b_%s_here_ms" % what], s["b_%s_parent_ms" % what] = med(here, what), med(parent, what)
            s["b_%s_here_spread_ms" % what], s["b_%s_parent_spread_ms" % what] = spread(here, what), spread(parent, what)
            s["b_%s_difference_ms" % what] = abs(med(here, what) - med(parent, what))
            s["b_%s_turn_to_turn_ms" % what] = max(max(h) - min(h), max(p) - min(p))
            s["b_%s_inside_the_spread" % what] = s["b_%s_difference_ms" % what] <= s["b_%s_turn_to_turn_ms" % what]
if args.parent_lib and args.bench_steps > 0:
    runs = []
    for which in ("parent", "here") * args.turns:
        row = run_worker("bench", "bench", args.parent_lib if which == "parent" else None)
        row.update(build=which)
        print(json.dumps(row), file=sys.stderr, flush=True)
        runs.append(row)
    res["runs"] += runs
    h = [r["queries_per_s"] for r in runs if r["build"] == "here"]
    p = [r["queries_per_s"] for r in runs if r["build"] == "parent"]
    res["summary"]["bench"] = {"here_queries_per_s": statistics.median(h), "parent_queries_per_s": statistics.median(p),
                               "here_all": h, "parent_all": p,
                               "difference": abs(statistics.median(h) - statistics.median(p)),
                               "turn_to_turn": max(max(h) - min(h), max(p) - min(p))}
    res["summary"]["bench"]["inside_the_spread"] = (res["summary"]["bench"]["difference"] <=
                                                    res["summary"]["bench"]["turn_to_turn"])
res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
