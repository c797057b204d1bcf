"""hs_cluster_weighted_profile and hs_cluster_pssm_cover on one MI355X against the raw cluster profile, the covering
radii and the host route, and the unchanged paths against the parent commit's library.

Shape: 10^7 synthetic 25-mers (hsearch_amd/synth.py); label sets of about 10^2, 10^4 and 10^6 clusters (label = a
uniform draw below the cluster count) and one cluster of everything; min_size 1, every array on the device.  Medians of
--reps warm repetitions with [min, max], every worker a fresh process, the builds taking turns:
  (a) weighted_dev   hs_cluster_weighted_profile_dev with counts, wsum and distinct            (this build)
  (b) profile_dev    hs_cluster_profile_dev with counts                                        (parent and this build)
  (c) host           the labels to the host + hs_pssm_weight_hits over the (row, member) tuples, the codes already
                     there (skipped where its tables would take more than --host-max-bytes)
  (d) cover_dev      hs_cluster_pssm_cover_dev, random profiles                                 (this build)
      radii_dev      hs_cluster_radii_dev against the profile's centroids                      (parent and this build)
  unchanged          with --parent-lib: profile_dev, radii_dev and one bench step (hs_query_dev at the bench shape),
                     parent against this build; this build's median is to lie inside the parent's spread

Usage (GPU box): python tools/cluster_pssm_sweep.py --out profiles/cluster_pssm_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--clusters", type=str, default="100,10000,1000000,1")
ap.add_argument("--host-max-bytes", type=int, default=8 << 30)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--bench-nq", type=int, default=100_000)
ap.add_argument("--bench-K", type=int, default=16)
ap.add_argument("--bench-L", type=int, default=8)
ap.add_argument("--bench-W", type=float, default=212.0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--turns", type=int, default=2, help="processes per arm and build, taking turns")
ap.add_argument("--worker-timeout", type=int, default=900)
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) new | base")
args = ap.parse_args()
CLUSTERS = [int(x) for x in args.clusters.split(",")]


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, capi, synth
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
    A = synth.coords().shape[0]
    cells = args.k * A
    a, b = synth.make_planes(args.k, 2, 1, args.bench_W)   # the tables play no part in a summary: one small table
    eng = Engine(args.k, 2, 1, args.bench_W, a, b)
    eng.index_build(codes)
    rng = np.random.default_rng(11)
    for c in CLUSTERS:
        label = rng.integers(0, c, size=args.n).astype(np.uint32)
        rows = len(np.unique(label))
        d_label = torch.from_numpy(label.view(np.int32)).to(dev)
        d_ol, d_osz = (torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(2))
        d_counts = torch.empty((rows, cells), dtype=torch.int32, device=dev)
        row = {"rows": rows}
        torch.cuda.synchronize()
        if mode == "new":
            d_wc = torch.empty((rows, cells), dtype=torch.int64, device=dev)
            d_ws = torch.empty(rows, dtype=torch.int64, device=dev)
            d_di = torch.empty(rows, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def weighted():
                state["rows"] = eng.cluster_weighted_profile_dev(d_label.data_ptr(), 1, d_ol.data_ptr(), d_osz.data_ptr(),
                                                                 d_counts.data_ptr(), d_wc.data_ptr(), d_ws.data_ptr(),
                                                                 d_di.data_ptr(), rows)
            row["a_weighted_dev"] = timed(weighted)
            row["a_weighted_dev"]["items"] = eng.profile()["summary_weight_items"]
            assert state["rows"] == rows and bool((d_wc.view(rows, args.k, A).sum(dim=2) == d_ws[:, None]).all())
            d_S = torch.randn((rows, cells), dtype=torch.float64, device=dev)
            d_ms = torch.empty(rows, dtype=torch.float64, device=dev)
            d_am = torch.empty(rows, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            row["d_cover_dev"] = timed(lambda: eng.cluster_pssm_cover_dev(d_label.data_ptr(), 1, d_S.data_ptr(), rows,
                                                                          d_ms.data_ptr(), d_am.data_ptr()))
            del d_S
            if rows * cells * 20 <= args.host_max_bytes:
                row_of = np.cumsum(np.bincount(label, minlength=c) > 0) - 1
                wc = d_wc.cpu().numpy().view(np.uint64).reshape(rows, args.k, A)

                def host():
                    lab = d_label.cpu().numpy().view(np.uint32)
                    got = capi.pssm_weight_hits(codes, A, row_of[lab], np.arange(args.n, dtype=np.uint32),
                                                np.zeros(args.n), rows)
                    state["c"] = got["wcounts"]
                row["c_host"] = timed(host, reps=args.host_reps, warmup=1)
                assert np.array_equal(state["c"], wc)
            else:
                row["c_host_skipped"] = "the host rule's tables would take %d bytes" % (rows * cells * 20)
            del d_wc
        else:
            d_cen = torch.empty((rows, 8 * args.k), dtype=torch.float64, device=dev)
            d_mx, d_rad = (torch.empty(rows, dtype=torch.float64, device=dev) for _ in range(2))
            d_med = torch.empty(rows, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            row["b_profile_dev"] = timed(lambda: eng.cluster_profile_dev(d_label.data_ptr(), 1, d_ol.data_ptr(),
                                                                         d_osz.data_ptr(), d_counts.data_ptr(),
                                                                         d_cen.data_ptr(), rows))
            row["d_radii_dev"] = timed(lambda: eng.cluster_radii_dev(d_label.data_ptr(), 1, d_cen.data_ptr(), rows,
                                                                     d_mx.data_ptr(), d_rad.data_ptr(), d_med.data_ptr()))
            del d_cen
        res["clusters_%d" % c] = row
        del d_counts, d_label
    eng.close()
    if mode == "base":
        a, b = synth.make_planes(args.k, args.bench_K, args.bench_L, args.bench_W)
        q, _ = synth.make_queries(codes, args.bench_nq, jitter=0.05)
        eng = Engine(args.k, args.bench_K, args.bench_L, args.bench_W, a, b)
        eng.index_build(codes)
        d_c = torch.from_numpy(q).to(dev)
        cap = 64 * args.bench_nq
        d_q, d_id, d_tb = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
        d_d = torch.empty(cap, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def step():
            state["hits"] = eng.query_dev(d_c.data_ptr(), args.bench_nq, args.R, d_q.data_ptr(), d_id.data_ptr(),
                                          d_tb.data_ptr(), d_d.data_ptr(), cap)
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
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--clusters", args.clusters]
    for name in ("n", "k", "R", "host_max_bytes", "host_reps", "bench_nq", "bench_K", "bench_L", "bench_W", "warmup",
                 "reps"):
        argv += ["--" + name.replace("_", "-"), repr(getattr(args, name))]
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=args.worker_timeout)
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
    order.append(("new", "here"))
    if args.parent_lib:
        order.append(("base", "parent"))
    order.append(("base", "here"))
for mode, which in order:
    row = run_worker(mode, args.parent_lib if which == "parent" else None)
    row.update(build=which)
    print(json.dumps(row), file=sys.stderr, flush=True)
    res["runs"].append(row)
    if args.out:   # what was measured so far survives a later worker's failure
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def pooled(rows):
    if not rows:
        return None
    out = {"median_ms": statistics.median(r["median_ms"] for r in rows), "min_ms": min(r["min_ms"] for r in rows),
           "max_ms": max(r["max_ms"] for r in rows), "turns": len(rows)}
    if "items" in rows[-1]:
        out["items"] = rows[-1]["items"]
    return out


def cell(mode, build, key, arm):
    return pooled([r[key][arm] for r in res["runs"] if r["mode"] == mode and r["build"] == build and arm in r.get(key, {})])


s = res["summary"]
base_build = "parent" if args.parent_lib else "here"
for c in CLUSTERS:
    key = "clusters_%d" % c
    out = {"rows": [r[key]["rows"] for r in res["runs"] if key in r][-1]}
    for arm in ("a_weighted_dev", "d_cover_dev", "c_host"):
        p = cell("new", "here", key, arm)
        if p:
            out[arm] = p
    skipped = [r[key]["c_host_skipped"] for r in res["runs"] if "c_host_skipped" in r.get(key, {})]
    if skipped:
        out["c_host_skipped"] = skipped[-1]
    out["b_profile_dev"] = cell("base", base_build, key, "b_profile_dev")
    out["d_radii_dev"] = cell("base", base_build, key, "d_radii_dev")
    out["a_over_b"] = out["a_weighted_dev"]["median_ms"] / out["b_profile_dev"]["median_ms"]
    out["cover_over_radii"] = out["d_cover_dev"]["median_ms"] / out["d_radii_dev"]["median_ms"]
    if "c_host" in out:
        out["c_over_a"] = out["c_host"]["median_ms"] / out["a_weighted_dev"]["median_ms"]
    s[key] = out
    if args.parent_lib:
        for arm in ("b_profile_dev", "d_radii_dev"):
            p, h = cell("base", "parent", key, arm), cell("base", "here", key, arm)
            s["unchanged_%s_%d" % (arm, c)] = {"parent": p, "here": h, "verdict": (
                "inside" if p["min_ms"] <= h["median_ms"] <= p["max_ms"] else
                "faster" if h["median_ms"] < p["min_ms"] else "slower")}
if args.parent_lib:
    p = pooled([r["search_step"] for r in res["runs"] if r["mode"] == "base" and r["build"] == "parent"])
    h = pooled([r["search_step"] for r in res["runs"] if r["mode"] == "base" and r["build"] == "here"])
    s["unchanged_search_step"] = {"parent": p, "here": h, "verdict": (
        "inside" if p["min_ms"] <= h["median_ms"] <= p["max_ms"] else "faster" if h["median_ms"] < p["min_ms"] else "slower")}
if res["runs"]:
    res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
