"""What growing an index costs (hs_index_append) beside building it again, at the C2 shape (10^7 25-mers, K = 16,
L = 8, W = 200): an append of m = 10^4, 10^5 and 10^6 k-mers -- mutated copies of indexed k-mers, so that most land in
occupied buckets -- against hs_index_build of n + m by ANOTHER build of the library (--parent-lib: the parent
commit's).  Both calls take host pointers, so PCIe is in both, as a caller pays it.  Every figure is a median of warm
repetitions with [min, max]; every worker is a fresh process; the builds take turns in one job.
  (a) append     per m: the index of n rebuilt (untimed), then hs_index_append of the block (timed); its phase split from
                 hs_profile (ms_hash / ms_sort / ms_gather / ms_total, new buckets, rebuilds)
  (b) rebuild    per m: hs_index_build of n + m, by the parent's library and by this one
  (c) unchanged  hs_index_build of n and one hs_query_codes_dev step (10^5 queries, R = 40), parent and here taking turns:
                 this build's medians must lie inside the spread of the parent's repeated turns ("inside" / "outside")
Usage (GPU box): python tools/append_sweep.py --out profiles/append_sweep.json --parent-lib other/libhsearch_amd.so"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--m", type=str, default="10000,100000,1000000")
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--K", type=int, default=16)
ap.add_argument("--L", type=int, default=8)
ap.add_argument("--W", type=float, default=200.0)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--nq", type=int, default=100_000)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--turns", type=int, default=2, help="processes per build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) append | rebuild")
args = ap.parse_args()
MS = [int(x) for x in args.m.split(",")]


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, synth
    res = {"mode": mode, "gpu": torch.cuda.get_device_name(0)}
    A = synth.make_db(args.n, args.k)
    blocks = {m: synth.make_query_codes(A, m, max_subst=2, seed=100 + i)[0] for i, m in enumerate(MS)}
    a, b = synth.make_planes(args.k, args.K, args.L, args.W)
    eng = Engine(args.k, args.K, args.L, args.W, a, b)

    def timed(call, before=None):
        ms = []
        for i in range(args.warmup + args.reps):
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()      # (the library's calls return with their stream drained)
            if i >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return summary(ms)

    if mode == "append":
        for m in MS:
            phases = []

            def grow():
                eng.index_append(blocks[m])
                phases.append(eng.profile())
            row = timed(grow, before=lambda: eng.index_build(A))
            last = phases[args.warmup:]
            for f in ("ms_hash", "ms_sort", "ms_gather", "ms_total"):
                row[f] = statistics.median(p[f] for p in last)
            row["new_buckets"] = int(last[-1]["append_new_buckets"])
            row["rebuilds"] = int(max(p["append_rebuilds"] for p in last))
            row["buckets_after"] = int(sum(eng.index_info()["n_buckets"]))
            res["append_%d" % m] = row
    else:
        for m in MS:
            both = np.concatenate([A, blocks[m]])
            res["build_%d" % (args.n + m)] = timed(lambda: eng.index_build(both))
            del both
        res["build_n"] = timed(lambda: eng.index_build(A))
        dev = torch.device("cuda", 0)
        qc, _ = synth.make_query_codes(A, args.nq)
        d_qc = torch.from_numpy(qc).to(dev)
        cap = 64 * args.nq
        d_q, d_id, d_t = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
        d_d = torch.empty(cap, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        hits = []
        res["query_codes_dev"] = timed(lambda: hits.append(eng.query_dev(d_qc.data_ptr(), args.nq, args.R, d_q.data_ptr(),
                                                                        d_id.data_ptr(), d_t.data_ptr(), d_d.data_ptr(),
                                                                        cap, codes=True)))
        res["n_hits"] = int(hits[-1])
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(mode, lib):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--m", args.m]
    for name in ("n", "k", "K", "L", "W", "R", "nq", "warmup", "reps"):
        argv += ["--" + name, repr(getattr(args, name))]
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:   # a failed measurement ends the sweep: nothing else is started
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("worker failed with status %d" % r.returncode)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


if args.worker:
    worker(args.worker)
    sys.exit(0)
res = {"shape": {k: v for k, v in vars(args).items() if k not in ("worker", "out")}, "taken": time.strftime("%Y-%m-%d"),
       "runs": [], "summary": {}}
order = []
for _ in range(args.turns):
    order += [("append", "here")] + ([("rebuild", "parent")] if args.parent_lib else []) + [("rebuild", "here")]
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


def over(rows, what):
    return {"median_ms": statistics.median(r[what]["median_ms"] for r in rows),
            "spread_ms": [min(r[what]["min_ms"] for r in rows), max(r[what]["max_ms"] for r in rows)]}


app = [r for r in res["runs"] if r["mode"] == "append"]
for m in MS:
    key = "append_%d" % m
    s[key] = over(app, key)
    for f in ("ms_hash", "ms_sort", "ms_gather", "ms_total"):
        s[key][f] = statistics.median(r[key][f] for r in app)
    s[key].update(new_buckets=app[-1][key]["new_buckets"], rebuilds=max(r[key]["rebuilds"] for r in app),
                  turn_medians_ms=[r[key]["median_ms"] for r in app])   # (the call allocates: turns can differ)
for which in ("parent", "here"):
    rows = [r for r in res["runs"] if r["mode"] == "rebuild" and r["build"] == which]
    if rows:
        for what in ["build_%d" % (args.n + m) for m in MS] + ["build_n", "query_codes_dev"]:
            s["%s_%s" % (what, which)] = over(rows, what)
if args.parent_lib:
    for m in MS:   # the comparison the sweep is for
        s["append_%d" % m]["parent_rebuild_over_append"] = (s["build_%d_parent" % (args.n + m)]["median_ms"] /
                                                            s["append_%d" % m]["median_ms"])
    for what in ("build_n", "query_codes_dev"):   # the yardstick: the parent's own spread over its turns
        lo, hi = s[what + "_parent"]["spread_ms"]
        s[what + "_verdict"] = "inside" if lo <= s[what + "_here"]["median_ms"] <= hi else "outside"
if res["runs"]:
    res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
