"""What shrinking an index costs (hs_index_remove) beside building it again, at the C2 shape (10^7 25-mers, K = 16,
L = 8, W = 200): a removal of m = 10^4, 10^5 and 10^6 random ids against hs_index_build of the n - m survivors by
ANOTHER build of the library (--parent-lib: the parent commit's).  Both calls take host pointers, so PCIe is in both,
as a caller pays it.  Every figure is a median of warm repetitions with [min, max]; every worker is a fresh process;
the builds take turns in one job.
  (a) remove     per m: the index of n rebuilt (untimed), then hs_index_remove of the ids with new_id handed back (timed),
                 and the same call without new_id; its phase split from hs_profile (ms_hash / ms_sort / ms_gather /
                 ms_total, dead buckets, retupled buckets, rebuilds)
  (b) rebuild    per m: hs_index_build of the n - m survivors, by the parent's library and by this one
  (c) unchanged  hs_index_build of n, one hs_index_append of 10^5 and one hs_query_codes_dev step (10^5 queries, R = 40),
                 parent and here taking turns: this build's medians must lie inside the spread of the parent's repeated
                 turns ("inside" / "outside")
Usage (GPU box): python tools/remove_sweep.py --out profiles/remove_sweep.json --parent-lib other/libhsearch_amd.so"""
import argparse, ctypes, json, os, statistics, subprocess, sys, time
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
ap.add_argument("--append", type=int, default=100_000)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--turns", type=int, default=2, help="processes per build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) remove | rebuild")
args = ap.parse_args()
MS = [int(x) for x in args.m.split(",")]
PHASES = ("ms_hash", "ms_sort", "ms_gather", "ms_total")


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, synth
    res = {"mode": mode, "gpu": torch.cuda.get_device_name(0)}
    A = synth.make_db(args.n, args.k)
    dead = {m: np.random.default_rng(200 + i).choice(args.n, size=m, replace=False).astype(np.uint32)
            for i, m in enumerate(MS)}
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

    if mode == "remove":
        for m in MS:
            phases = []
            new_id = np.zeros(args.n, dtype=np.uint32)      # (touched: the pages exist before the first copy)
            ptr = dead[m].ctypes.data_as(ctypes.c_void_p)

            def shrink(out):
                eng._check(eng._lib.hs_index_remove(eng._h, ptr, ctypes.c_uint64(m), out))
                phases.append(eng.profile())
            row = timed(lambda: shrink(new_id.ctypes.data_as(ctypes.c_void_p)), before=lambda: eng.index_build(A))
            last = phases[args.warmup:]
            for f in PHASES:
                row[f] = statistics.median(p[f] for p in last)
            row["dead_buckets"] = int(last[-1]["remove_dead_buckets"])
            row["retupled"] = int(last[-1]["remove_retupled"])
            row["rebuilds"] = int(max(p["remove_rebuilds"] for p in last))
            row["n_after"] = int(eng.index_info()["n"])
            row["survivors_in_new_id"] = int((new_id != 0xffffffff).sum())
            res["remove_%d" % m] = row
            res["remove_%d_no_new_id" % m] = timed(lambda: shrink(None), before=lambda: eng.index_build(A))
    else:
        for m in MS:
            keep = np.ones(args.n, dtype=bool)
            keep[dead[m]] = False
            rest = A[keep]
            res["build_%d" % (args.n - m)] = timed(lambda: eng.index_build(rest))
            del rest
        res["build_n"] = timed(lambda: eng.index_build(A))
        block = synth.make_query_codes(A, args.append, max_subst=2, seed=100)[0]
        res["append"] = timed(lambda: eng.index_append(block), before=lambda: eng.index_build(A))
        eng.index_build(A)
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
    for name in ("n", "k", "K", "L", "W", "R", "nq", "append", "warmup", "reps"):
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
res = {"shape": {k: v for k, v in vars(args).items() if k not in ("worker", "out", "parent_lib")},
       "taken": time.strftime("%Y-%m-%d"), "runs": [], "summary": {}}
order = []
for _ in range(args.turns):
    order += [("remove", "here")] + ([("rebuild", "parent")] if args.parent_lib else []) + [("rebuild", "here")]
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


rem = [r for r in res["runs"] if r["mode"] == "remove"]
for m in MS:
    key = "remove_%d" % m
    s[key] = over(rem, key)
    s[key + "_no_new_id"] = over(rem, key + "_no_new_id")
    for f in PHASES:
        s[key][f] = statistics.median(r[key][f] for r in rem)
    s[key].update(dead_buckets=rem[-1][key]["dead_buckets"], retupled=rem[-1][key]["retupled"],
                  rebuilds=max(r[key]["rebuilds"] for r in rem),
                  turn_medians_ms=[r[key]["median_ms"] for r in rem])   # (the call allocates: turns can differ)
UNCHANGED = ("build_n", "append", "query_codes_dev")
for which in ("parent", "here"):
    rows = [r for r in res["runs"] if r["mode"] == "rebuild" and r["build"] == which]
    if rows:
        for what in ["build_%d" % (args.n - m) for m in MS] + list(UNCHANGED):
            s["%s_%s" % (what, which)] = over(rows, what)
if args.parent_lib:
    for m in MS:   # the comparison the sweep is for
        s["remove_%d" % m]["parent_rebuild_over_remove"] = (s["build_%d_parent" % (args.n - m)]["median_ms"] /
                                                            s["remove_%d" % m]["median_ms"])
    for what in UNCHANGED:   # the yardstick: the parent's own spread over its turns
        lo, hi = s[what + "_parent"]["spread_ms"]
        s[what + "_verdict"] = "inside" if lo <= s[what + "_here"]["median_ms"] <= hi else "outside"
if res["runs"]:
    res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
