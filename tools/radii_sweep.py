"""What per-query radii (hs_query_radii_dev) cost, at the bench's default shape (10^7 25-mers, K = 16, L = 8, W = 212,
10^5 queries given as codes, R = 40), through the device-pointer entry points, every figure a median of warm
repetitions with its spread:
  scalar      hs_query_codes_dev -- with --parent-lib also for that build of the library (another commit's), the two
              builds taking turns in fresh processes of one session: the scalar path must not have changed
  uniform     hs_query_radii_dev with every radius = R: the cost of reading radii[q]
  mixed       90 % of the queries at R and 10 % at --R-wide in one call, against the sum of two scalar calls over
              the two subsets: the evidence for or against splitting a batch into a narrow-row and a wide-row class
Usage (GPU box): python tools/radii_sweep.py --out profiles/radii_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--queries", type=int, default=100_000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--K", type=int, default=16)
ap.add_argument("--L", type=int, default=8)
ap.add_argument("--W", type=float, default=212.0)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--R-wide", type=float, default=55.0)
ap.add_argument("--wide-share", type=float, default=0.1)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--turns", type=int, default=2, help="with --parent-lib: processes per build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", action="store_true", help="(internal) measure the library HSEARCH_AMD_LIB names")
args = ap.parse_args()


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1],
            "q1_ms": s[len(s) // 4], "q3_ms": s[(3 * len(s)) // 4], "reps": len(s)}


def worker():
    import numpy as np
    import torch
    from hsearch_amd import Engine, synth
    dev = torch.device("cuda", 0)
    codes = synth.make_db(args.n, args.k)
    qcodes, _ = synth.make_query_codes(codes, args.queries)
    a, b = synth.make_planes(args.k, args.K, args.L, args.W)
    eng = Engine(args.k, args.K, args.L, args.W, a, b)
    eng.index_build(codes)
    nq = args.queries
    rng = np.random.default_rng(11)
    wide = np.zeros(nq, dtype=bool)
    wide[rng.choice(nq, int(round(args.wide_share * nq)), replace=False)] = True
    radii = np.where(wide, args.R_wide, args.R)
    d_q = torch.from_numpy(qcodes).to(dev)
    d_narrow, d_wide = torch.from_numpy(qcodes[~wide]).to(dev), torch.from_numpy(qcodes[wide]).to(dev)
    d_uniform = torch.full((nq,), args.R, dtype=torch.float64, device=dev)
    d_mixed = torch.from_numpy(radii).to(dev)
    cap = 64 * nq
    out = [torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3)] + \
          [torch.empty(cap, dtype=torch.float64, device=dev)]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in out]

    def scalar(d, R):
        return lambda: eng.query_dev(d.data_ptr(), d.shape[0], R, *ptrs, cap, codes=True)

    def with_radii(d_r):
        return lambda: eng.query_radii_dev(d_q.data_ptr(), nq, d_r.data_ptr(), *ptrs, cap, codes=True)

    def timed(call):
        for _ in range(args.warmup):
            hits = call()
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()   # (returns with the hits on the device and the stream idle)
            ms.append((time.perf_counter() - t0) * 1e3)
        p = eng.profile()
        row = summary(ms)
        row.update(hits=int(hits), join_wide=p["join_wide"], ms_verify=p["ms_verify"], ms_join=p["ms_join"],
                   ms_finalize=p["ms_finalize"], ms_total_device=p["ms_total"], provisional=p["provisional"],
                   join_async_retries=p["join_async_retries"])
        return row
    res = {"scalar": timed(scalar(d_q, args.R))}
    if hasattr(eng._lib, "hs_query_radii_dev"):
        res["uniform_radii"] = timed(with_radii(d_uniform))
        res["mixed_radii"] = timed(with_radii(d_mixed))
        res["scalar_narrow_subset"] = timed(scalar(d_narrow, args.R))
        res["scalar_wide_subset"] = timed(scalar(d_wide, args.R_wide))
        res["scalar_again"] = timed(scalar(d_q, args.R))   # drift over the process
        assert res["uniform_radii"]["hits"] == res["scalar"]["hits"]
        assert res["mixed_radii"]["hits"] == res["scalar_narrow_subset"]["hits"] + res["scalar_wide_subset"]["hits"]
    res["gpu"] = torch.cuda.get_device_name(0)
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(lib):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker"]
    for name in ("n", "queries", "k", "K", "L", "W", "R", "R_wide", "wide_share", "warmup", "reps"):
        argv += ["--" + name.replace("_", "-"), repr(getattr(args, name))]
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:   # a failed measurement ends the sweep: nothing else is started
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("worker failed with status %d" % r.returncode)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


if args.worker:
    worker()
    sys.exit(0)
res = {"shape": {k: v for k, v in vars(args).items() if k not in ("worker", "out")}, "taken": time.strftime("%Y-%m-%d"),
       "runs": []}
order = (["parent", "here"] * args.turns) if args.parent_lib else ["here"]
for which in order:
    row = run_worker(args.parent_lib if which == "parent" else None)
    row["build"] = which
    print(json.dumps(row), file=sys.stderr, flush=True)
    res["runs"].append(row)
here = [r for r in res["runs"] if r["build"] == "here"]
parent = [r for r in res["runs"] if r["build"] == "parent"]
med = lambda rows, what: statistics.median(r[what]["median_ms"] for r in rows)
res["gpu"] = here[0]["gpu"]
s = res["summary"] = {"scalar_here_ms": med(here, "scalar"),
                      "scalar_here_spread_ms": [min(r["scalar"]["min_ms"] for r in here), max(r["scalar"]["max_ms"] for r in here)]}
if parent:
    s["scalar_parent_ms"] = med(parent, "scalar")
    s["scalar_parent_spread_ms"] = [min(r["scalar"]["min_ms"] for r in parent), max(r["scalar"]["max_ms"] for r in parent)]
    s["scalar_here_over_parent"] = s["scalar_here_ms"] / s["scalar_parent_ms"]
s["uniform_radii_ms"] = med(here, "uniform_radii")
s["uniform_over_scalar"] = s["uniform_radii_ms"] / s["scalar_here_ms"]
s["mixed_radii_ms"] = med(here, "mixed_radii")
s["two_scalar_calls_ms"] = med(here, "scalar_narrow_subset") + med(here, "scalar_wide_subset")
s["mixed_over_two_calls"] = s["mixed_radii_ms"] / s["two_scalar_calls_ms"]
s["mixed_join_wide"] = here[0]["mixed_radii"]["join_wide"]
s["mixed_ms_verify"] = med(here, "mixed_radii") and statistics.median(r["mixed_radii"]["ms_verify"] for r in here)
s["scalar_ms_verify"] = statistics.median(r["scalar"]["ms_verify"] for r in here)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(s, indent=1))
