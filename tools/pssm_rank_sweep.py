"""hs_pssm_rank on one MI355X against the routes the parent commit's library offers, and the unchanged paths against
that library.  The protocol of tools/pssm_topk_sweep.py: 10^7 synthetic 25-mers, the Euclidean-equivalent profiles of
search centres, medians of --reps warm repetitions with [min, max], every worker a fresh process, the builds taking turns.

  (a) rank       hs_pssm_rank_dev on this build, nm x rank, with its three phases (ms_hash: sample pass + its select,
                 ms_verify: tables + filter, ms_finalize: exact pass + select), the hits scanned per rank and the
                 retries; and the sample sizes --samples at --sample-nm x --sample-rank
  (b) oracle     with --parent-lib: hs_pssm_scan_dev by THAT library at the ORACLE threshold -- t_rank, taken from (a).
                 The floor: it needs the answer in advance
  (c) nothresh   with --parent-lib, the smallest nm only: that library's hs_pssm_scan with host pointers at -DBL_MAX plus
                 the selection on the host (numpy partition per profile): the route a user has today
  unchanged      with --parent-lib: hs_pssm_scan at the largest nm (t = -R^2), hs_pssm_topk at nm = 256 with topk = 10
                 and one bench step (hs_query_dev at the bench shape), parent against this build; this build's median
                 is to lie inside the parent's own spread
Cells named in --skip ("nm:rank,...") are left out and listed in the result.

Usage (GPU box): python tools/pssm_rank_sweep.py --out profiles/pssm_rank_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, tempfile, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--nm", type=str, default="16,256,4096")
ap.add_argument("--rank", type=str, default="100,10000,100000")
ap.add_argument("--skip", type=str, default="", help="cells left out, as nm:rank,nm:rank")
ap.add_argument("--samples", type=str, default="16384,65536,262144")
ap.add_argument("--sample-nm", type=int, default=4096)
ap.add_argument("--sample-rank", type=int, default=10000)
ap.add_argument("--bench-nq", type=int, default=100_000)
ap.add_argument("--bench-K", type=int, default=16)
ap.add_argument("--bench-L", type=int, default=8)
ap.add_argument("--bench-W", type=float, default=212.0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--turns", type=int, default=2, help="processes per arm and build, taking turns")
ap.add_argument("--worker-limit", type=int, default=420, help="seconds a worker process may run")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) rank | parent | unchanged")
ap.add_argument("--oracle-file", type=str, default=None, help="(internal) the oracle thresholds, written by rank")
args = ap.parse_args()
NM = [int(x) for x in args.nm.split(",")]
RANKS = [int(x) for x in args.rank.split(",")]
SAMPLES = [int(x) for x in args.samples.split(",")]
SKIP = {tuple(int(v) for v in c.split(":")) for c in args.skip.split(",") if c}
CELLS = [(nm, rank) for nm in NM for rank in RANKS if (nm, rank) not in SKIP]
ALL = -1.7976931348623157e308


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, HsError, synth
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
    centers, _ = synth.make_queries(codes, max(NM + [args.sample_nm, 256]), jitter=0.05)
    coords = synth.coords()

    def profiles(nm):
        c = centers[:nm].reshape(nm, args.k, 1, 8)
        return np.ascontiguousarray(-((coords[None, None, :, :] - c) ** 2).sum(axis=3))

    def scan_engine():   # the tables play no part in a scan: one small table
        a, b = synth.make_planes(args.k, 2, 1, args.bench_W)
        eng = Engine(args.k, 2, 1, args.bench_W, a, b)
        eng.index_build(codes)
        return eng

    def rank_call(eng, nm, rank):
        d_S = torch.from_numpy(profiles(nm)).to(dev)
        d_r = torch.full((nm,), rank, dtype=torch.int64, device=dev)
        d_t = torch.empty(nm, dtype=torch.float64, device=dev)
        d_ge, d_gt = (torch.empty(nm, dtype=torch.int64, device=dev) for _ in range(2))
        d_ro = torch.empty(nm, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def call():
            eng.pssm_rank_dev(d_S.data_ptr(), d_r.data_ptr(), nm, d_t.data_ptr(), d_ge.data_ptr(), d_gt.data_ptr(), None,
                              d_ro.data_ptr())
        return call, d_t, d_ge, d_ro

    def rank_row(eng, nm, rank):
        call, d_t, d_ge, d_ro = rank_call(eng, nm, rank)
        row = timed(call)
        p = eng.profile()
        row.update(sample_select_ms=p["ms_hash"], filter_ms=p["ms_verify"], exact_select_ms=p["ms_finalize"],
                   device_ms=p["ms_total"], survivors=p["pssm_survivors"], hits=p["hits"],
                   hits_per_rank=p["hits"] / (nm * rank), cnt_ge_per_rank=float(d_ge.sum().item()) / (nm * rank),
                   retries=p["pssm_rank_retries"], rounds_max=int(d_ro.max().item()), sample=p["pssm_rank_sample"])
        return row, d_t.cpu().numpy()

    if mode == "rank":
        eng = scan_engine()
        oracle = {}
        for nm, rank in CELLS:
            row, t = rank_row(eng, nm, rank)
            res["rank_%d_%d" % (nm, rank)] = row
            oracle["t_%d_%d" % (nm, rank)] = t
        for sample in SAMPLES:
            eng.set_option("pssm_rank_sample", sample)
            res["sample_%d" % sample], _ = rank_row(eng, args.sample_nm, args.sample_rank)
        eng.close()
        if args.oracle_file:
            np.savez(args.oracle_file, **oracle)
    elif mode == "parent":
        eng = scan_engine()
        oracle = np.load(args.oracle_file)
        for nm, rank in CELLS:
            t = oracle["t_%d_%d" % (nm, rank)]
            d_S, d_t = torch.from_numpy(profiles(nm)).to(dev), torch.from_numpy(t).to(dev)
            torch.cuda.synchronize()
            try:     # capacity 0 asks for the count
                cap = eng.pssm_scan_dev(d_S.data_ptr(), d_t.data_ptr(), nm, 0, 0, 0, 0) + 1
            except HsError as e:
                cap = int(e.n_hits) + 1
            d_m, d_id = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
            d_sc = torch.empty(cap, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()

            def call():
                state["hits"] = eng.pssm_scan_dev(d_S.data_ptr(), d_t.data_ptr(), nm, d_m.data_ptr(), d_id.data_ptr(),
                                                  d_sc.data_ptr(), cap)
            row = timed(call)
            row.update(hits=state["hits"])
            res["oracle_%d_%d" % (nm, rank)] = row
            del d_m, d_id, d_sc
        nm = NM[0]
        S, t = profiles(nm), np.full(nm, ALL)
        cap = nm * args.n
        for rank in RANKS:
            if (nm, rank) in SKIP:
                continue

            def nothresh():
                h = eng.pssm_scan(S, t, cap=cap, want_counts=False)
                sc = h["score"].reshape(nm, args.n)          # (m, id) order, every k-mer a hit
                state["t"] = -np.partition(-sc, rank - 1, axis=1)[:, rank - 1]
            row = timed(nothresh, reps=3, warmup=1)
            row.update(same_t=bool(np.array_equal(state["t"], oracle["t_%d_%d" % (nm, rank)])))
            res["nothresh_%d_%d" % (nm, rank)] = row
        eng.close()
    else:
        eng = scan_engine()
        nm = NM[-1]
        S, t = profiles(nm), np.full(nm, -args.R * args.R)
        cap = len(eng.pssm_scan(S, t, want_counts=False)["m"]) + 1
        res["scan_%d" % nm] = timed(lambda: eng.pssm_scan(S, t, cap=cap, want_counts=False))
        S256 = profiles(256)
        res["topk_256_10"] = timed(lambda: eng.pssm_topk(S256, 10))
        eng.close()
        a, b = synth.make_planes(args.k, args.bench_K, args.bench_L, args.bench_W)
        q, _ = synth.make_queries(codes, args.bench_nq, jitter=0.05)
        eng = Engine(args.k, args.bench_K, args.bench_L, args.bench_W, a, b)
        eng.index_build(codes)
        d_c = torch.from_numpy(q).to(dev)
        cap = 64 * args.bench_nq
        d_q, d_id, d_t = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
        d_d = torch.empty(cap, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def step():
            state["hits"] = eng.query_dev(d_c.data_ptr(), args.bench_nq, args.R, d_q.data_ptr(), d_id.data_ptr(),
                                          d_t.data_ptr(), d_d.data_ptr(), cap)
        res["search_step"] = timed(step)
        res["n_hits"] = state["hits"]
        eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(mode, lib, oracle_file):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--nm", args.nm, "--rank", args.rank,
            "--skip", args.skip, "--samples", args.samples, "--oracle-file", oracle_file]
    for name in ("n", "k", "R", "sample_nm", "sample_rank", "bench_nq", "bench_K", "bench_L", "bench_W", "warmup", "reps"):
        argv += ["--" + name.replace("_", "-"), repr(getattr(args, name))]
    # every GPU step under a time limit of its own; a failed measurement ends the sweep: nothing else is started
    r = subprocess.run(["timeout", "-k", "10", str(args.worker_limit)] + argv, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("worker %s failed with status %d" % (mode, r.returncode))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


if args.worker:
    worker(args.worker)
    sys.exit(0)
shape = {k: v for k, v in vars(args).items() if k not in ("worker", "out", "oracle_file", "parent_lib")}
shape["parent_lib"] = "the parent commit's libhsearch_amd.so" if args.parent_lib else None
res = {"shape": shape, "taken": time.strftime("%Y-%m-%d"), "left_out": sorted("nm %d rank %d" % c for c in SKIP),
       "runs": [], "summary": {}}
order = []
for _ in range(args.turns):
    order.append(("rank", "here"))
    if args.parent_lib:
        order += [("parent", "parent"), ("unchanged", "parent"), ("unchanged", "here")]
with tempfile.TemporaryDirectory() as tmp:
    oracle_file = os.path.join(tmp, "oracle.npz")
    for mode, which in order:
        row = run_worker(mode, args.parent_lib if which == "parent" else None, oracle_file)
        row.update(build=which)
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["runs"].append(row)
        if args.out:   # what was measured so far survives a later worker's failure
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

s = res["summary"]


def pooled(mode, which, what):
    rows = [r[what] for r in res["runs"] if r["mode"] == mode and r["build"] == which and what in r]
    if not rows:
        return None
    out = {"median_ms": statistics.median(r["median_ms"] for r in rows), "min_ms": min(r["min_ms"] for r in rows),
           "max_ms": max(r["max_ms"] for r in rows), "turns": len(rows)}
    out.update({f: v for f, v in rows[-1].items() if f not in ("median_ms", "min_ms", "max_ms", "reps")})
    return out


def ratio(name, a, b):
    s[name] = a["median_ms"] / b["median_ms"]
    s[name + "_spread"] = [a["min_ms"] / b["max_ms"], a["max_ms"] / b["min_ms"]]


for nm, rank in CELLS:
    a = pooled("rank", "here", "rank_%d_%d" % (nm, rank))
    b = pooled("parent", "parent", "oracle_%d_%d" % (nm, rank))
    c = pooled("parent", "parent", "nothresh_%d_%d" % (nm, rank))
    if a:
        s["a_rank_%d_%d" % (nm, rank)] = a
    if b:
        s["b_oracle_parent_%d_%d" % (nm, rank)] = b
    if c:
        s["c_nothresh_parent_%d_%d" % (nm, rank)] = c
    if a and b:
        ratio("a_over_b_%d_%d" % (nm, rank), a, b)
    if a and c:
        ratio("a_over_c_%d_%d" % (nm, rank), a, c)
best = None
for sample in SAMPLES:
    r = pooled("rank", "here", "sample_%d" % sample)
    if r:
        s["sample_%d" % sample] = r
        if best is None or r["median_ms"] < best[1]:
            best = (sample, r["median_ms"])
if best:
    s["fastest_sample"] = best[0]
for what in ("scan_%d" % NM[-1], "topk_256_10", "search_step"):
    p, h = pooled("unchanged", "parent", what), pooled("unchanged", "here", what)
    if p and h:
        s["unchanged_%s_parent" % what], s["unchanged_%s_here" % what] = p, h
        s["unchanged_%s_verdict" % what] = ("inside" if p["min_ms"] <= h["median_ms"] <= p["max_ms"] else
                                               "faster" if h["median_ms"] < p["min_ms"] else "slower")
if res["runs"]:
    res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
