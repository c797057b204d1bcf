"""hs_pssm_family_chain on one MI355X beside the family scan of the same library, and the unchanged paths against the
parent commit's library.

Shape (tools/pssm_family_sweep.py's): 10^7 synthetic 25-mers (hsearch_amd/synth.py) in sequences of 300 windows; the
profiles are the Euclidean equivalents of search centres -- S[p][a] = -sum_j (coords[a][j] - c[8 p + j])^2 --; nm = 16,
256, 4096 in families of 4 (m_group = m / 4, m_off = 3 (m % 4)), min_count = 1, no score filter (every segment reports
a row: the most the sink can be asked to write), gap_open = 4, gap_ext = 1.  The scores are negative squared distances,
so no link is ever taken (a link needs a positive chain behind it): the run measures the sink's machinery -- keys,
sort, segments, the bisections of every hit against the earlier runs -- and NOT chains of several blocks.  Two
thresholds:
  bench   t = -R^2 at R = 40: about one hit per profile
  heavy   one value for all profiles, the median over the first 16 profiles of the 0.999 quantile of their scores over
          the first 200 000 k-mers: over 10^7 k-mers a profile hits about 6 x 10^4 windows
Medians of --reps warm repetitions with [min, max], every worker a fresh process, the builds taking turns:
  (a) chain_dev   hs_pssm_family_chain_dev at max_shift = 0, 3 and 30: device pointers, the rows stay on the device
  (b) family_dev  hs_pssm_family_scan_dev on the same handle
  unchanged       with --parent-lib: hs_pssm_scan at the largest nm (bench threshold, host pointers),
                  hs_pssm_family_scan_dev at nm = 256 heavy, and one bench step (hs_query_dev at the bench shape), parent
                  against this build; this build's median is to lie inside the parent's own spread
Per nm and threshold: hits, segments, rows kept, ms of the routes, the device's ms_finalize of each.

Usage (GPU box): python tools/pssm_chain_sweep.py --out profiles/pssm_chain_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--nm", type=str, default="16,256,4096")
ap.add_argument("--family", type=int, default=4)
ap.add_argument("--spacing", type=int, default=3)
ap.add_argument("--seq-windows", type=int, default=300)
ap.add_argument("--heavy-quantile", type=float, default=0.999)
ap.add_argument("--shifts", type=str, default="0,3,30")
ap.add_argument("--gap-open", type=float, default=4.0)
ap.add_argument("--gap-extend", type=float, default=1.0)
ap.add_argument("--unchanged-seq-nm", type=int, default=256)
ap.add_argument("--bench-nq", type=int, default=100_000)
ap.add_argument("--bench-K", type=int, default=16)
ap.add_argument("--bench-L", type=int, default=8)
ap.add_argument("--bench-W", type=float, default=212.0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--turns", type=int, default=2, help="processes per arm and build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) chain | unchanged")
args = ap.parse_args()
NM = [int(x) for x in args.nm.split(",")]
SHIFTS = [int(x) for x in args.shifts.split(",")]


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, HsError, capi, synth
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

    codes = synth.make_db(args.n, args.k)
    centers, _ = synth.make_queries(codes, max(max(NM), args.unchanged_seq_nm), jitter=0.05)
    coords = synth.coords()
    res["n"] = args.n
    dev = torch.device("cuda", 0)
    id_start = np.append(np.arange(0, args.n, args.seq_windows), args.n).astype(np.uint64)
    n_seq = len(id_start) - 1
    d_ids = torch.from_numpy(id_start.astype(np.int64)).to(dev)

    def profiles(nm):
        c = centers[:nm].reshape(nm, args.k, 1, 8)
        return np.ascontiguousarray(-((coords[None, None, :, :] - c) ** 2).sum(axis=3))

    def heavy_threshold():   # from the contract's left-to-right sum over a sample
        S16, sample = profiles(16), codes[:200_000]
        acc = np.zeros((S16.shape[0], len(sample)))
        for p in range(args.k):
            acc = acc + S16[:, p, :][:, sample[:, p]]
        return float(np.median(np.quantile(acc, args.heavy_quantile, axis=1)))

    def scan_engine():   # the tables play no part in a scan: one small table
        a, b = synth.make_planes(args.k, 2, 1, args.bench_W)
        eng = Engine(args.k, 2, 1, args.bench_W, a, b)
        eng.index_build(codes)
        return eng

    def family_dev_call(eng, d_S, d_t, nm, d_g, n_groups, d_o):
        """(call(ptrs, cap), n_rows, n_hits) of hs_pssm_family_scan_dev"""
        fam = lambda ptrs, cap: eng.pssm_family_scan_dev(d_S.data_ptr(), d_t.data_ptr(), nm, d_g.data_ptr(), n_groups,
                                                         d_o.data_ptr(), d_ids.data_ptr(), n_seq, 1, 0, ptrs, cap)
        try:
            n_rows, n_hits = fam([0] * 10, 0)
        except HsError as e:
            n_rows, n_hits = e.needed, e.n_hits
        return fam, n_rows, n_hits

    def row_arrays(fields, n):
        return [torch.empty(n + 1, dtype=torch.float64 if ty == np.float64 else torch.int32, device=dev) for _, ty in fields]

    def groups(nm):
        m_group = (np.arange(nm) // args.family).astype(np.uint32)
        m_off = ((np.arange(nm) % args.family) * args.spacing).astype(np.uint32)
        return (int(m_group[-1]) + 1, torch.from_numpy(m_group.astype(np.int32)).to(dev),
                torch.from_numpy(m_off.astype(np.int32)).to(dev))

    t_heavy = heavy_threshold()
    res.update(n_seq=n_seq, t_heavy=t_heavy, t_bench=-args.R * args.R)
    if mode == "chain":
        eng = scan_engine()
        for nm in NM:
            d_S = torch.from_numpy(profiles(nm)).to(dev)
            n_groups, d_g, d_o = groups(nm)
            for name, tv in (("bench", -args.R * args.R), ("heavy", t_heavy)):
                d_t = torch.from_numpy(np.full(nm, tv)).to(dev)
                torch.cuda.synchronize()
                row = {"t": tv}
                for shift in SHIFTS:
                    chain = lambda ptrs, cap: eng.pssm_family_chain_dev(
                        d_S.data_ptr(), d_t.data_ptr(), nm, d_g.data_ptr(), n_groups, d_o.data_ptr(), d_ids.data_ptr(),
                        n_seq, shift, args.gap_open, args.gap_extend, 1, 0, ptrs, cap)
                    try:
                        n_rows, n_hits = chain([0] * 10, 0)
                    except HsError as e:
                        n_rows, n_hits = e.needed, e.n_hits
                    rows = row_arrays(capi.PSSM_CHAIN_FIELDS, n_rows)
                    ptrs = [r.data_ptr() for r in rows]
                    torch.cuda.synchronize()

                    def chain_dev():
                        state["a"] = chain(ptrs, n_rows + 1)
                    arm = timed(chain_dev)
                    p = eng.profile()
                    arm.update(device_ms=p["ms_total"], finalize_ms=p["ms_finalize"], filter_ms=p["ms_verify"])
                    assert state["a"] == (n_rows, n_hits) and p["pssm_chain_kept"] == n_rows == p["pssm_chain_segs"]
                    row["a_chain_dev_%d" % shift] = arm
                    row.update(hits=n_hits, segs=p["pssm_chain_segs"], kept=n_rows, survivors=p["pssm_survivors"],
                               longest_chain=int(rows[2][:n_rows].max()) if n_rows else 0)
                    del rows
                fam, f_rows, f_hits = family_dev_call(eng, d_S, d_t, nm, d_g, n_groups, d_o)
                assert f_hits == row["hits"]
                rows = row_arrays(capi.PSSM_FAMILY_FIELDS, f_rows)
                ptrs = [r.data_ptr() for r in rows]
                torch.cuda.synchronize()

                def family_dev():
                    state["b"] = fam(ptrs, f_rows + 1)
                row["b_family_dev"] = timed(family_dev)
                p = eng.profile()
                row["b_family_dev"].update(device_ms=p["ms_total"], finalize_ms=p["ms_finalize"], filter_ms=p["ms_verify"])
                row["family_rows"] = f_rows
                del rows
                res["%s_%d" % (name, nm)] = row
                torch.cuda.empty_cache()
        eng.close()
    else:
        eng = scan_engine()
        nm = max(NM)
        S, t = profiles(nm), np.full(nm, -args.R * args.R)
        cap = len(eng.pssm_scan(S, t, want_counts=False)["m"]) + 1
        res["scan_%d" % nm] = timed(lambda: eng.pssm_scan(S, t, cap=cap, want_counts=False))
        nm = args.unchanged_seq_nm
        d_S = torch.from_numpy(profiles(nm)).to(dev)
        d_t = torch.from_numpy(np.full(nm, t_heavy)).to(dev)
        n_groups, d_g, d_o = groups(nm)
        fam, f_rows, _ = family_dev_call(eng, d_S, d_t, nm, d_g, n_groups, d_o)
        rows = row_arrays(capi.PSSM_FAMILY_FIELDS, f_rows)
        ptrs = [r.data_ptr() for r in rows]
        torch.cuda.synchronize()
        res["family_heavy_%d" % nm] = timed(lambda: fam(ptrs, f_rows + 1))
        eng.close()
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
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--nm", args.nm]
    argv += ["--shifts", args.shifts]
    for name in ("n", "k", "R", "family", "spacing", "seq_windows", "heavy_quantile", "gap_open", "gap_extend",
                 "unchanged_seq_nm", "bench_nq", "bench_K", "bench_L", "bench_W", "warmup", "reps"):
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
res = {"shape": {k: v for k, v in vars(args).items() if k not in ("worker", "out", "parent_lib")},
       "parent_lib": "the parent commit's build" if args.parent_lib else None,
       "taken": time.strftime("%Y-%m-%d"), "runs": [], "summary": {}}
order = []
for _ in range(args.turns):
    order.append(("chain", "here"))
    if args.parent_lib:
        order += [("unchanged", "parent"), ("unchanged", "here")]
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


def pooled(rows):
    if not rows:
        return None
    return {"median_ms": statistics.median(r["median_ms"] for r in rows), "min_ms": min(r["min_ms"] for r in rows),
            "max_ms": max(r["max_ms"] for r in rows), "turns": len(rows)}


chain_runs = [r for r in res["runs"] if r["mode"] == "chain"]
if chain_runs:
    s["t_heavy"], s["n_seq"] = chain_runs[-1]["t_heavy"], chain_runs[-1]["n_seq"]
for nm in NM:
    for name in ("bench", "heavy"):
        cases = [r["%s_%d" % (name, nm)] for r in chain_runs if "%s_%d" % (name, nm) in r]
        if not cases:
            continue
        out = {f: cases[-1][f] for f in ("t", "hits", "segs", "kept", "family_rows", "survivors", "longest_chain")}
        for arm in ["a_chain_dev_%d" % sh for sh in SHIFTS] + ["b_family_dev"]:
            p = pooled([c[arm] for c in cases if arm in c])
            if p:
                p["finalize_ms"] = statistics.median(c[arm]["finalize_ms"] for c in cases)
                out[arm] = p
        for sh in SHIFTS:
            out["a_%d_over_b" % sh] = out["a_chain_dev_%d" % sh]["median_ms"] / out["b_family_dev"]["median_ms"]
        s["%s_%d" % (name, nm)] = out
for what in ("search_step", "scan_%d" % max(NM), "family_heavy_%d" % args.unchanged_seq_nm):
    p = pooled([r[what] for r in res["runs"] if r["mode"] == "unchanged" and r["build"] == "parent" and what in r])
    h = pooled([r[what] for r in res["runs"] if r["mode"] == "unchanged" and r["build"] == "here" and what in r])
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
