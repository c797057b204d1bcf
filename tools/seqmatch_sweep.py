"""What the per-sequence reduction (hs_seq_match_dev) costs against the list call it replaces -- every figure a median of
warm repetitions with [min, max], every worker a fresh process, one MI355X:
  (a) bench       the bench shape (bench.py: 10^7 25-mers, K = 16, L = 8, W = 212, R = 40) cut into sequences of 300
                  windows, 10^5 query codes in groups of 100 with their offset in the group as q_off: hs_seq_match_dev
                  against hs_query_codes_dev on the same arguments
  (b) k15         the hit-heavy shape of tools/hit_distribution_k15.py (k = 15: hundreds of hits per query), points as
                  queries: hs_seq_match_dev against hs_query_dev; the ratio is recorded whatever it is
  (c) host route  in the bench worker: hs_query_codes (the hits over PCIe) plus hs_seq_match_hits on the host, with
                  the bytes each route moves
  (d) unchanged   with --parent-lib: hs_query_codes_dev, hs_annotate_dev and hs_query_topk_dev at the bench shape for
                  that build of the library (another commit's) and this one, the two builds taking turns: this build's
                  medians must lie inside the spread of the other's repeated turns; the verdict is recorded as
                  "inside" or "outside"
Usage (GPU box): python tools/seqmatch_sweep.py --out profiles/seqmatch_sweep.json [--parent-lib other/libhsearch_amd.so]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--nq", type=int, default=100_000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--K", type=int, default=16)
ap.add_argument("--L", type=int, default=8)
ap.add_argument("--W", type=float, default=212.0)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--seq-len", type=int, default=300, help="windows per database sequence")
ap.add_argument("--group", type=int, default=100, help="queries per group")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--turns", type=int, default=2, help="with --parent-lib: processes per build, taking turns")
ap.add_argument("--parent-lib", type=str, default=None)
ap.add_argument("--skip", type=str, default="", help="comma list of workers left out: bench, k15, unchanged")
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--worker", type=str, default=None, help="(internal) bench | k15 | unchanged")
args = ap.parse_args()


def summary(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(mode):
    import numpy as np
    import torch
    from hsearch_amd import Engine, capi, synth
    dev = torch.device("cuda", 0)
    res = {"mode": mode, "gpu": torch.cuda.get_device_name(0)}
    state = {}
    k = 15 if mode == "k15" else args.k
    n, nq = args.n, args.nq

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

    codes = synth.make_db(n, k)
    a, b = synth.make_planes(k, args.K, args.L, args.W)
    if mode == "k15":
        queries, _ = synth.make_queries(codes, nq, seed=synth.SEED_QUERIES)
    else:
        queries, _ = synth.make_query_codes(codes, nq)
    as_codes = mode != "k15"
    eng = Engine(k, args.K, args.L, args.W, a, b)
    eng.index_build(codes)
    d_queries = torch.from_numpy(queries).to(dev)
    res.update(n=n, nq=nq, k=k)

    def list_call(cap):
        d_q, d_id, d_t = (torch.empty(max(cap, 1), dtype=torch.int32, device=dev) for _ in range(3))
        d_d = torch.empty(max(cap, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def step():
            state["hits"] = eng.query_dev(d_queries.data_ptr(), nq, args.R, d_q.data_ptr(), d_id.data_ptr(),
                                          d_t.data_ptr(), d_d.data_ptr(), cap, codes=as_codes)
        return step

    try:  # the two-call pattern, once
        list_call(64 * nq)()
    except capi.HsError as e:
        state["hits"] = e.needed
    n_hits = state["hits"]
    res["n_hits"] = n_hits
    res["query_dev"] = timed(list_call(n_hits))
    res["query_dev"]["bytes_out"] = n_hits * 20

    if mode == "unchanged":
        cap = min(n, n_hits)
        d_i = [torch.empty(max(cap, 1), dtype=torch.int32, device=dev) for _ in range(3)]
        d_d = torch.empty(max(cap, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def annotate():
            state["ann"] = eng.annotate_dev(d_queries.data_ptr(), nq, args.R, None, d_i[0].data_ptr(), d_i[1].data_ptr(),
                                            d_i[2].data_ptr(), d_d.data_ptr(), cap, codes=True)
        res["annotate_dev"] = timed(annotate)
        topk = 10
        t_i = [torch.empty(nq * topk, dtype=torch.int32, device=dev) for _ in range(2)]
        t_d = torch.empty(nq * topk, dtype=torch.float64, device=dev)
        t_c = torch.empty(nq, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def top():
            state["top"] = eng.query_topk_dev(d_queries.data_ptr(), nq, topk, args.R, None, t_i[0].data_ptr(),
                                              t_i[1].data_ptr(), t_d.data_ptr(), t_c.data_ptr(), codes=True)
        res["query_topk_dev"] = timed(top)
        assert state["top"] == n_hits
    else:
        id_start = np.append(np.arange(0, n, args.seq_len), n).astype(np.uint64)
        q_group = (np.arange(nq) // args.group).astype(np.uint32)
        q_off = (np.arange(nq) % args.group).astype(np.uint32)
        n_groups = int(q_group[-1]) + 1
        d_g, d_o = torch.from_numpy(q_group.view(np.int32)).to(dev), torch.from_numpy(q_off.view(np.int32)).to(dev)
        d_s = torch.from_numpy(id_start.view(np.int64)).to(dev)

        def rows_call(cap):
            bufs = [torch.empty(max(cap, 1), dtype=torch.float64 if t == np.float64 else torch.int32, device=dev)
                    for _, t in capi.SEQ_MATCH_FIELDS]
            torch.cuda.synchronize()

            def step():
                state["rows"] = eng.seq_match_dev(d_queries.data_ptr(), nq, args.R, None, d_g.data_ptr(), n_groups,
                                                  d_o.data_ptr(), d_s.data_ptr(), len(id_start) - 1,
                                                  [t.data_ptr() for t in bufs], cap, codes=as_codes)
            return step, bufs

        try:
            rows_call(0)[0]()
            n_rows = 0
        except capi.HsError as e:
            n_rows = e.needed
        step, bufs = rows_call(n_rows)
        res["seq_match_dev"] = timed(step)
        assert state["rows"] == (n_rows, n_hits), (state["rows"], n_rows, n_hits)
        res["n_rows"] = n_rows
        res["seq_match_dev"]["bytes_out"] = n_rows * 40
        if mode == "bench":  # the host route, PCIe included, checked against the device's rows
            def host_route():
                h = eng.query_codes(queries, args.R, cap=n_hits, want_cand=False)
                state["host"] = capi.seq_match_hits(h["q"], h["id"], h["dist"], nq, id_start, q_group=q_group,
                                                    n_groups=n_groups, q_off=q_off)
            res["host_route"] = timed(host_route, reps=3, warmup=1)
            res["host_route"]["bytes_over_pcie"] = n_hits * 20
            for (name, dtype), t in zip(capi.SEQ_MATCH_FIELDS, bufs):
                got = t[:n_rows].cpu().numpy()
                got = got if dtype == np.float64 else got.view(dtype)
                assert np.array_equal(got.view(np.uint64) if dtype == np.float64 else got,
                                      state["host"][name].view(np.uint64) if dtype == np.float64 else state["host"][name]), name
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(mode, lib):
    env = dict(os.environ)
    if lib:
        env["HSEARCH_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("HSEARCH_AMD_LIB", None)
    argv = [sys.executable, os.path.abspath(__file__), "--worker", mode]
    for name in ("n", "nq", "k", "K", "L", "W", "R", "seq_len", "group", "warmup", "reps"):
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
res = {"shape": {k: v for k, v in vars(args).items() if k not in ("worker", "out", "skip")},
       "taken": time.strftime("%Y-%m-%d"), "runs": [], "summary": {}}
skip = set(args.skip.split(","))
order = [(m, "here") for m in ("bench", "k15") if m not in skip]
if args.parent_lib and "unchanged" not in skip:
    order += [("unchanged", "parent"), ("unchanged", "here")] * args.turns
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
for row in res["runs"]:
    if row["mode"] == "unchanged":
        continue
    m = row["mode"]
    for what, v in row.items():
        if isinstance(v, dict):
            s["%s_%s_ms" % (m, what)] = v["median_ms"]
            s["%s_%s_spread_ms" % (m, what)] = [v["min_ms"], v["max_ms"]]
            for extra in ("bytes_out", "bytes_over_pcie"):
                if extra in v:
                    s["%s_%s_%s" % (m, what, extra)] = v[extra]
        elif what in ("n", "nq", "n_hits", "n_rows"):
            s["%s_%s" % (m, what)] = v
    if "seq_match_dev" in row:
        s["%s_seq_match_over_query" % m] = row["seq_match_dev"]["median_ms"] / row["query_dev"]["median_ms"]
CALLS = ("query_dev", "annotate_dev", "query_topk_dev")
med = lambda rows, what: statistics.median(r[what]["median_ms"] for r in rows)
spread = lambda rows, what: [min(r[what]["min_ms"] for r in rows), max(r[what]["max_ms"] for r in rows)]
for which in ("here", "parent"):
    un = [r for r in res["runs"] if r["mode"] == "unchanged" and r["build"] == which]
    for what in CALLS:
        if un:
            s["unchanged_%s_%s_ms" % (what, which)] = med(un, what)
            s["unchanged_%s_%s_spread_ms" % (what, which)] = spread(un, what)
if "unchanged_query_dev_parent_ms" in s:   # the yardstick: the parent's own spread over its turns
    for what in CALLS:
        lo, hi = s["unchanged_%s_parent_spread_ms" % what]
        s["unchanged_%s_verdict" % what] = "inside" if lo <= s["unchanged_%s_here_ms" % what] <= hi else "outside"
if res["runs"]:
    res["gpu"] = res["runs"][0]["gpu"]
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res["summary"], indent=1))
