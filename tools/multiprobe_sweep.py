"""Multi-probe LSH (hs_set_multiprobe) against more tables: for every (L, T, W) of a grid at the bench's shape,
radius recall against the exhaustive scan (hs_bruteforce) on a query subsample, candidates per query, queries/s
of a short timed loop, the phase times and the index's HBM.  --c2: the configs[2]-shape comparison instead (K = 20:
L = 8 with the smallest T of --c2-T that reaches radius recall >= 0.925 at some W <= 160, against L = 32, T = 0,
W = 160).
Usage (GPU box): python tools/multiprobe_sweep.py [--n 10000000 --queries 100000] --out profiles/x.json"""
import argparse, hashlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from hsearch_amd import Engine, synth


def kernel_source_hash():
    """sha256 over the sources of the search's kernels, the multi-probe ones included"""
    h = hashlib.sha256()
    for f in ("hs_join8.hip", "hs_join.hip", "hs_kernels.hip", "hs_internal.h", "hs_multiprobe.hip", "hs_capi.hip",
              "hs_capi_index.hip", "hs_handle.h"):
        h.update(open(os.path.join(ROOT, "hsearch_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--queries", type=int, default=100_000)
ap.add_argument("--k", type=int, default=25)
ap.add_argument("--K", type=int, default=16)
ap.add_argument("--R", type=float, default=40.0)
ap.add_argument("--L", type=str, default="2,4,8")
ap.add_argument("--T", type=str, default="0,4,8,16,32")
ap.add_argument("--W", type=str, default="120,160,212")
ap.add_argument("--recall-queries", type=int, default=2000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--c2", action="store_true")
ap.add_argument("--c2-T", type=str, default="2,4,8,16,32,63")
ap.add_argument("--c2-W", type=str, default="120,140,160")
ap.add_argument("--out", type=str, required=True)
args = ap.parse_args()
if args.c2:
    args.K = 20
codes = synth.make_db(args.n, args.k)
centers, _ = synth.make_queries(codes, args.queries)
dev = torch.device("cuda", 0)
d_centers = torch.from_numpy(centers).to(dev)
nr = min(args.recall_queries, args.queries)
truth = None
engines = {}


def engine(L, W):
    global truth
    key = (L, W)
    if key not in engines:
        for e in engines.values():
            e.close()
        engines.clear()
        a, b = synth.make_planes(args.k, args.K, L, W)
        e = Engine(args.k, args.K, L, W, a, b)
        e.index_build(codes)
        if truth is None:
            bf = e.bruteforce(centers[:nr], args.R)
            truth = set(zip(bf["q"].tolist(), bf["id"].tolist()))
        engines[key] = e
    return engines[key]


def point(L, T, W):
    eng = engine(L, W)
    eng.set_multiprobe(T)
    lsh = eng.query(centers[:nr], args.R, want_cand=False)
    found = set(zip(lsh["q"].tolist(), lsh["id"].tolist()))
    cap = [64 * args.queries]
    out = []

    def alloc():
        out[:] = [torch.empty(cap[0], dtype=torch.int32, device=dev) for _ in range(3)] + \
                 [torch.empty(cap[0], dtype=torch.float64, device=dev)]
    alloc()

    def step():
        try:
            return eng.query_dev(d_centers.data_ptr(), args.queries, args.R, out[0].data_ptr(),
                                 out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), cap[0])
        except Exception as e:   # HS_ERR_CAPACITY (.needed): room for every hit, then once more
            if not hasattr(e, "needed"):
                raise
            cap[0] = e.needed + 1024
            alloc()
            return eng.query_dev(d_centers.data_ptr(), args.queries, args.R, out[0].data_ptr(),
                                 out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), cap[0])
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    p = eng.profile()
    row = {"L": L, "T": T, "W": W, "radius_recall": len(truth & found) / max(len(truth), 1),
           "true_pairs": len(truth), "candidates_per_query": p["candidates"] / args.queries,
           "queries_per_s": args.queries / dt, "ms_per_step": dt * 1e3, "ms_hash": p["ms_hash"],
           "ms_probe": p["ms_probe"], "ms_verify": p["ms_verify"], "ms_total_device": p["ms_total"],
           "hits": p["hits"], "device_bytes": eng.index_info()["device_bytes"]}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


res = {"shape": vars(args), "kernel_source_hash": kernel_source_hash(),
       "gpu": torch.cuda.get_device_name(0), "taken": time.strftime("%Y-%m-%d")}
if not args.c2:
    rows = []
    for L in [int(x) for x in args.L.split(",")]:
        for W in [float(x) for x in args.W.split(",")]:
            for T in [int(x) for x in args.T.split(",")]:
                rows.append(point(L, T, W))
    res["sweep"] = rows
else:
    base = point(32, 0, 160.0)
    best = None
    tried = []
    for T in [int(x) for x in args.c2_T.split(",")]:
        for W in [float(x) for x in args.c2_W.split(",")]:
            r = point(8, T, W)
            tried.append(r)
            if r["radius_recall"] >= 0.925 and (best is None or r["queries_per_s"] > best["queries_per_s"]):
                best = r
        if best is not None:
            break
    res["c2_comparison"] = {"L32_T0_W160": base, "L8_tried": tried, "L8_smallest_T_reaching_0.925": best}
for e in engines.values():
    e.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({k: v for k, v in res.items() if k != "sweep"})[:2000])
