// hs_density.hip -- the density tree of the near-neighbour graph (hs_core_distance, hs_density_tree,
// include/hsearch.h): the core distance of every k-mer, found on the device from the self-join's unordered pairs, and
// the minimum spanning forest under the mutual-reachability distance by the Boruvka rounds of hs_msf.hip; the same
// rule on the host for any edge list (hs_density_tree_edges, hs_density_tree_cut).
//
// The rule.  d{a,b} is the distance the self-join reports for the pair (the same bits from both ends).  core[i] is the
// (min_pts - 1)-th smallest of the multiset { d{i,j} : j adjacent to i }, +0 for min_pts = 1, +inf when i has fewer
// neighbours.  w{a,b} = max(core[a], core[b], d{a,b}); a pair with an infinite end is no edge.  The tree is the minimum
// spanning forest under (w, lo, hi).
//
// Why (w, lo, hi) is a strict total order seen identically from both ends: core[] is final before the first Boruvka
// pass (the core pass ends at a kernel boundary and a stream synchronisation), d is the same bits from both ends, and
// max is symmetric, so the ordered pairs (a, b) and (b, a) and the kept entry {lo, hi} all compute the same 64 bits of
// w.  All three operands are >= +0 and none is a NaN, so their bit patterns order like the doubles and max on the bits
// is max on the doubles.  Ties in w -- mutual reachability makes many -- are broken by the pair, which is unique per
// edge.  That is all the argument at the head of hs_msf.hip asks for; the rounds <= ceil(log2 n) bound does not look
// at the weights at all.
//
// State, owned by the handle and sized by the index, on top of hs_msf's 56 bytes (28 bytes per indexed k-mer):
//   core [n] u64  the bits of the core distance; DT_OPEN -- the bits of no distance -- while the k-mer is unsettled
//   thr  [n] u64  the smallest bit pattern of a neighbour distance that is not yet counted (0 at the start)
//   next [n] u64  the smallest neighbour distance >= thr seen in this round; MSF_EMPTY: none
//   cnt  [n] u32  the neighbours counted so far: those with a distance < thr, with multiplicity
//
// The core pass.  The invariant it stands on (hs_capi.hip reduce_batch, run_query): ALL hits (a, .) of one k-mer a lie
// in ONE reduce_batch call -- a batch is a range of queries, the queries of a self-join are the k-mers themselves, and
// a batch cut in halves is cut by queries and handed on only once it came through whole -- and every ordered pair is
// there exactly once.  So the rounds below run per batch, over the batch's hit buffers while they are live, and only
// touch the state of the batch's own range of k-mers.  One round is three steps, each behind a kernel boundary, so
// that the next reads final words with plain loads:
//   1. next   every hit (a, ., d) of an open a with d >= thr[a] takes a 64-bit atomicMin(next + a, d) (the
//             peek-then-atomic early-out of msf_lower)
//   2. count  every hit of an open a with d == next[a] adds 1 to cnt[a]: three neighbours at one distance count thrice
//   3. settle one lane per k-mer of the batch's range: cnt >= min_pts - 1: core = next, settled; next empty: no
//             neighbour is left, core = +inf, settled; otherwise thr = next + 1, next emptied, and the k-mer is counted
//             as still open
// Every round moves thr of an open k-mer past at least one more neighbour, so min_pts - 1 rounds settle everything;
// the host reads the open count back after every round (8 bytes; the stream is idle between batches anyway) and stops
// at zero -- with low degrees that is long before min_pts - 1.  The result does not depend on any order: a min, and
// integer adds.  Step 2 is NOT idempotent; it relies on every ordered pair coming once, as hs_dbscan's degrees do.
// All stores are vector stores.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_msf_round.h"
#include "hs_unionfind.h"

namespace {

#define DT_OPEN MSF_EMPTY
#define DT_INF 0x7ff0000000000000ull

__global__ __launch_bounds__(256) void hs_dt_begin_kernel(u64* __restrict__ core, u64* __restrict__ thr,
                                                          u64* __restrict__ next, uint32_t* __restrict__ cnt,
                                                          uint32_t n, u64 core0) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  core[i] = core0;
  thr[i] = 0ull;
  next[i] = MSF_EMPTY;
  cnt[i] = 0u;
}

// the batch's ordered pairs counted; KEEP: those with a < b appended to `kept` with their RAW distance bits (while
// there is room: the counter keeps running, so the caller sees an overflow)
template <bool KEEP>
__global__ __launch_bounds__(256) void hs_dt_pairs_kernel(const uint64_t* __restrict__ key,
                                                          const uint64_t* __restrict__ val, uint32_t n_hits,
                                                          uint32_t self_first, uint32_t n, u64* __restrict__ counts,
                                                          ulonglong2* __restrict__ kept, u64 kept_cap) {
  const MsfPair p = msf_load_hit(key, val, blockIdx.x * 256u + threadIdx.x, n_hits, self_first, n);
  cc_count(p.live, counts + MSF_N_PAIRS);
  if (KEEP) {
    const bool mine = p.live && p.a < p.b;
    const u64 pos = msf_append_pos(mine, counts + MSF_N_KEPT);
    if (mine && pos < kept_cap) kept[pos] = make_ulonglong2((u64)p.a << 32 | p.b, p.d);
  }
}

// step 1 (core and thr were written by earlier kernels: plain loads)
__global__ __launch_bounds__(256) void hs_dt_next_kernel(const uint64_t* __restrict__ key,
                                                         const uint64_t* __restrict__ val, uint32_t n_hits,
                                                         uint32_t self_first, uint32_t n,
                                                         const u64* __restrict__ core, const u64* __restrict__ thr,
                                                         u64* __restrict__ next) {
  const MsfPair p = msf_load_hit(key, val, blockIdx.x * 256u + threadIdx.x, n_hits, self_first, n);
  if (p.live && core[p.a] == DT_OPEN && p.d >= thr[p.a]) msf_lower(next + p.a, p.d);
}

// step 2 (next is final: step 1 ended at a kernel boundary)
__global__ __launch_bounds__(256) void hs_dt_count_kernel(const uint64_t* __restrict__ key,
                                                          const uint64_t* __restrict__ val, uint32_t n_hits,
                                                          uint32_t self_first, uint32_t n,
                                                          const u64* __restrict__ core, const u64* __restrict__ next,
                                                          uint32_t* __restrict__ cnt) {
  const MsfPair p = msf_load_hit(key, val, blockIdx.x * 256u + threadIdx.x, n_hits, self_first, n);
  if (p.live && core[p.a] == DT_OPEN && p.d == next[p.a]) atomicAdd(cnt + p.a, 1u);
}

// step 3 over the k-mers [first, first + count) (count is a multiple of nothing: every lane checks its bound)
__global__ __launch_bounds__(256) void hs_dt_settle_kernel(uint32_t first, uint32_t count, uint32_t need,
                                                           u64* __restrict__ core, u64* __restrict__ thr,
                                                           u64* __restrict__ next, const uint32_t* __restrict__ cnt,
                                                           u64* __restrict__ counts) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  bool open = false;
  if (t < count) {
    const uint32_t i = first + t;
    if (core[i] == DT_OPEN) {
      const u64 nx = next[i];
      if (nx == MSF_EMPTY) {
        core[i] = DT_INF;
      } else if (cnt[i] >= need) {
        core[i] = nx;
      } else {
        thr[i] = nx + 1ull;
        next[i] = MSF_EMPTY;
        open = true;
      }
    }
  }
  cc_count(open, counts + MSF_N_OPEN);
}

// behind the core pass: a k-mer no batch settled (an index whose self-join ran no batch) has no neighbour; the
// finite ones counted
__global__ __launch_bounds__(256) void hs_dt_core_finish_kernel(u64* __restrict__ core, uint32_t n,
                                                                u64* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool finite = false;
  if (i < n) {
    u64 c = core[i];
    if (c == DT_OPEN) core[i] = c = DT_INF;
    finite = c < DT_INF;
  }
  cc_count(finite, counts + MSF_N_CORE);
}

// the mutual-reachability weight in place of the distance; a pair with an infinite end is not live
__device__ __forceinline__ MsfPair dt_weigh(MsfPair p, const u64* __restrict__ core) {
  if (p.live) {
    const u64 ca = core[p.a], cb = core[p.b];
    const u64 m = ca > cb ? ca : cb;
    p.d = p.d > m ? p.d : m;
    p.live = p.d < DT_INF;
  }
  return p;
}

__global__ __launch_bounds__(256) void hs_dt_min_d_hits_kernel(const uint64_t* __restrict__ key,
                                                               const uint64_t* __restrict__ val, uint32_t n_hits,
                                                               uint32_t self_first, const u64* __restrict__ core,
                                                               const uint32_t* __restrict__ comp,
                                                               u64* __restrict__ best_d, uint32_t n,
                                                               u64* __restrict__ counts) {
  const MsfPair p = dt_weigh(msf_load_hit(key, val, blockIdx.x * 256u + threadIdx.x, n_hits, self_first, n), core);
  const bool cross = p.live && msf_min_d(comp, best_d, p.a, p.b, p.d, false);
  cc_count(cross, counts + MSF_N_CROSS);
}

__global__ __launch_bounds__(256) void hs_dt_min_pair_hits_kernel(const uint64_t* __restrict__ key,
                                                                  const uint64_t* __restrict__ val, uint32_t n_hits,
                                                                  uint32_t self_first, const u64* __restrict__ core,
                                                                  const uint32_t* __restrict__ comp,
                                                                  const u64* __restrict__ best_d,
                                                                  u64* __restrict__ best_pair, uint32_t n) {
  const MsfPair p = dt_weigh(msf_load_hit(key, val, blockIdx.x * 256u + threadIdx.x, n_hits, self_first, n), core);
  if (p.live) msf_min_pair(comp, best_d, best_pair, p.a, p.b, p.d, false);
}

__global__ __launch_bounds__(256) void hs_dt_min_d_kept_kernel(const ulonglong2* __restrict__ kept, u64 n_kept,
                                                               const u64* __restrict__ core,
                                                               const uint32_t* __restrict__ comp,
                                                               u64* __restrict__ best_d, uint32_t n,
                                                               u64* __restrict__ counts) {
  const MsfPair p = dt_weigh(msf_load_kept(kept, (u64)blockIdx.x * 256u + threadIdx.x, n_kept, n), core);
  const bool cross = p.live && msf_min_d(comp, best_d, p.a, p.b, p.d, true);
  cc_count(cross, counts + MSF_N_CROSS);
}

__global__ __launch_bounds__(256) void hs_dt_min_pair_kept_kernel(const ulonglong2* __restrict__ kept, u64 n_kept,
                                                                  const u64* __restrict__ core,
                                                                  const uint32_t* __restrict__ comp,
                                                                  const u64* __restrict__ best_d,
                                                                  u64* __restrict__ best_pair, uint32_t n) {
  const MsfPair p = dt_weigh(msf_load_kept(kept, (u64)blockIdx.x * 256u + threadIdx.x, n_kept, n), core);
  if (p.live) msf_min_pair(comp, best_d, best_pair, p.a, p.b, p.d, true);
}

// the labels (label != null) and the clusters counted (counts != null): a k-mer without a finite core distance is
// noise, the others carry their component
__global__ __launch_bounds__(256) void hs_dt_finish_kernel(const uint32_t* __restrict__ comp,
                                                           const u64* __restrict__ core, uint32_t n,
                                                           uint32_t* __restrict__ label, u64* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool root = false;
  if (i < n) {
    const bool finite = core[i] < DT_INF;
    const uint32_t c = comp[i];
    if (label) label[i] = finite ? c : HS_NOISE;
    root = finite && c == i;
  }
  if (counts) cc_count(root, counts + MSF_N_ROOTS);
}

}  // namespace

hipError_t hs_launch_dt_begin(uint64_t* d_core, uint64_t* d_thr, uint64_t* d_next, uint32_t* d_cnt, uint32_t n,
                              uint32_t min_pts, hipStream_t s) {
  if (!n) return hipSuccess;
  hs_dt_begin_kernel<<<cc_blocks(n), 256, 0, s>>>(reinterpret_cast<u64*>(d_core), reinterpret_cast<u64*>(d_thr),
                                                 reinterpret_cast<u64*>(d_next), d_cnt, n,
                                                 min_pts <= 1 ? 0ull : DT_OPEN);
  return hipGetLastError();
}

hipError_t hs_launch_dt_pairs(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits, uint32_t self_first,
                              uint32_t n, uint64_t* d_counts, void* d_kept, uint64_t kept_cap, hipStream_t s) {
  if (!n_hits) return hipSuccess;
  u64* const cn = reinterpret_cast<u64*>(d_counts);
  if (d_kept)
    hs_dt_pairs_kernel<true><<<cc_blocks(n_hits), 256, 0, s>>>(d_key, d_val, n_hits, self_first, n, cn,
                                                              reinterpret_cast<ulonglong2*>(d_kept), kept_cap);
  else
    hs_dt_pairs_kernel<false><<<cc_blocks(n_hits), 256, 0, s>>>(d_key, d_val, n_hits, self_first, n, cn, nullptr, 0);
  return hipGetLastError();
}

hipError_t hs_launch_dt_round(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits, uint32_t self_first,
                              uint32_t n, uint32_t first, uint32_t count, uint32_t min_pts, uint64_t* d_core,
                              uint64_t* d_thr, uint64_t* d_next, uint32_t* d_cnt, uint64_t* d_counts, hipStream_t s) {
  if (!count) return hipSuccess;
  if (first >= n || count > n - first) return hipErrorInvalidValue;  // the range must lie inside the state arrays
  u64* const core = reinterpret_cast<u64*>(d_core);
  u64* const thr = reinterpret_cast<u64*>(d_thr);
  u64* const next = reinterpret_cast<u64*>(d_next);
  if (n_hits) {
    hs_dt_next_kernel<<<cc_blocks(n_hits), 256, 0, s>>>(d_key, d_val, n_hits, self_first, n, core, thr, next);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hs_dt_count_kernel<<<cc_blocks(n_hits), 256, 0, s>>>(d_key, d_val, n_hits, self_first, n, core, next, d_cnt);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hs_dt_settle_kernel<<<cc_blocks(count), 256, 0, s>>>(first, count, min_pts - 1u, core, thr, next, d_cnt,
                                                      reinterpret_cast<u64*>(d_counts));
  return hipGetLastError();
}

hipError_t hs_launch_dt_core_finish(uint64_t* d_core, uint32_t n, uint64_t* d_counts, hipStream_t s) {
  if (!n) return hipSuccess;
  hs_dt_core_finish_kernel<<<cc_blocks(n), 256, 0, s>>>(reinterpret_cast<u64*>(d_core), n,
                                                       reinterpret_cast<u64*>(d_counts));
  return hipGetLastError();
}

hipError_t hs_launch_dt_min_d_hits(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits, uint32_t self_first,
                                   const uint64_t* d_core, const uint32_t* d_comp, uint64_t* d_best_d, uint32_t n,
                                   uint64_t* d_counts, hipStream_t s) {
  if (!n_hits) return hipSuccess;
  hs_dt_min_d_hits_kernel<<<cc_blocks(n_hits), 256, 0, s>>>(d_key, d_val, n_hits, self_first,
                                                           reinterpret_cast<const u64*>(d_core), d_comp,
                                                           reinterpret_cast<u64*>(d_best_d), n,
                                                           reinterpret_cast<u64*>(d_counts));
  return hipGetLastError();
}

hipError_t hs_launch_dt_min_pair_hits(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits,
                                      uint32_t self_first, const uint64_t* d_core, const uint32_t* d_comp,
                                      const uint64_t* d_best_d, uint64_t* d_best_pair, uint32_t n, hipStream_t s) {
  if (!n_hits) return hipSuccess;
  hs_dt_min_pair_hits_kernel<<<cc_blocks(n_hits), 256, 0, s>>>(d_key, d_val, n_hits, self_first,
                                                              reinterpret_cast<const u64*>(d_core), d_comp,
                                                              reinterpret_cast<const u64*>(d_best_d),
                                                              reinterpret_cast<u64*>(d_best_pair), n);
  return hipGetLastError();
}

hipError_t hs_launch_dt_min_d_kept(const void* d_kept, uint64_t n_kept, const uint64_t* d_core, const uint32_t* d_comp,
                                   uint64_t* d_best_d, uint32_t n, uint64_t* d_counts, hipStream_t s) {
  if (!n_kept) return hipSuccess;
  hs_dt_min_d_kept_kernel<<<msf_blocks64(n_kept), 256, 0, s>>>(reinterpret_cast<const ulonglong2*>(d_kept), n_kept,
                                                              reinterpret_cast<const u64*>(d_core), d_comp,
                                                              reinterpret_cast<u64*>(d_best_d), n,
                                                              reinterpret_cast<u64*>(d_counts));
  return hipGetLastError();
}

hipError_t hs_launch_dt_min_pair_kept(const void* d_kept, uint64_t n_kept, const uint64_t* d_core,
                                      const uint32_t* d_comp, const uint64_t* d_best_d, uint64_t* d_best_pair,
                                      uint32_t n, hipStream_t s) {
  if (!n_kept) return hipSuccess;
  hs_dt_min_pair_kept_kernel<<<msf_blocks64(n_kept), 256, 0, s>>>(reinterpret_cast<const ulonglong2*>(d_kept), n_kept,
                                                                 reinterpret_cast<const u64*>(d_core), d_comp,
                                                                 reinterpret_cast<const u64*>(d_best_d),
                                                                 reinterpret_cast<u64*>(d_best_pair), n);
  return hipGetLastError();
}

hipError_t hs_launch_dt_finish(const uint32_t* d_comp, const uint64_t* d_core, uint32_t n, uint32_t* d_label,
                               uint64_t* d_counts, hipStream_t s) {
  if (!n) return hipSuccess;
  hs_dt_finish_kernel<<<cc_blocks(n), 256, 0, s>>>(d_comp, reinterpret_cast<const u64*>(d_core), n, d_label,
                                                  reinterpret_cast<u64*>(d_counts));
  return hipGetLastError();
}

// ---- the same rule on the host (no GPU, no handle) -------------------------------------------------------

extern "C" hs_status hs_density_tree_edges(const uint32_t* ei, const uint32_t* ej, const double* dist,
                                           uint64_t n_edges, uint64_t n, uint32_t min_pts, uint32_t* out_lo,
                                           uint32_t* out_hi, double* out_w, uint64_t cap, uint32_t* label,
                                           double* core, hs_density_info* out) {
  if (!out) return HS_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  if (n >= (1ull << 32) || !min_pts) return HS_ERR_INVALID;
  if (n_edges && (!ei || !ej || !dist)) return HS_ERR_INVALID;
  if (cap && (!out_lo || !out_hi || !out_w)) return HS_ERR_INVALID;
  for (uint64_t e = 0; e < n_edges; ++e)
    if (ei[e] >= n || ej[e] >= n || !(dist[e] >= 0.0)) return HS_ERR_INVALID;  // (a NaN fails the comparison)
  try {
    // (-0.0 + 0.0 = +0.0: every weight is >= +0, so that bit patterns order like the doubles, as on the device)
    std::vector<HostEdge> edges;
    edges.reserve(n_edges);
    for (uint64_t e = 0; e < n_edges; ++e)
      if (ei[e] != ej[e]) edges.push_back({dist[e] + 0.0, std::min(ei[e], ej[e]), std::max(ei[e], ej[e])});
    // by pair first: the occurrences of one unordered pair side by side, their distance bits compared
    std::sort(edges.begin(), edges.end(), [](const HostEdge& x, const HostEdge& y) {
      if (x.lo != y.lo) return x.lo < y.lo;
      if (x.hi != y.hi) return x.hi < y.hi;
      return x.d < y.d;
    });
    size_t kept = 0;
    for (size_t e = 0; e < edges.size(); ++e) {
      if (kept && edges[kept - 1].lo == edges[e].lo && edges[kept - 1].hi == edges[e].hi) {
        if (memcmp(&edges[kept - 1].d, &edges[e].d, 8) != 0) return HS_ERR_INVALID;
        continue;
      }
      edges[kept++] = edges[e];
    }
    edges.resize(kept);
    // the core distances: every vertex's neighbour distances gathered (a counting sort by vertex), the
    // (min_pts - 1)-th smallest selected
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> cd(n, min_pts == 1 ? 0.0 : inf);
    if (min_pts > 1) {
      std::vector<uint64_t> off(n + 1, 0);
      for (const HostEdge& e : edges) {
        ++off[e.lo + 1];
        ++off[e.hi + 1];
      }
      for (uint64_t i = 0; i < n; ++i) off[i + 1] += off[i];
      std::vector<double> nb(2 * edges.size());
      std::vector<uint64_t> at(off.begin(), off.end() - 1);
      for (const HostEdge& e : edges) {
        nb[at[e.lo]++] = e.d;
        nb[at[e.hi]++] = e.d;
      }
      const uint64_t need = min_pts - 1;
      for (uint64_t i = 0; i < n; ++i) {
        if (off[i + 1] - off[i] < need) continue;
        double* const b = nb.data() + off[i];
        std::nth_element(b, b + (need - 1), nb.data() + off[i + 1]);
        cd[i] = b[need - 1];
      }
    }
    uint64_t n_core = 0;
    for (uint64_t i = 0; i < n; ++i) n_core += cd[i] < inf;
    const uint64_t n_graph = 2 * (uint64_t)edges.size();
    size_t live = 0;
    for (size_t e = 0; e < edges.size(); ++e) {
      HostEdge x = edges[e];
      x.d = std::max(x.d, std::max(cd[x.lo], cd[x.hi]));
      if (x.d < inf) edges[live++] = x;
    }
    edges.resize(live);
    std::sort(edges.begin(), edges.end(), edge_less);
    HostForest forest(n);
    std::vector<HostEdge> tree;
    for (const HostEdge& e : edges)
      if (forest.unite(e.lo, e.hi)) tree.push_back(e);
    out->n_tree_edges = tree.size();
    out->n_core = n_core;
    out->n_clusters = n_core - tree.size();
    out->n_graph_edges = n_graph;
    if (tree.size() > cap) return HS_ERR_CAPACITY;
    for (size_t t = 0; t < tree.size(); ++t) {
      out_lo[t] = tree[t].lo;
      out_hi[t] = tree[t].hi;
      out_w[t] = tree[t].d;
    }
    if (label) {
      forest.labels(label);
      for (uint64_t i = 0; i < n; ++i)
        if (!(cd[i] < inf)) label[i] = HS_NOISE;
    }
    if (core)
      for (uint64_t i = 0; i < n; ++i) core[i] = cd[i];
  } catch (const std::bad_alloc&) {
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}

extern "C" hs_status hs_density_tree_cut(const uint32_t* lo, const uint32_t* hi, const double* w, uint64_t m,
                                         const double* core, uint64_t n, double r, uint32_t* label,
                                         uint64_t* n_clusters) {
  if (!n_clusters) return HS_ERR_INVALID;
  *n_clusters = 0;
  if (n >= (1ull << 32) || !(r == r)) return HS_ERR_INVALID;
  if (m && (!lo || !hi || !w)) return HS_ERR_INVALID;
  if (n && (!label || !core)) return HS_ERR_INVALID;
  for (uint64_t i = 0; i < n; ++i)
    if (!(core[i] >= 0.0)) return HS_ERR_INVALID;  // (a NaN fails the comparison; +inf is "no core distance")
  try {
    // the input must be a forest over 0 .. n-1 (as hs_msf_cut asks) whose weights are mutual-reachability weights:
    // none below the core distance of either end
    HostForest whole(n), cut(n);
    for (uint64_t t = 0; t < m; ++t) {
      if (lo[t] >= n || hi[t] >= n || lo[t] == hi[t] || !(w[t] == w[t])) return HS_ERR_INVALID;
      if (w[t] < core[lo[t]] || w[t] < core[hi[t]]) return HS_ERR_INVALID;
      if (!whole.unite(lo[t], hi[t])) return HS_ERR_INVALID;
      if (w[t] <= r) cut.unite(lo[t], hi[t]);
    }
    cut.labels(label);
    uint64_t clusters = 0;
    for (uint64_t i = 0; i < n; ++i) {
      if (core[i] <= r && core[i] < std::numeric_limits<double>::infinity())
        clusters += label[i] == i;
      else
        label[i] = HS_NOISE;
    }
    *n_clusters = clusters;
  } catch (const std::bad_alloc&) {
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}
