// hs_msf.hip -- the minimum spanning forest of the near-neighbour graph (the single-linkage tree up to R), found on
// the device by Boruvka rounds over the self-join's pairs (hs_msf, include/hsearch.h), and the same rule on the host
// for any edge list (hs_msf_edges, hs_msf_cut).
//
// The rule.  An edge is the unordered pair {lo < hi} with the distance the self-join reports for it (the same bits
// from both ends).  Edges are ordered by (dist, lo, hi): a strict total order, so the forest is unique.
//
// State, owned by the handle and sized by the index (56 bytes per indexed k-mer + the sort's scratch):
//   comp      [n] u32  the component of every k-mer at the START of the round: its smallest member's id
//   parent    [n] u32  the union-find forest of hs_components.hip (parent[x] <= x), the identity at the start of a call
//   best_d    [n] u64  indexed by a component's id: the smallest distance bits of an edge that leaves the component
//                      (a distance is >= +0, so its bits order like the doubles); MSF_EMPTY -- the bits of no
//                      distance -- marks a component no edge leaves
//   best_pair [n] u64  lo << 32 | hi of the smallest such pair AT that distance
//   out_pair, out_d [n] u64  the tree edges, in no order until the final sort
// One round is three steps, each behind a kernel boundary, so that a later step reads the earlier ones' words with
// plain loads:
//   1. min-d     every ordered pair (a, b) with comp[a] != comp[b] takes atomicMin(best_d + comp[a], bits); the
//                mirrored pair serves comp[b].  The pairs that still cross are counted: zero ends the call.
//   2. min-pair  the crossing pairs whose bits ARE best_d[comp[a]] take atomicMin(best_pair + comp[a], lo << 32 | hi).
//   3. select    one lane per component c with a non-empty slot: its edge e = {lo, hi} joins it to c' = the other
//                end's component.  The lane appends e to the output -- unless c' chose the very same edge and
//                c' < c: a mutual choice is emitted once -- and unites lo and hi in `parent`.  Then the flatten
//                kernel writes comp[i] = find(i) and empties the slots.
// Every step is idempotent: a repeated pair changes nothing.
//
// Why the chosen edges close no cycle.  Within a round every component chooses the SMALLEST edge that leaves it under
// one strict total order, seen identically from both ends.  Suppose the chosen edges, taken as distinct unordered
// pairs, held a cycle c_0 - c_1 - ... - c_{m-1} - c_0 of components (m >= 2; with m = 2 two DIFFERENT edges between
// the same two components).  Every edge of it was chosen by one of its two ends and a component chooses one edge, so
// m edges are chosen by m components: each component of the cycle chose exactly one of the cycle's edges, and the
// cycle can be walked so that c_t chose the edge to c_{t+1}.  The edge c_{t-1} chose also leaves c_t, so c_t's
// choice is not larger: e_0 >= e_1 >= ... >= e_{m-1} >= e_0, all equal under a strict order, so all the same edge:
// no cycle of distinct edges.  An edge that is the smallest leaving some component belongs to the (unique) minimum
// spanning forest (the cut property), so every emitted edge is a tree edge; when no pair crosses two components
// any more the components are those of the graph, and the n - n_components edges emitted are the whole forest.
// The components with an edge leaving them at least halve per round: rounds <= ceil(log2 n); the host loop stops
// with an error at HS_MSF_MAX_ROUNDS and never runs unbounded.
//
// The union in step 3 follows the rules of hs_components.hip: no lane waits for another, every read of `parent`
// inside the uniting kernel is the agent-scope atomic load of hs_unionfind.h, all stores are vector stores.  comp,
// best_d and best_pair are only READ in step 3 (written by earlier kernels), and `parent` is only read through
// cc_find / cc_unite.  The early-out loads in steps 1 and 2 (skip the atomic when the slot already holds something
// as small) are agent-scope atomic loads too; a stale answer could only be LARGER than the slot, which costs an
// atomic and never skips one.
//
// Where the pairs come from: a batch's exact hits as finalize_hits leaves them (key = q << 37 | table << 32 | id,
// val = the distance bits; both directions of a pair are there), or the list the first pass kept in HBM -- every
// pair once with lo < hi, as (lo << 32 | hi, bits) -- which serves both ends from one entry.  Steps 1 and 2 are one
// device function each on (a, b, bits) under the two loaders.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_msf_round.h"
#include "hs_unionfind.h"

namespace {

__global__ __launch_bounds__(256) void hs_msf_begin_kernel(uint32_t* __restrict__ comp, uint32_t* __restrict__ parent,
                                                           u64* __restrict__ best_d, u64* __restrict__ best_pair,
                                                           uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  comp[i] = i;
  parent[i] = i;
  best_d[i] = MSF_EMPTY;
  best_pair[i] = MSF_EMPTY;
}

// step 1 over a batch's hits; KEEP: the pairs with a < b are appended to `kept` as well (while there is room: the
// counter keeps running, so the caller sees an overflow)
template <bool KEEP>
__global__ __launch_bounds__(256) void hs_msf_min_d_hits_kernel(const uint64_t* __restrict__ key,
                                                                const uint64_t* __restrict__ val, uint32_t n_hits,
                                                                uint32_t self_first, const uint32_t* __restrict__ comp,
                                                                u64* __restrict__ best_d, uint32_t n,
                                                                u64* __restrict__ counts, ulonglong2* __restrict__ kept,
                                                                u64 kept_cap) {
  const MsfPair p = msf_load_hit(key, val, blockIdx.x * 256u + threadIdx.x, n_hits, self_first, n);
  cc_count(p.live, counts + MSF_N_PAIRS);
  const bool cross = p.live && msf_min_d(comp, best_d, p.a, p.b, p.d, false);
  cc_count(cross, counts + MSF_N_CROSS);
  if (KEEP) {
    const bool mine = p.live && p.a < p.b;
    const u64 pos = msf_append_pos(mine, counts + MSF_N_KEPT);
    if (mine && pos < kept_cap) kept[pos] = make_ulonglong2((u64)p.a << 32 | p.b, p.d);
  }
}

__global__ __launch_bounds__(256) void hs_msf_min_pair_hits_kernel(const uint64_t* __restrict__ key,
                                                                   const uint64_t* __restrict__ val, uint32_t n_hits,
                                                                   uint32_t self_first,
                                                                   const uint32_t* __restrict__ comp,
                                                                   const u64* __restrict__ best_d,
                                                                   u64* __restrict__ best_pair, uint32_t n) {
  const MsfPair p = msf_load_hit(key, val, blockIdx.x * 256u + threadIdx.x, n_hits, self_first, n);
  if (p.live) msf_min_pair(comp, best_d, best_pair, p.a, p.b, p.d, false);
}

// the same two steps over the kept list: one entry serves both ends (and counts as two ordered pairs)
__global__ __launch_bounds__(256) void hs_msf_min_d_kept_kernel(const ulonglong2* __restrict__ kept, u64 n_kept,
                                                                const uint32_t* __restrict__ comp,
                                                                u64* __restrict__ best_d, uint32_t n,
                                                                u64* __restrict__ counts) {
  const MsfPair p = msf_load_kept(kept, (u64)blockIdx.x * 256u + threadIdx.x, n_kept, n);
  const bool cross = p.live && msf_min_d(comp, best_d, p.a, p.b, p.d, true);
  cc_count(cross, counts + MSF_N_CROSS);
}

__global__ __launch_bounds__(256) void hs_msf_min_pair_kept_kernel(const ulonglong2* __restrict__ kept, u64 n_kept,
                                                                   const uint32_t* __restrict__ comp,
                                                                   const u64* __restrict__ best_d,
                                                                   u64* __restrict__ best_pair, uint32_t n) {
  const MsfPair p = msf_load_kept(kept, (u64)blockIdx.x * 256u + threadIdx.x, n_kept, n);
  if (p.live) msf_min_pair(comp, best_d, best_pair, p.a, p.b, p.d, true);
}

// step 3: comp, best_d and best_pair are final (plain loads); `parent` is touched through cc_unite alone
__global__ __launch_bounds__(256) void hs_msf_select_kernel(const uint32_t* __restrict__ comp,
                                                            uint32_t* __restrict__ parent,
                                                            const u64* __restrict__ best_d,
                                                            const u64* __restrict__ best_pair, uint32_t n,
                                                            u64* __restrict__ out_pair, u64* __restrict__ out_d,
                                                            u64* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool chose = false, emit = false;
  uint32_t lo = 0, hi = 0;
  u64 p = MSF_EMPTY, d = MSF_EMPTY;
  if (i < n && comp[i] == i) {
    d = best_d[i];
    p = best_pair[i];
    lo = (uint32_t)(p >> 32);
    hi = (uint32_t)p;
    chose = d != MSF_EMPTY && lo < hi && hi < n;
  }
  if (chose) {
    const uint32_t cl = comp[lo], other = cl == i ? comp[hi] : cl;
    emit = !(other < i && best_pair[other] == p);
  }
  const u64 pos = msf_append_pos(emit, counts + MSF_N_OUT);
  if (emit && pos < n) {
    out_pair[pos] = p;
    out_d[pos] = d;
  }
  if (chose) cc_unite(parent, lo, hi);
}

// behind the kernel boundary of the unions: the components of the next round, the slots emptied
__global__ __launch_bounds__(256) void hs_msf_flatten_kernel(uint32_t* __restrict__ comp, uint32_t* __restrict__ parent,
                                                             u64* __restrict__ best_d, u64* __restrict__ best_pair,
                                                             uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  comp[i] = cc_find(parent, i);
  best_d[i] = MSF_EMPTY;
  best_pair[i] = MSF_EMPTY;
}

__global__ __launch_bounds__(256) void hs_msf_finish_kernel(const uint32_t* __restrict__ comp, uint32_t n,
                                                            uint32_t* __restrict__ label, u64* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t c = 0xffffffffu;
  if (i < n) {
    c = comp[i];
    if (label) label[i] = c;
  }
  cc_count(i < n && c == i, counts + MSF_N_ROOTS);
}

__global__ __launch_bounds__(256) void hs_msf_unpack_kernel(const u64* __restrict__ pair, const u64* __restrict__ d,
                                                            uint32_t m, uint32_t* __restrict__ lo,
                                                            uint32_t* __restrict__ hi, double* __restrict__ dist) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  const u64 p = pair[i];
  lo[i] = (uint32_t)(p >> 32);
  hi[i] = (uint32_t)p;
  dist[i] = __longlong_as_double((long long)d[i]);
}

}  // namespace

hipError_t hs_launch_msf_begin(uint32_t* d_comp, uint32_t* d_parent, uint64_t* d_best_d, uint64_t* d_best_pair,
                               uint32_t n, uint64_t* d_counts, hipStream_t s) {
  hipError_t e = hipMemsetAsync(d_counts, 0, 64, s);
  if (e != hipSuccess || !n) return e;
  hs_msf_begin_kernel<<<cc_blocks(n), 256, 0, s>>>(d_comp, d_parent, reinterpret_cast<u64*>(d_best_d),
                                                  reinterpret_cast<u64*>(d_best_pair), n);
  return hipGetLastError();
}

hipError_t hs_launch_msf_min_d_hits(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits, uint32_t self_first,
                                    const uint32_t* d_comp, uint64_t* d_best_d, uint32_t n, uint64_t* d_counts,
                                    void* d_kept, uint64_t kept_cap, hipStream_t s) {
  if (!n_hits) return hipSuccess;
  u64* const bd = reinterpret_cast<u64*>(d_best_d);
  u64* const cn = reinterpret_cast<u64*>(d_counts);
  if (d_kept)
    hs_msf_min_d_hits_kernel<true><<<cc_blocks(n_hits), 256, 0, s>>>(d_key, d_val, n_hits, self_first, d_comp, bd, n, cn,
                                                                    reinterpret_cast<ulonglong2*>(d_kept), kept_cap);
  else
    hs_msf_min_d_hits_kernel<false><<<cc_blocks(n_hits), 256, 0, s>>>(d_key, d_val, n_hits, self_first, d_comp, bd, n,
                                                                     cn, nullptr, 0);
  return hipGetLastError();
}

hipError_t hs_launch_msf_min_pair_hits(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits,
                                       uint32_t self_first, const uint32_t* d_comp, const uint64_t* d_best_d,
                                       uint64_t* d_best_pair, uint32_t n, hipStream_t s) {
  if (!n_hits) return hipSuccess;
  hs_msf_min_pair_hits_kernel<<<cc_blocks(n_hits), 256, 0, s>>>(d_key, d_val, n_hits, self_first, d_comp,
                                                               reinterpret_cast<const u64*>(d_best_d),
                                                               reinterpret_cast<u64*>(d_best_pair), n);
  return hipGetLastError();
}

hipError_t hs_launch_msf_min_d_kept(const void* d_kept, uint64_t n_kept, const uint32_t* d_comp, uint64_t* d_best_d,
                                    uint32_t n, uint64_t* d_counts, hipStream_t s) {
  if (!n_kept) return hipSuccess;
  hs_msf_min_d_kept_kernel<<<msf_blocks64(n_kept), 256, 0, s>>>(reinterpret_cast<const ulonglong2*>(d_kept), n_kept,
                                                               d_comp, reinterpret_cast<u64*>(d_best_d), n,
                                                               reinterpret_cast<u64*>(d_counts));
  return hipGetLastError();
}

hipError_t hs_launch_msf_min_pair_kept(const void* d_kept, uint64_t n_kept, const uint32_t* d_comp,
                                       const uint64_t* d_best_d, uint64_t* d_best_pair, uint32_t n, hipStream_t s) {
  if (!n_kept) return hipSuccess;
  hs_msf_min_pair_kept_kernel<<<msf_blocks64(n_kept), 256, 0, s>>>(reinterpret_cast<const ulonglong2*>(d_kept), n_kept,
                                                                  d_comp, reinterpret_cast<const u64*>(d_best_d),
                                                                  reinterpret_cast<u64*>(d_best_pair), n);
  return hipGetLastError();
}

hipError_t hs_launch_msf_select(uint32_t* d_comp, uint32_t* d_parent, uint64_t* d_best_d, uint64_t* d_best_pair,
                                uint32_t n, uint64_t* d_out_pair, uint64_t* d_out_d, uint64_t* d_counts,
                                hipStream_t s) {
  if (!n) return hipSuccess;
  u64* const bd = reinterpret_cast<u64*>(d_best_d);
  u64* const bp = reinterpret_cast<u64*>(d_best_pair);
  hs_msf_select_kernel<<<cc_blocks(n), 256, 0, s>>>(d_comp, d_parent, bd, bp, n, reinterpret_cast<u64*>(d_out_pair),
                                                   reinterpret_cast<u64*>(d_out_d), reinterpret_cast<u64*>(d_counts));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hs_msf_flatten_kernel<<<cc_blocks(n), 256, 0, s>>>(d_comp, d_parent, bd, bp, n);
  return hipGetLastError();
}

hipError_t hs_launch_msf_finish(const uint32_t* d_comp, uint32_t n, uint32_t* d_label, uint64_t* d_counts,
                                hipStream_t s) {
  if (!n) return hipSuccess;
  hs_msf_finish_kernel<<<cc_blocks(n), 256, 0, s>>>(d_comp, n, d_label, reinterpret_cast<u64*>(d_counts));
  return hipGetLastError();
}

hipError_t hs_launch_msf_unpack(const uint64_t* d_pair, const uint64_t* d_d, uint32_t m, uint32_t* d_lo, uint32_t* d_hi,
                                double* d_dist, hipStream_t s) {
  if (!m) return hipSuccess;
  hs_msf_unpack_kernel<<<cc_blocks(m), 256, 0, s>>>(reinterpret_cast<const u64*>(d_pair),
                                                   reinterpret_cast<const u64*>(d_d), m, d_lo, d_hi, d_dist);
  return hipGetLastError();
}

// ---- the same rule on the host (no GPU, no handle): HostForest and HostEdge are in hs_msf_round.h ----

extern "C" hs_status hs_msf_edges(const uint32_t* ei, const uint32_t* ej, const double* dist, uint64_t n_edges,
                                  uint64_t n, uint32_t* out_lo, uint32_t* out_hi, double* out_dist, uint64_t cap,
                                  uint32_t* label, hs_msf_info* out) {
  if (!out) return HS_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  if (n >= (1ull << 32)) return HS_ERR_INVALID;
  if (n_edges && (!ei || !ej || !dist)) return HS_ERR_INVALID;
  if (cap && (!out_lo || !out_hi || !out_dist)) return HS_ERR_INVALID;
  for (uint64_t e = 0; e < n_edges; ++e)
    if (ei[e] >= n || ej[e] >= n || !(dist[e] >= 0.0)) return HS_ERR_INVALID;  // (a NaN fails the comparison)
  try {
    std::vector<HostEdge> edges;
    edges.reserve(n_edges);
    for (uint64_t e = 0; e < n_edges; ++e)
      if (ei[e] != ej[e]) edges.push_back({dist[e], std::min(ei[e], ej[e]), std::max(ei[e], ej[e])});
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
    std::sort(edges.begin(), edges.end(), edge_less);
    HostForest forest(n);
    std::vector<HostEdge> tree;
    for (const HostEdge& e : edges)
      if (forest.unite(e.lo, e.hi)) tree.push_back(e);
    out->n_tree_edges = tree.size();
    out->n_components = n - tree.size();
    out->n_graph_edges = 2 * (uint64_t)edges.size();
    out->rounds = 0;
    out->resident = 0;
    if (tree.size() > cap) return HS_ERR_CAPACITY;
    for (size_t t = 0; t < tree.size(); ++t) {
      out_lo[t] = tree[t].lo;
      out_hi[t] = tree[t].hi;
      out_dist[t] = tree[t].d;
    }
    if (label) forest.labels(label);
  } catch (const std::bad_alloc&) {
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}

extern "C" hs_status hs_msf_cut(const uint32_t* lo, const uint32_t* hi, const double* dist, uint64_t m, uint64_t n,
                                double r, uint32_t* label, uint64_t* n_components) {
  if (!n_components) return HS_ERR_INVALID;
  *n_components = 0;
  if (n >= (1ull << 32) || !(r == r)) return HS_ERR_INVALID;
  if (m && (!lo || !hi || !dist)) return HS_ERR_INVALID;
  if (n && !label) return HS_ERR_INVALID;
  try {
    // the input must be a forest over 0 .. n-1: ids in range, no self pair, no NaN, and no edge that closes a cycle
    // (which also rules out a repeated pair)
    HostForest whole(n), cut(n);
    for (uint64_t t = 0; t < m; ++t) {
      if (lo[t] >= n || hi[t] >= n || lo[t] == hi[t] || !(dist[t] == dist[t])) return HS_ERR_INVALID;
      if (!whole.unite(lo[t], hi[t])) return HS_ERR_INVALID;
      if (dist[t] <= r) cut.unite(lo[t], hi[t]);
    }
    *n_components = cut.labels(label);
  } catch (const std::bad_alloc&) {
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}
