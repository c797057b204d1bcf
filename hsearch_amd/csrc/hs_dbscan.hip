// hs_dbscan.hip -- density clusters (DBSCAN) of the near-neighbour graph, reduced on the device (hs_degrees, hs_dbscan,
// include/hsearch.h), and the same rule on the host for any edge list (hs_dbscan_edges).
//
// The graph is the self-join's: every batch of a self-join leaves its exact, de-duplicated ORDERED pairs in hit_key
// (key = q << 37 | table << 32 | id; a = self_first + q, b = id), so every unordered pair {a, b} arrives twice, as
// (a, b) and as (b, a).  Two self-joins with the same arguments reduce those pairs into state that belongs to the
// handle and is sized by the index, never by the edges -- 12 bytes per indexed k-mer:
//   deg    [n] u32   pass 1: deg[a] += 1 per live pair (a, b).  0 at the start of every call
//   parent [n] u32   pass 2: the union-find forest of hs_components.hip (hs_unionfind.h) over the CORE vertices
//                    (deg[i] + 1 >= min_pts); the identity at the start of every call
//   anchor [n] u32   pass 2: the smallest core neighbour of a non-core vertex; HS_NOISE at the start of every call
// Pass 1 ends at a kernel boundary (and a stream synchronisation: run_query returns the hit count), so pass 2 reads
// deg with plain loads.  finish, one lane per vertex, behind the kernel boundary of the last unite:
//   core              label = find(i); the roots among the cores are the clusters
//   non-core, anchor  label = find(anchor): border
//   otherwise         HS_NOISE
// The root of a tree is its smallest id (the hook keeps the smaller root) and only cores are ever united, so a label
// is the smallest core id of its cluster.
//
// THE DEGREE COUNT IS NOT IDEMPOTENT, unlike the union and the min: a pair counted twice is a wrong degree.  It
// relies on two rules of the caller (run_query, hs_capi.hip), and hs_db_degree_kernel is launched from that one
// place only:
//   * only a batch that came through query_batch whole hands its pairs on -- a batch cut in halves by
//     HS_SPLIT_BATCH has handed on nothing, and its halves bring each pair once;
//   * hit_key holds each ordered pair once (the first-seen de-duplication across tables has run): what the tests
//     pin as n_edges == len(self_join).
//
// One pair per lane and one atomic per live lane; all stores are vector stores.
#include <algorithm>
#include <vector>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_unionfind.h"

namespace {

__global__ __launch_bounds__(256) void hs_db_init_kernel(uint32_t* __restrict__ deg, uint32_t* __restrict__ parent,
                                                         uint32_t* __restrict__ anchor, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) {
    deg[i] = 0;
    parent[i] = i;
    anchor[i] = HS_NOISE;
  }
}

// pass 1 (not idempotent: see the head of the file)
__global__ __launch_bounds__(256) void hs_db_degree_kernel(const uint64_t* __restrict__ key, uint32_t n_hits,
                                                           uint32_t self_first, uint32_t* __restrict__ deg,
                                                           uint32_t n, unsigned long long* __restrict__ n_pairs) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  uint32_t a = 0;
  bool live = false;
  if (e < n_hits) {
    const uint64_t kk = key[e];
    a = self_first + (uint32_t)(kk >> 37);
    const uint32_t b = (uint32_t)kk;
    live = a != b && a < n && b < n;
  }
  cc_count(live, n_pairs);
  if (live) atomicAdd(deg + a, 1u);
}

// pass 2: two cores are united; a core b next to a non-core a is a's anchor if it is the smallest such.  (The
// mirrored pair (b, a) covers the non-core b next to a core a.)
__global__ __launch_bounds__(256) void hs_db_unite_kernel(const uint64_t* __restrict__ key, uint32_t n_hits,
                                                          uint32_t self_first, const uint32_t* __restrict__ deg,
                                                          uint32_t need, uint32_t* __restrict__ parent,
                                                          uint32_t* __restrict__ anchor, uint32_t n) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n_hits) return;
  const uint64_t kk = key[e];
  const uint32_t a = self_first + (uint32_t)(kk >> 37), b = (uint32_t)kk;
  if (a == b || a >= n || b >= n) return;
  if (deg[b] < need) return;  // need = min_pts - 1 neighbours make a core
  if (deg[a] >= need)
    cc_unite(parent, a, b);
  else
    atomicMin(anchor + a, b);
}

// counts: {ordered pairs, clusters, core, border, noise}
__global__ __launch_bounds__(256) void hs_db_finish_kernel(uint32_t* __restrict__ parent,
                                                           const uint32_t* __restrict__ deg,
                                                           const uint32_t* __restrict__ anchor, uint32_t need,
                                                           uint32_t n, uint32_t* __restrict__ label,
                                                           unsigned long long* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool core = false, border = false;
  uint32_t r = HS_NOISE;
  if (i < n) {
    core = deg[i] >= need;
    const uint32_t from = core ? i : anchor[i];
    border = !core && from != HS_NOISE;
    if (from != HS_NOISE) r = cc_find(parent, from);
    label[i] = r;
  }
  cc_count(core && r == i, counts + 1);
  cc_count(core, counts + 2);
  cc_count(border, counts + 3);
  cc_count(i < n && !core && !border, counts + 4);
}

}  // namespace

hipError_t hs_launch_db_begin(uint32_t* d_deg, uint32_t* d_parent, uint32_t* d_anchor, uint32_t n, uint64_t* d_counts,
                              hipStream_t s) {
  hipError_t e = hipMemsetAsync(d_counts, 0, 40, s);
  if (e != hipSuccess || !n) return e;
  hs_db_init_kernel<<<cc_blocks(n), 256, 0, s>>>(d_deg, d_parent, d_anchor, n);
  return hipGetLastError();
}

hipError_t hs_launch_db_degree(const uint64_t* d_key, uint32_t n_hits, uint32_t self_first, uint32_t* d_deg, uint32_t n,
                               uint64_t* d_counts, hipStream_t s) {
  if (!n_hits) return hipSuccess;
  hs_db_degree_kernel<<<cc_blocks(n_hits), 256, 0, s>>>(d_key, n_hits, self_first, d_deg, n,
                                                       reinterpret_cast<unsigned long long*>(d_counts));
  return hipGetLastError();
}

hipError_t hs_launch_db_unite(const uint64_t* d_key, uint32_t n_hits, uint32_t self_first, const uint32_t* d_deg,
                              uint32_t min_pts, uint32_t* d_parent, uint32_t* d_anchor, uint32_t n, hipStream_t s) {
  if (!n_hits) return hipSuccess;
  hs_db_unite_kernel<<<cc_blocks(n_hits), 256, 0, s>>>(d_key, n_hits, self_first, d_deg, min_pts - 1, d_parent,
                                                      d_anchor, n);
  return hipGetLastError();
}

hipError_t hs_launch_db_finish(uint32_t* d_parent, const uint32_t* d_deg, const uint32_t* d_anchor, uint32_t min_pts,
                               uint32_t n, uint32_t* d_label, uint64_t* d_counts, hipStream_t s) {
  if (!n) return hipSuccess;
  hs_db_finish_kernel<<<cc_blocks(n), 256, 0, s>>>(d_parent, d_deg, d_anchor, min_pts - 1, n, d_label,
                                                  reinterpret_cast<unsigned long long*>(d_counts));
  return hipGetLastError();
}

// ---- the same rule on the host for any list of pairs (no GPU, no handle) --------------------------------
extern "C" hs_status hs_dbscan_edges(const uint32_t* ei, const uint32_t* ej, uint64_t n_edges, uint64_t n,
                                     uint32_t min_pts, uint32_t* label, uint32_t* degree, hs_dbscan_counts* out) {
  if (!out) return HS_ERR_INVALID;
  out->n_clusters = out->n_core = out->n_border = out->n_noise = out->n_edges = 0;
  if (!min_pts || n >= (1ull << 32) || (n && !label) || (n_edges && (!ei || !ej))) return HS_ERR_INVALID;
  for (uint64_t e = 0; e < n_edges; ++e)
    if (ei[e] >= n || ej[e] >= n) return HS_ERR_INVALID;
  try {
    // the graph is the set of unordered pairs: (smaller << 32 | larger), self pairs dropped, each once
    std::vector<uint64_t> pairs;
    pairs.reserve(n_edges);
    for (uint64_t e = 0; e < n_edges; ++e)
      if (ei[e] != ej[e]) pairs.push_back((uint64_t)std::min(ei[e], ej[e]) << 32 | std::max(ei[e], ej[e]));
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    std::vector<uint32_t> deg(n, 0), parent(n), anchor(n, HS_NOISE);
    for (const uint64_t p : pairs) {
      ++deg[p >> 32];
      ++deg[(uint32_t)p];
    }
    for (uint64_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    auto find = [&](uint32_t x) {
      while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
      }
      return x;
    };
    const uint32_t need = min_pts - 1;
    for (const uint64_t p : pairs) {
      const uint32_t lo = (uint32_t)(p >> 32), hi = (uint32_t)p;
      const bool clo = deg[lo] >= need, chi = deg[hi] >= need;
      if (clo && chi) {
        const uint32_t a = find(lo), b = find(hi);
        if (a != b) parent[a > b ? a : b] = a > b ? b : a;  // the smaller root stays: parent[x] <= x
      } else if (chi) {
        anchor[lo] = std::min(anchor[lo], hi);
      } else if (clo) {
        anchor[hi] = std::min(anchor[hi], lo);
      }
    }
    for (uint64_t i = 0; i < n; ++i) {
      const bool core = deg[i] >= need;
      const uint32_t from = core ? (uint32_t)i : anchor[i];
      label[i] = from == HS_NOISE ? HS_NOISE : find(from);
      out->n_clusters += core && label[i] == i;
      out->n_core += core;
      out->n_border += !core && from != HS_NOISE;
      out->n_noise += from == HS_NOISE;
      if (degree) degree[i] = deg[i];
    }
    out->n_edges = 2 * (uint64_t)pairs.size();
  } catch (const std::bad_alloc&) {
    out->n_clusters = out->n_core = out->n_border = out->n_noise = out->n_edges = 0;
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}
