// hs_msf_round.h -- the device side of a Boruvka round that hs_msf.hip and hs_density.hip share: the two sources of
// pairs (a batch's hits, the kept list), steps 1 and 2 on (a, b, weight bits), and the per-wave append.  The state, the
// round and why the chosen edges close no cycle are written at the head of hs_msf.hip; the argument only needs the
// weight to be one strict total order seen identically from both ends of a pair.
#pragma once

#include <stdint.h>

#include <numeric>
#include <vector>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_unionfind.h"

namespace {

#define MSF_EMPTY HS_ANNOT_EMPTY

typedef unsigned long long u64;

// counts: eight 64-bit words; hs_msf uses the first five, hs_density_tree all of them
enum { MSF_N_PAIRS = 0, MSF_N_CROSS = 1, MSF_N_KEPT = 2, MSF_N_OUT = 3, MSF_N_ROOTS = 4, MSF_N_CORE = 5,
       MSF_N_OPEN = 6 };

struct MsfPair {
  uint32_t a, b;
  u64 d;
  bool live;
};

// pair e of a batch's hits; the pair of an id with itself is not live
__device__ __forceinline__ MsfPair msf_load_hit(const uint64_t* __restrict__ key, const uint64_t* __restrict__ val,
                                                uint32_t e, uint32_t n_hits, uint32_t self_first, uint32_t n) {
  MsfPair p = {0u, 0u, 0ull, false};
  if (e < n_hits) {
    const uint64_t kk = key[e];
    p.a = self_first + (uint32_t)(kk >> 37);
    p.b = (uint32_t)kk;
    p.d = val[e];
    p.live = p.a != p.b && p.a < n && p.b < n;
  }
  return p;
}
// entry e of the kept list: a = lo, b = hi
__device__ __forceinline__ MsfPair msf_load_kept(const ulonglong2* __restrict__ kept, uint64_t e, uint64_t n_kept,
                                                 uint32_t n) {
  MsfPair p = {0u, 0u, 0ull, false};
  if (e < n_kept) {
    const ulonglong2 w = kept[e];
    p.a = (uint32_t)(w.x >> 32);
    p.b = (uint32_t)w.x;
    p.d = w.y;
    p.live = p.a != p.b && p.a < n && p.b < n;
  }
  return p;
}

__device__ __forceinline__ u64 msf_peek(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void msf_lower(u64* slot, u64 v) {
  if (v < msf_peek(slot)) atomicMin(slot, v);
}

// step 1 for the pair (a, b): serves comp[a] (both: and comp[b]); true if the pair crosses two components
__device__ __forceinline__ bool msf_min_d(const uint32_t* __restrict__ comp, u64* __restrict__ best_d, uint32_t a,
                                          uint32_t b, u64 d, bool both) {
  const uint32_t ca = comp[a], cb = comp[b];
  if (ca == cb) return false;
  msf_lower(best_d + ca, d);
  if (both) msf_lower(best_d + cb, d);
  return true;
}
// step 2 (best_d is final: step 1 ended at a kernel boundary)
__device__ __forceinline__ void msf_min_pair(const uint32_t* __restrict__ comp, const u64* __restrict__ best_d,
                                             u64* __restrict__ best_pair, uint32_t a, uint32_t b, u64 d, bool both) {
  const uint32_t ca = comp[a], cb = comp[b];
  if (ca == cb) return;
  const u64 p = a < b ? (u64)a << 32 | b : (u64)b << 32 | a;
  if (best_d[ca] == d) msf_lower(best_pair + ca, p);
  if (both && best_d[cb] == d) msf_lower(best_pair + cb, p);
}

// the position of every flagged lane in a list whose length is *counter: one 64-bit add per wave (all lanes of the
// wave must call)
__device__ __forceinline__ u64 msf_append_pos(bool flag, u64* __restrict__ counter) {
  const u64 m = __ballot(flag);
  if (!m) return 0;
  const unsigned lane = threadIdx.x & 63u;
  const int leader = __ffsll((long long)m) - 1;
  u64 base = 0;
  if ((int)lane == leader) base = atomicAdd(counter, (u64)__popcll(m));
  base = __shfl(base, leader);
  return base + (u64)__popcll(m & ((1ull << lane) - 1ull));
}

inline unsigned msf_blocks64(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

// ---- the host side of the same rule (hs_msf_edges, hs_msf_cut, hs_density_tree_edges, hs_density_tree_cut) ----
struct HostForest {
  std::vector<uint32_t> parent;
  explicit HostForest(uint64_t n) : parent(n) { std::iota(parent.begin(), parent.end(), 0u); }
  uint32_t find(uint32_t x) {
    while (parent[x] != x) {
      parent[x] = parent[parent[x]];
      x = parent[x];
    }
    return x;
  }
  // false: already in one tree.  The smaller root stays: parent[x] <= x
  bool unite(uint32_t a, uint32_t b) {
    a = find(a);
    b = find(b);
    if (a == b) return false;
    parent[a > b ? a : b] = a > b ? b : a;
    return true;
  }
  // the labels (ascending i: parent[i] < i is final already) into out; returns the number of roots
  uint64_t labels(uint32_t* out) {
    uint64_t roots = 0;
    for (size_t i = 0; i < parent.size(); ++i) {
      parent[i] = parent[parent[i]];
      roots += parent[i] == i;
      if (out) out[i] = parent[i];
    }
    return roots;
  }
};

struct HostEdge {
  double d;
  uint32_t lo, hi;
};
inline bool edge_less(const HostEdge& x, const HostEdge& y) {
  if (x.d != y.d) return x.d < y.d;
  if (x.lo != y.lo) return x.lo < y.lo;
  return x.hi < y.hi;
}

}  // namespace
