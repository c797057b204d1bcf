// hs_unionfind.h -- the device side of the lock-free union-find that hs_components.hip and hs_dbscan.hip share:
// the agent-scope loads and stores of `parent`, find with path halving, the hook by smaller id, and the per-wave
// count.  The invariant (parent[x] <= x), why no lane ever waits and why every read of `parent` is an agent-scope
// atomic load are written at the top of hs_components.hip.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace {

inline unsigned cc_blocks(uint32_t n) { return (n + 255u) / 256u; }

__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cc_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x, halving the path on the way (parent[x] <= x: every step descends)
__device__ __forceinline__ uint32_t cc_find(uint32_t* __restrict__ parent, uint32_t x) {
  for (;;) {
    const uint32_t p = cc_load(parent + x);
    if (p >= x) return x;  // (== x: a root; > x cannot be, and would end the walk rather than prolong it)
    const uint32_t g = cc_load(parent + p);
    if (g >= p) return p;
    cc_store(parent + x, g);
    x = g;
  }
}

// a and b into one tree: the larger root goes under the smaller; a lost CAS starts again from find
__device__ __forceinline__ void cc_unite(uint32_t* __restrict__ parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(parent + hi, hi, lo) == hi) return;
  }
}

// one 64-bit add per wave of the number of lanes with `flag` (all lanes of the wave must call)
__device__ __forceinline__ void cc_count(bool flag, unsigned long long* __restrict__ counter) {
  const unsigned long long m = __ballot(flag);
  if (m && (threadIdx.x & 63u) == (unsigned)(__ffsll((long long)m) - 1))
    atomicAdd(counter, (unsigned long long)__popcll(m));
}

}  // namespace
