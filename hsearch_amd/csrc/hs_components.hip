// hs_components.hip -- connected components of the near-neighbour graph, reduced on the device (hs_components,
// include/hsearch.h).
//
// A self-join returns every ordered pair (i, j) of indexed k-mers that share a bucket and lie within R; the
// components call keeps, per k-mer, the smallest id it is connected to.  The reduction runs batch by batch on the
// unordered exact hits a batch leaves in hit_key (key = q << 37 | table << 32 | id; i = self_first + q), into state
// that belongs to the handle and is sized by the index, never by the edges:
//   parent [n] u32   a union-find forest; the identity at the start of every call
// Invariant, at every instant: parent[x] <= x.  A word is written in two ways only:
//   hook      a ROOT hi goes under a smaller root lo by atomicCAS(&parent[hi], hi, lo): the word leaves the value
//             hi once, and only for something smaller
//   halving   a NON-root x is pointed at its grandparent, read just before: an ancestor of x, so <= parent[x] < x.
//             Two lanes may halve the same word in either order; both values are ancestors of x
// So a walk up the parents strictly descends and ends; no cycle can form; a non-root never becomes a root again;
// and the root of a tree is its smallest id (a hook keeps the smaller root).  When no lane is left, two ids are in
// one tree exactly if a path of united pairs joins them -- whatever the order in which batches, waves and lanes came.
//
// No lane ever waits for another: a lane whose CAS loses has seen proof that some other hook succeeded (parent[hi]
// changed), and starts again from find.  At most n - 1 hooks succeed per call, which bounds every retry loop.
//
// Every read of `parent` inside hs_cc_union_kernel is an agent-scope atomic load and every halving write an
// agent-scope atomic store of a value read that way.  The chip's eight L2s are not coherent with each other and a
// CU's L1 is never refreshed by another CU's stores: a plain load may go on answering "x is a root" from a stale
// line while the CAS -- which executes at the coherent point -- goes on failing, and that lane would never end.
// The atomic forms are served past L1 at agent scope and see what the CAS sees.
//
// One pair per lane, no wave-level pre-reduction of equal roots and both directions of a pair united (the second
// finds both ends under one root and writes nothing).  All stores are vector stores.
#include <vector>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_unionfind.h"  // cc_find, cc_unite, cc_count: shared with hs_dbscan.hip

namespace {

__global__ __launch_bounds__(256) void hs_cc_union_kernel(const uint64_t* __restrict__ key, uint32_t n_hits,
                                                          uint32_t self_first, uint32_t* __restrict__ parent,
                                                          uint32_t n, unsigned long long* __restrict__ n_pairs) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  uint32_t a = 0, b = 0;
  bool live = false;
  if (e < n_hits) {
    const uint64_t kk = key[e];
    a = self_first + (uint32_t)(kk >> 37);
    b = (uint32_t)kk;
    live = a != b && a < n && b < n;
  }
  cc_count(live, n_pairs);
  if (!live) return;
  cc_unite(parent, a, b);
}

__global__ __launch_bounds__(256) void hs_cc_iota_kernel(uint32_t* __restrict__ parent, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) parent[i] = i;
}

// behind the kernel boundary of the last union: label[i] = the root of i; the roots are counted
__global__ __launch_bounds__(256) void hs_cc_flatten_kernel(uint32_t* __restrict__ parent, uint32_t n,
                                                            uint32_t* __restrict__ label,
                                                            unsigned long long* __restrict__ n_roots) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t r = 0;
  if (i < n) {
    r = cc_find(parent, i);
    label[i] = r;
  }
  cc_count(i < n && r == i, n_roots);
}

}  // namespace

hipError_t hs_launch_cc_begin(uint32_t* d_parent, uint32_t n, uint64_t* d_counts, hipStream_t s) {
  hipError_t e = hipMemsetAsync(d_counts, 0, 16, s);
  if (e != hipSuccess || !n) return e;
  hs_cc_iota_kernel<<<cc_blocks(n), 256, 0, s>>>(d_parent, n);
  return hipGetLastError();
}

hipError_t hs_launch_cc_union(const uint64_t* d_key, uint32_t n_hits, uint32_t self_first, uint32_t* d_parent,
                              uint32_t n, uint64_t* d_counts, hipStream_t s) {
  if (!n_hits) return hipSuccess;
  hs_cc_union_kernel<<<cc_blocks(n_hits), 256, 0, s>>>(d_key, n_hits, self_first, d_parent, n,
                                                      reinterpret_cast<unsigned long long*>(d_counts));
  return hipGetLastError();
}

hipError_t hs_launch_cc_flatten(uint32_t* d_parent, uint32_t n, uint32_t* d_label, uint64_t* d_counts, hipStream_t s) {
  if (!n) return hipSuccess;
  hs_cc_flatten_kernel<<<cc_blocks(n), 256, 0, s>>>(d_parent, n, d_label,
                                                   reinterpret_cast<unsigned long long*>(d_counts) + 1);
  return hipGetLastError();
}

// ---- the merge of several label arrays on the host (no GPU, no handle) ---------------------------------
extern "C" hs_status hs_components_merge(const uint32_t* labels, uint64_t m, uint64_t n, uint32_t* out_label,
                                         uint64_t* n_components) {
  if (!n_components) return HS_ERR_INVALID;
  *n_components = 0;
  if (n >= (1ull << 32)) return HS_ERR_INVALID;
  if (n && ((m && !labels) || !out_label)) return HS_ERR_INVALID;
  // every input is a forest of depth one whose roots are the smallest ids of their trees
  for (uint64_t r = 0; r < m; ++r) {
    const uint32_t* const lab = labels + r * n;
    for (uint64_t i = 0; i < n; ++i)
      if (lab[i] > i || lab[lab[i]] != lab[i]) return HS_ERR_INVALID;
  }
  try {
    std::vector<uint32_t> parent(n);
    for (uint64_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    auto find = [&](uint32_t x) {
      while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
      }
      return x;
    };
    for (uint64_t r = 0; r < m; ++r) {
      const uint32_t* const lab = labels + r * n;
      for (uint64_t i = 0; i < n; ++i) {
        const uint32_t a = find((uint32_t)i), b = find(lab[i]);
        if (a != b) parent[a > b ? a : b] = a > b ? b : a;  // the smaller root stays: parent[x] <= x
      }
    }
    // ascending i: parent[i] < i is final already
    uint64_t roots = 0;
    for (uint64_t i = 0; i < n; ++i) {
      parent[i] = parent[parent[i]];
      roots += parent[i] == i;
    }
    for (uint64_t i = 0; i < n; ++i) out_label[i] = parent[i];
    *n_components = roots;
  } catch (const std::bad_alloc&) {
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}
