// hs_annotate.hip -- the nearest centre of every DB k-mer, reduced on the device (hs_annotate, include/hsearch.h).
//
// A search returns one tuple per (centre, k-mer) pair within the radius; an annotation keeps, per k-mer, the
// tuple that is smallest under (dist, table, q).  The reduction runs batch by batch on the unordered exact hits
// a batch leaves in hit_key / hit_val (key = q << 37 | table << 32 | id, val = the fp64 bits of the distance),
// or on the four arrays of a multi-probe chunk's merged list, into state that belongs to the handle and is sized
// by the index, never by the hits:
//   best_dist [n] u64  the fp64 bits of the smallest distance seen (a distance is >= +0, so its bits order like
//                      the doubles); HS_ANNOT_EMPTY -- no double a square root returns -- marks an untouched slot
//   best_tq   [n] u32  table << 27 | q of the smallest (table, q) among the hits AT that distance
//   touched   [<= n]   the ids whose slot left the empty state in this call, in no order
// The 96-bit key does not fit one atomic, so a batch takes two kernels over its hits:
//   1. hs_annot_min_kernel: atomicMin of the distance bits.  A hit that LOWERS its slot stores the empty value into
//      best_tq[id]: whatever (table, q) stood there belonged to a larger distance.  Several hits may lower one slot
//      in turn; they all store the same word, and no hit reads best_tq in this kernel.  The hit that finds the slot
//      empty -- exactly one per slot and call, the atomic's return value says which -- appends the id to `touched`.
//   2. hs_annot_tq_kernel (after the kernel boundary: every slot's distance is final for the batch): the hits whose
//      distance IS the slot's take atomicMin of table << 27 | q.  A slot this batch did not lower keeps the word of
//      the earlier batches, so a tie across batches is decided like a tie inside one.
// Both steps are idempotent: reducing a hit twice changes nothing.
// At the end of the call the touched ids are sorted (a radix sort of that many 32-bit keys: nothing here ever
// walks the n slots) and hs_annot_gather_kernel writes the rows in ascending id and hands every slot it read
// back EMPTY, which is what the next call starts from.  (A call that ends early leaves its slots dirty; the C-ABI
// layer remembers that and clears all n slots once before the next annotation.)
//
// One hit per lane, no wave-level pre-reduction of equal ids: a wave's 64 hits come from the survivor list in
// bucket order and name 64 different ids except where a k-mer is hit by several centres of one segment.  All
// stores are vector stores.
#include <algorithm>
#include <vector>

#include <hip/hip_runtime.h>

#include "hs_internal.h"

namespace {

inline unsigned annot_blocks(uint32_t n) { return (n + 255u) / 256u; }

struct AnnotHit {
  uint32_t id, tq;
  uint64_t d;
};

// hit i of a batch (key / val) or of a merged list (q, id, table, dist)
__device__ __forceinline__ AnnotHit annot_load(const uint64_t* __restrict__ key, const uint64_t* __restrict__ val,
                                               const uint32_t* __restrict__ q, const uint32_t* __restrict__ id,
                                               const uint32_t* __restrict__ table, const double* __restrict__ dist,
                                               uint32_t i) {
  AnnotHit h;
  if (key) {
    const uint64_t kk = key[i];
    h.id = (uint32_t)kk;
    h.tq = ((uint32_t)(kk >> 32) & 31u) << 27 | (uint32_t)(kk >> 37);
    h.d = val[i];
  } else {
    h.id = id[i];
    h.tq = table[i] << 27 | q[i];
    h.d = (uint64_t)__double_as_longlong(dist[i]);
  }
  return h;
}

__global__ __launch_bounds__(256) void hs_annot_min_kernel(const uint64_t* __restrict__ key,
                                                           const uint64_t* __restrict__ val,
                                                           const uint32_t* __restrict__ q,
                                                           const uint32_t* __restrict__ id,
                                                           const uint32_t* __restrict__ table,
                                                           const double* __restrict__ dist, uint32_t n_hits,
                                                           unsigned long long* __restrict__ best_dist,
                                                           uint32_t* __restrict__ best_tq, uint32_t n_slots,
                                                           uint32_t* __restrict__ touched,
                                                           uint32_t* __restrict__ n_touched) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_hits) return;
  const AnnotHit h = annot_load(key, val, q, id, table, dist, i);
  if (h.id >= n_slots) return;
  const unsigned long long old = atomicMin(best_dist + h.id, (unsigned long long)h.d);
  if (h.d < old) {
    best_tq[h.id] = 0xffffffffu;
    if (old == HS_ANNOT_EMPTY) {
      const uint32_t t = atomicAdd(n_touched, 1u);
      if (t < n_slots) touched[t] = h.id;
    }
  }
}

__global__ __launch_bounds__(256) void hs_annot_tq_kernel(const uint64_t* __restrict__ key,
                                                          const uint64_t* __restrict__ val,
                                                          const uint32_t* __restrict__ q,
                                                          const uint32_t* __restrict__ id,
                                                          const uint32_t* __restrict__ table,
                                                          const double* __restrict__ dist, uint32_t n_hits,
                                                          const unsigned long long* __restrict__ best_dist,
                                                          uint32_t* __restrict__ best_tq, uint32_t n_slots) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_hits) return;
  const AnnotHit h = annot_load(key, val, q, id, table, dist, i);
  if (h.id >= n_slots) return;
  if (best_dist[h.id] == h.d) atomicMin(best_tq + h.id, h.tq);
}

// row i = the slot of the i-th smallest touched id; the slot goes back to the empty state.  out_id == null: the
// rows are not wanted (the caller's arrays are too short), the slots are emptied all the same.
__global__ __launch_bounds__(256) void hs_annot_gather_kernel(const uint32_t* __restrict__ sorted_id, uint32_t cnt,
                                                              unsigned long long* __restrict__ best_dist,
                                                              const uint32_t* __restrict__ best_tq, uint32_t n_slots,
                                                              uint32_t* __restrict__ out_id,
                                                              uint32_t* __restrict__ out_q,
                                                              uint32_t* __restrict__ out_table,
                                                              double* __restrict__ out_dist) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= cnt) return;
  const uint32_t id = sorted_id[i];
  if (id >= n_slots) return;
  if (out_id) {
    const uint32_t tq = best_tq[id];
    out_id[i] = id;
    out_q[i] = tq & ((1u << 27) - 1u);
    out_table[i] = tq >> 27;
    out_dist[i] = __longlong_as_double((long long)best_dist[id]);
  }
  best_dist[id] = HS_ANNOT_EMPTY;
}

}  // namespace

hipError_t hs_launch_annot_reduce(const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_q,
                                  const uint32_t* d_id, const uint32_t* d_table, const double* d_dist,
                                  uint32_t n_hits, uint64_t* d_best_dist, uint32_t* d_best_tq, uint32_t n_slots,
                                  uint32_t* d_touched, uint32_t* d_n_touched, hipStream_t s) {
  if (!n_hits) return hipSuccess;
  unsigned long long* const bd = reinterpret_cast<unsigned long long*>(d_best_dist);
  hs_annot_min_kernel<<<annot_blocks(n_hits), 256, 0, s>>>(d_key, d_val, d_q, d_id, d_table, d_dist, n_hits, bd,
                                                          d_best_tq, n_slots, d_touched, d_n_touched);
  hs_annot_tq_kernel<<<annot_blocks(n_hits), 256, 0, s>>>(d_key, d_val, d_q, d_id, d_table, d_dist, n_hits, bd,
                                                         d_best_tq, n_slots);
  return hipGetLastError();
}

hipError_t hs_launch_annot_gather(const uint32_t* d_sorted_id, uint32_t cnt, uint64_t* d_best_dist,
                                  const uint32_t* d_best_tq, uint32_t n_slots, uint32_t* d_out_id, uint32_t* d_out_q,
                                  uint32_t* d_out_table, double* d_out_dist, hipStream_t s) {
  if (!cnt) return hipSuccess;
  hs_annot_gather_kernel<<<annot_blocks(cnt), 256, 0, s>>>(d_sorted_id, cnt,
                                                          reinterpret_cast<unsigned long long*>(d_best_dist),
                                                          d_best_tq, n_slots, d_out_id, d_out_q, d_out_table,
                                                          d_out_dist);
  return hipGetLastError();
}

// ---- the same rule on the host (no GPU, no handle) ---------------------------------------------------
extern "C" hs_status hs_merge_best(const uint32_t* id, const uint32_t* q, const uint32_t* table, const double* dist,
                                   uint64_t n, uint32_t* out_id, uint32_t* out_q, uint32_t* out_table,
                                   double* out_dist, uint64_t cap, uint64_t* n_out) {
  if (!n_out) return HS_ERR_INVALID;
  *n_out = 0;
  if (n && (!id || !q || !table || !dist)) return HS_ERR_INVALID;
  if (cap && (!out_id || !out_q || !out_table || !out_dist)) return HS_ERR_INVALID;
  try {
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) {
      if (id[x] != id[y]) return id[x] < id[y];
      if (dist[x] != dist[y]) return dist[x] < dist[y];
      if (table[x] != table[y]) return table[x] < table[y];
      return q[x] < q[y];
    });
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n; ++i)
      if (i == 0 || id[order[i]] != id[order[i - 1]]) order[kept++] = order[i];
    *n_out = kept;
    if (kept > cap) return HS_ERR_CAPACITY;
    for (uint64_t i = 0; i < kept; ++i) {
      const uint64_t j = order[i];
      out_id[i] = id[j];
      out_q[i] = q[j];
      out_table[i] = table[j];
      out_dist[i] = dist[j];
    }
  } catch (const std::bad_alloc&) {
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}
