// hs_pssm_counts.hip -- hs_pssm_hit_counts: the position frequency matrices of a profile scan's hits, reduced on the
// device (include/hsearch.h), and the host rules of hs_pssm_counts.h behind the C ABI (hs_pssm_count_hits,
// hs_pssm_log_odds, hs_pssm_background).
//
// A sink of the scan's batch loop.  Counting is free of order: a profile's sites only have to lie side by side, so
// the batch's hits are split into (m, id) words and sorted on the m bits alone (a stable radix sort of 32-bit pairs
// over bit_width(m) bits; the scan's own (m, id) sort moves 16 bytes per hit through 44 bits).  In the one-site-per-
// protein mode the sites are the best ids of hs_pssm_seq.hip's rows, which already ascend in m.  Per batch of ns sites:
//   split   key m << 32 | id -> m [nh], id [nh]                                        (every-site mode only)
//   items   per profile j of the batch: where its run starts (a binary search in the sorted m) and how many chunks of
//           ch sites it is cut into; the caller's exclusive scan numbers the items, its total is read back
//   count   one work item (profile run, chunk of at most ch sites) per wave, four waves per workgroup.  The wave
//           keeps a [k][alphabet] uint32 histogram in LDS (at most 75 x 32 x 4 = 9600 bytes), reads its sites with
//           lpm = the power of two >= k lanes per site (hs_summary.hip's shape) and counts with LDS atomics.  An item
//           that holds its profile's whole run stores the histogram plainly; a run cut into several items adds its
//           non-zero bins with integer atomicAdd onto the zeroed counts.  No global atomic per hit and position.
//   used    after the last batch: used[m] = the sum over a of counts[m][0][a] (every site adds one to every position)
// Integer sums: the result does not depend on the chunk size, the order of the items or the order inside a run.
// All stores are vector stores.
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_pssm_counts.h"

namespace {

typedef unsigned long long u64;

#define PC_WAVES 4u

inline unsigned pc_blocks(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

__global__ __launch_bounds__(256) void hs_pc_split_kernel(const uint64_t* __restrict__ key, uint32_t n,
                                                          uint32_t* __restrict__ m, uint32_t* __restrict__ id) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t v = key[i];
  m[i] = (uint32_t)(v >> 32);
  id[i] = (uint32_t)v;
}

// the first site whose profile is >= m (ns when there is none)
__device__ __forceinline__ uint32_t pc_lower_bound(const uint32_t* __restrict__ site_m, uint32_t ns, uint32_t m) {
  uint32_t lo = 0, hi = ns;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (site_m[mid] < m) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// j <= mb: start[j] = where the run of profile m0 + j begins (start[mb] = ns: every site's m is below m0 + mb),
// n_item[j] = the chunks of ch sites its run is cut into (n_item[mb] = 0: its scan slot receives the total)
__global__ __launch_bounds__(256) void hs_pc_items_kernel(const uint32_t* __restrict__ site_m, uint32_t ns, uint32_t m0,
                                                          uint32_t mb, uint32_t ch, uint32_t* __restrict__ start,
                                                          uint32_t* __restrict__ n_item) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j > mb) return;
  const uint32_t a = j < mb ? pc_lower_bound(site_m, ns, m0 + j) : ns;
  const uint32_t b = j + 1u < mb ? pc_lower_bound(site_m, ns, m0 + j + 1u) : ns;
  start[j] = a;
  n_item[j] = j < mb ? (uint32_t)(((u64)(b - a) + ch - 1u) / ch) : 0u;
}

// Item blockIdx.x * 4 + wave: chunk (item - off[j]) of profile m0 + j, j = the last profile with off[j] <= item that
// has items (off [mb + 1]: the exclusive scan of n_item; off[mb] = n_items).
__global__ __launch_bounds__(256) void hs_pc_count_kernel(const uint8_t* __restrict__ codes, uint32_t k,
                                                          uint32_t alphabet, const uint32_t* __restrict__ site_id,
                                                          const uint32_t* __restrict__ start,
                                                          const uint32_t* __restrict__ off, uint32_t m0, uint32_t mb,
                                                          uint32_t ch, uint32_t n_items, uint32_t lpm_shift,
                                                          uint32_t* __restrict__ counts) {
  extern __shared__ uint32_t pc_hist[];  // [PC_WAVES][cells]
  const uint32_t cells = k * alphabet;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  uint32_t* const mine = pc_hist + wave * cells;
  const uint32_t item = blockIdx.x * PC_WAVES + wave;
  const bool active = item < n_items;
  uint32_t j = 0, lo = 0, hi = 0;
  bool whole = false;
  if (active) {
    uint32_t a = 0, b = mb;  // off[a] <= item < off[b]
    while (b - a > 1u) {
      const uint32_t mid = (a + b) >> 1;
      if (off[mid] <= item) a = mid; else b = mid;
    }
    j = a;  // (off[a + 1] > item: profile a has the item)
    const uint32_t s0 = start[j], s1 = start[j + 1u];
    const u64 at = (u64)s0 + (u64)(item - off[j]) * ch;
    lo = (uint32_t)(at < s1 ? at : s1);
    hi = (u64)s1 - lo < ch ? s1 : lo + ch;
    whole = off[j + 1u] - off[j] == 1u;
  }
  for (uint32_t c = lane; c < cells; c += 64u) mine[c] = 0u;
  __syncthreads();
  if (active) {
    const uint32_t lpm = 1u << lpm_shift;        // lanes per site: the power of two >= k, at most 64
    const uint32_t per_wave = 64u >> lpm_shift;  // sites a wave reads per step
    const uint32_t sub = lane & (lpm - 1u), slot = lane >> lpm_shift;
    for (u64 s = (u64)lo + slot; s < hi; s += per_wave) {
      const uint8_t* row = codes + (size_t)site_id[s] * k;
      for (uint32_t p = sub; p < k; p += lpm) {
        // (hs_index_build refuses a code >= alphabet, so the test never fails; it keeps the LDS index inside the
        // histogram whatever the codes array holds)
        const uint32_t a = row[p];
        if (a < alphabet) atomicAdd(mine + p * alphabet + a, 1u);
      }
    }
  }
  __syncthreads();
  if (active) {
    uint32_t* const dst = counts + (size_t)(m0 + j) * cells;
    for (uint32_t c = lane; c < cells; c += 64u) {
      const uint32_t v = mine[c];
      if (whole)
        dst[c] = v;
      else if (v)
        atomicAdd(dst + c, v);
    }
  }
}

__global__ __launch_bounds__(256) void hs_pc_used_kernel(const uint32_t* __restrict__ counts, uint32_t nm,
                                                         uint32_t cells, uint32_t alphabet, u64* __restrict__ used,
                                                         u64* __restrict__ cnt) {
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  if (m >= nm) return;
  const uint32_t* c = counts + (size_t)m * cells;
  u64 sum = 0;
  for (uint32_t a = 0; a < alphabet; ++a) sum += c[a];
  if (used) used[m] = sum;
  if (cnt) cnt[m] = sum;
}

}  // namespace

hipError_t hs_launch_pssm_counts_split(const uint64_t* d_key, uint32_t n, uint32_t* d_m, uint32_t* d_id, hipStream_t s) {
  if (!n) return hipSuccess;
  hs_pc_split_kernel<<<pc_blocks(n), 256, 0, s>>>(d_key, n, d_m, d_id);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_counts_items(const uint32_t* d_site_m, uint32_t ns, uint32_t m0, uint32_t mb, uint32_t ch,
                                       uint32_t* d_start, uint32_t* d_n_item, hipStream_t s) {
  hs_pc_items_kernel<<<pc_blocks((uint64_t)mb + 1), 256, 0, s>>>(d_site_m, ns, m0, mb, ch, d_start, d_n_item);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_counts(const uint8_t* d_codes, int k, int alphabet, const uint32_t* d_site_id,
                                 const uint32_t* d_start, const uint32_t* d_off, uint32_t m0, uint32_t mb, uint32_t ch,
                                 uint32_t n_items, uint32_t* d_counts, hipStream_t s) {
  if (!n_items) return hipSuccess;
  uint32_t lpm_shift = 0;
  while ((1u << lpm_shift) < (uint32_t)k && lpm_shift < 6u) ++lpm_shift;
  const size_t lds = (size_t)PC_WAVES * k * alphabet * 4;
  hs_pc_count_kernel<<<(n_items + PC_WAVES - 1u) / PC_WAVES, 256, lds, s>>>(d_codes, (uint32_t)k, (uint32_t)alphabet,
                                                                           d_site_id, d_start, d_off, m0, mb, ch,
                                                                           n_items, lpm_shift, d_counts);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_counts_used(const uint32_t* d_counts, uint32_t nm, int k, int alphabet, uint64_t* d_used,
                                      uint64_t* d_cnt, hipStream_t s) {
  if (!nm || (!d_used && !d_cnt)) return hipSuccess;
  hs_pc_used_kernel<<<pc_blocks(nm), 256, 0, s>>>(d_counts, nm, (uint32_t)(k * alphabet), (uint32_t)alphabet,
                                                  reinterpret_cast<u64*>(d_used), reinterpret_cast<u64*>(d_cnt));
  return hipGetLastError();
}

static hs_status pc_status(int r) { return r == 0 ? HS_OK : r == 2 ? HS_ERR_NOMEM : HS_ERR_INVALID; }

extern "C" hs_status hs_pssm_count_hits(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet,
                                        const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                        uint64_t nm, const uint64_t* id_start, uint64_t n_seq, uint32_t* counts,
                                        uint64_t* used) {
  return pc_status(hs_pssm_count_hits_host(codes, n, k, alphabet, m, id, score, n_tuples, nm, id_start, n_seq, counts,
                                           used));
}

extern "C" hs_status hs_pssm_log_odds(const uint32_t* counts, uint64_t nm, uint32_t k, uint32_t alphabet,
                                      const double* bg, double pseudo, double* S_out) {
  return pc_status(hs_pssm_log_odds_host(counts, nm, k, alphabet, bg, pseudo, S_out));
}

extern "C" hs_status hs_pssm_background(const uint32_t* counts_row, uint32_t k, uint32_t alphabet, double* bg_out) {
  return pc_status(hs_pssm_background_host(counts_row, k, alphabet, bg_out));
}
