// hs_pssm_weights.hip -- hs_pssm_weighted_counts: position-based sequence weights (Henikoff and Henikoff 1994) and the
// weighted position frequency matrices of a profile scan's hits, reduced on the device (include/hsearch.h), and the
// host rules of hs_pssm_weights.h behind the C ABI (hs_pssm_weight_hits, hs_pssm_log_odds_weighted, hs_pssm_weight_u).
//
// A second sink stage of the scan's batch loop, after hs_pssm_counts.hip's: every hit of a profile lies in one batch,
// so the batch's raw counts are final when its count kernel has run, and the weights of its sites follow from them in
// one more pass over the same site list and the same (profile run, chunk) work items.  Per batch of mb profiles:
//   table   one wave per profile: r[p] = the residues that occur at position p, u[p][a] = floor(2^56 / (r[p] c[p][a]))
//           into a [mb][k][alphabet] uint64 scratch, distinct = the sum over p of r[p]
//   weight  one work item per wave, as hs_pc_count_kernel reads them.  The lpm lanes of a site add up their positions'
//           u and reduce W(i) across the lane group with shuffles; every lane then adds W(i) to the bins of its
//           positions in the wave's [k][alphabet] uint64 LDS histogram (one 64-bit LDS atomic each).  At most 75 x 32
//           x 8 = 19 200 bytes per wave, so a workgroup holds as many waves (4, or 3 above 16 KB) as fit 64 KB.  A
//           whole run is stored plainly; a cut run adds its non-zero bins with 64-bit integer atomics onto the zeroed
//           wcounts.
//   wsum    wsum[m] = the sum over a of wcounts[m][0][a] (every site adds W(i) to one bin of every position)
// Integer sums below 2^63 (hs_pssm_weights.h): the result does not depend on the chunk size, the order of the items
// or the order inside a run.  All stores are vector stores.
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_pssm_weights.h"

namespace {

typedef unsigned long long u64;

#define PW_LDS_BYTES 65536u

// Profile m0 + blockIdx.x of the batch: counts [k][alphabet] -> u [k][alphabet], distinct.  One wave; lane l takes the
// positions l, l + 64, ...
__global__ __launch_bounds__(64) void hs_pw_table_kernel(const uint32_t* __restrict__ counts, uint32_t k,
                                                         uint32_t alphabet, u64* __restrict__ u,
                                                         uint32_t* __restrict__ distinct) {
  const size_t cells = (size_t)k * alphabet;
  const uint32_t* const c = counts + blockIdx.x * cells;
  u64* const out = u + blockIdx.x * cells;
  uint32_t mine = 0;
  for (uint32_t p = threadIdx.x; p < k; p += 64u) {
    const uint32_t* const row = c + (size_t)p * alphabet;
    uint32_t r = 0;
    for (uint32_t a = 0; a < alphabet; ++a) r += row[a] > 0u;
    for (uint32_t a = 0; a < alphabet; ++a) out[(size_t)p * alphabet + a] = hs_pssm_weight_unit(r, row[a]);
    mine += r;
  }
  for (uint32_t o = 32u; o; o >>= 1) mine += __shfl_xor(mine, o);
  if (distinct && threadIdx.x == 0) distinct[blockIdx.x] = mine;
}

// Item blockIdx.x * waves + wave, decoded as hs_pc_count_kernel decodes it; u: the batch's tables, profile j's at
// j * cells.
__global__ __launch_bounds__(256) void hs_pw_weight_kernel(const uint8_t* __restrict__ codes, uint32_t k,
                                                           uint32_t alphabet, const uint32_t* __restrict__ site_id,
                                                           const uint32_t* __restrict__ start,
                                                           const uint32_t* __restrict__ off, uint32_t m0, uint32_t mb,
                                                           uint32_t ch, uint32_t n_items, uint32_t lpm_shift,
                                                           const u64* __restrict__ u, u64* __restrict__ wcounts) {
  extern __shared__ u64 pw_hist[];  // [waves][cells]
  const uint32_t cells = k * alphabet;
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  u64* const mine = pw_hist + (size_t)wave * cells;
  const uint32_t item = blockIdx.x * waves + wave;
  const bool active = item < n_items;
  uint32_t j = 0, lo = 0, hi = 0;
  bool whole = false;
  if (active) {
    uint32_t a = 0, b = mb;  // off[a] <= item < off[b]
    while (b - a > 1u) {
      const uint32_t mid = (a + b) >> 1;
      if (off[mid] <= item) a = mid; else b = mid;
    }
    j = a;
    const uint32_t s0 = start[j], s1 = start[j + 1u];
    const u64 at = (u64)s0 + (u64)(item - off[j]) * ch;
    lo = (uint32_t)(at < s1 ? at : s1);
    hi = (u64)s1 - lo < ch ? s1 : lo + ch;
    whole = off[j + 1u] - off[j] == 1u;
  }
  for (uint32_t c = lane; c < cells; c += 64u) mine[c] = 0ull;
  __syncthreads();
  if (active) {
    const uint32_t lpm = 1u << lpm_shift;        // lanes per site: the power of two >= k, at most 64
    const uint32_t per_wave = 64u >> lpm_shift;  // sites a wave reads per step
    const uint32_t sub = lane & (lpm - 1u), slot = lane >> lpm_shift;
    const u64* const tab = u + (size_t)j * cells;
    // (the wave walks its sites together, so that every lane takes part in the shuffles; a lane group past the end
    // carries zeros)
    for (u64 base = lo; base < hi; base += per_wave) {
      const u64 s = base + slot;
      const bool live = s < hi;
      const uint8_t* const row = codes + (live ? (size_t)site_id[s] * k : 0);
      u64 w = 0;
      if (live)
        for (uint32_t p = sub; p < k; p += lpm) {
          // (hs_index_build refuses a code >= alphabet, so the test never fails; it keeps the indices inside the tables)
          const uint32_t a = row[p];
          if (a < alphabet) w += tab[p * alphabet + a];
        }
      for (uint32_t o = lpm >> 1; o; o >>= 1) w += __shfl_xor(w, o);
      if (live)
        for (uint32_t p = sub; p < k; p += lpm) {
          const uint32_t a = row[p];
          if (a < alphabet) atomicAdd(mine + p * alphabet + a, w);
        }
    }
  }
  __syncthreads();
  if (active) {
    u64* const dst = wcounts + (size_t)(m0 + j) * cells;
    for (uint32_t c = lane; c < cells; c += 64u) {
      const u64 v = mine[c];
      if (whole)
        dst[c] = v;
      else if (v)
        atomicAdd(dst + c, v);
    }
  }
}

__global__ __launch_bounds__(256) void hs_pw_sum_kernel(const u64* __restrict__ wcounts, uint32_t nm, uint32_t cells,
                                                        uint32_t alphabet, u64* __restrict__ wsum) {
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  if (m >= nm) return;
  const u64* c = wcounts + (size_t)m * cells;
  u64 sum = 0;
  for (uint32_t a = 0; a < alphabet; ++a) sum += c[a];
  wsum[m] = sum;
}

}  // namespace

size_t hs_pssm_weights_table_bytes(uint32_t mb, int k, int alphabet) { return (size_t)mb * k * alphabet * 8; }

hipError_t hs_launch_pssm_weights_table(const uint32_t* d_counts, uint32_t mb, int k, int alphabet, uint64_t* d_u,
                                        uint32_t* d_distinct, hipStream_t s) {
  if (!mb) return hipSuccess;
  hs_pw_table_kernel<<<mb, 64, 0, s>>>(d_counts, (uint32_t)k, (uint32_t)alphabet, reinterpret_cast<u64*>(d_u),
                                       d_distinct);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_weights(const uint8_t* d_codes, int k, int alphabet, const uint32_t* d_site_id,
                                  const uint32_t* d_start, const uint32_t* d_off, uint32_t m0, uint32_t mb, uint32_t ch,
                                  uint32_t n_items, const uint64_t* d_u, uint64_t* d_wcounts, hipStream_t s) {
  if (!n_items) return hipSuccess;
  uint32_t lpm_shift = 0;
  while ((1u << lpm_shift) < (uint32_t)k && lpm_shift < 6u) ++lpm_shift;
  const size_t per_wave = (size_t)k * alphabet * 8;
  if (per_wave > PW_LDS_BYTES) return hipErrorInvalidValue;
  const uint32_t waves = (uint32_t)(PW_LDS_BYTES / per_wave < 4u ? PW_LDS_BYTES / per_wave : 4u);
  hs_pw_weight_kernel<<<(n_items + waves - 1u) / waves, waves * 64u, waves * per_wave, s>>>(
      d_codes, (uint32_t)k, (uint32_t)alphabet, d_site_id, d_start, d_off, m0, mb, ch, n_items, lpm_shift,
      reinterpret_cast<const u64*>(d_u), reinterpret_cast<u64*>(d_wcounts));
  return hipGetLastError();
}

hipError_t hs_launch_pssm_weights_sum(const uint64_t* d_wcounts, uint32_t nm, int k, int alphabet, uint64_t* d_wsum,
                                      hipStream_t s) {
  if (!nm || !d_wsum) return hipSuccess;
  hs_pw_sum_kernel<<<(nm + 255u) / 256u, 256, 0, s>>>(reinterpret_cast<const u64*>(d_wcounts), nm,
                                                     (uint32_t)(k * alphabet), (uint32_t)alphabet,
                                                     reinterpret_cast<u64*>(d_wsum));
  return hipGetLastError();
}

static hs_status pw_status(int r) { return r == 0 ? HS_OK : r == 2 ? HS_ERR_NOMEM : HS_ERR_INVALID; }

extern "C" hs_status hs_pssm_weight_hits(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet,
                                         const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                         uint64_t nm, const uint64_t* id_start, uint64_t n_seq, uint32_t* counts,
                                         uint64_t* wcounts, uint64_t* wsum, uint32_t* distinct, uint64_t* used) {
  return pw_status(hs_pssm_weight_hits_host(codes, n, k, alphabet, m, id, score, n_tuples, nm, id_start, n_seq, counts,
                                            wcounts, wsum, distinct, used));
}

extern "C" hs_status hs_pssm_log_odds_weighted(const uint64_t* wcounts, const uint64_t* wsum, const double* n_eff,
                                               uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                               double pseudo, double* S_out) {
  return pw_status(hs_pssm_log_odds_weighted_host(wcounts, wsum, n_eff, nm, k, alphabet, bg, pseudo, S_out));
}

extern "C" uint64_t hs_pssm_weight_u(uint32_t r, uint32_t c) { return hs_pssm_weight_unit(r, c); }
