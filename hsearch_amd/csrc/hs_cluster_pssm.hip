// hs_cluster_pssm.hip -- hs_cluster_weighted_profile and hs_cluster_pssm_cover: from the clusters of a label array to
// weighted, searchable profiles on the device (include/hsearch.h), and the host rules of hs_cluster_pssm.h behind the C
// ABI (hs_cluster_weights_codes, hs_cluster_cover_codes).
//
// Both calls run on the state hs_summary.hip groups (its head lists it): the rows, their member slots, and work items of
// ch consecutive slots whose segments hs_sm_segment (hs_internal.h) deals to the workgroup's four waves.
//
// Weights, per batch of rows, behind hs_sm_profile_kernel (the batch's raw counts are final then):
//   table   hs_launch_pssm_weights_table (hs_pssm_weights.hip): one wave per row, u[p][a] = floor(2^56 / (r[p] c[p][a]))
//           into a [rows of the batch][k][alphabet] uint64 scratch, distinct = the sum over p of r[p]
//   weight  hs_cp_weight_kernel: the items and segments of the profile kernel once more.  The lpm lanes of a member add
//           up their positions' u and reduce W(i) across the lane group with shuffles; every lane then adds W(i) to the
//           bins of its positions in the wave's [k][alphabet] uint64 LDS histogram (one 64-bit LDS atomic each).  A
//           segment that is its whole row is stored plainly; a cut one adds its non-zero bins with 64-bit integer
//           atomics onto rows hs_cp_zero_split_kernel zeroed.
//   wsum    hs_launch_pssm_weights_sum: wsum[r] = the sum over a of wcounts[r][0][a]
// Integer sums below 2^63 (hs_pssm_weights.h): the chunk size, the row batches and the order of the members never show.
//
// Cover: hs_cp_cover_kernel stages a segment's profile in LDS (as hs_sm_radii_kernel stages a centre), one member per
// lane scores it left to right from +0.0 -- hs_pssm_scan's sum, bit for bit (this file is compiled without contraction;
// the sum has no product anyway) -- and keeps the order-preserving key of the bits (hs_pssm_order_key: scores are
// negative as well) per member slot and, with one atomicMin per wave and segment, per row.  hs_cp_argmin_kernel, behind
// the kernel boundary, takes the smallest id among the members AT the minimum; hs_cp_score_kernel turns the keys back.
//
// LDS: four wave-private tables of k * alphabet * 8 bytes are 76 800 bytes at k = 75, alphabet 32, above the 64 KB a
// kernel gets without asking: both item kernels ask for the dynamic-LDS grant once per process and size, as
// hs_join8r_kernel and hs_pssm_null_conv_kernel do (a CU has 160 KB, so two such workgroups still fit one).
// All stores are vector stores; no inline assembly.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "hs_cluster_pssm.h"
#include "hs_internal.h"

namespace {

typedef unsigned long long u64;

inline unsigned cp_blocks(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

// rows of the batch [r0, r1) that more than one item touches are summed with atomics: they start from zero
// (hs_sm_zero_split_kernel's test, on the 64-bit rows)
__global__ __launch_bounds__(256) void hs_cp_zero_split_kernel(const uint32_t* __restrict__ row_off, uint32_t r0,
                                                               uint32_t r1, uint32_t ch, uint32_t cells,
                                                               u64* __restrict__ wcounts) {
  const uint32_t r = r0 + blockIdx.x;
  if (r >= r1) return;
  const uint32_t base = row_off[r0], lo = row_off[r] - base, hi = row_off[r + 1] - 1u - base;
  if (lo / ch == hi / ch) return;
  u64* dst = wcounts + (size_t)(r - r0) * cells;
  for (uint32_t c = threadIdx.x; c < cells; c += 256u) dst[c] = 0ull;
}

// The weighted profile of rows [r0, r1): wcounts[(row - r0)][k][alphabet] from u[(row - r0)][k][alphabet].  Items and
// segments are hs_sm_profile_kernel's.
__global__ __launch_bounds__(256) void hs_cp_weight_kernel(const uint8_t* __restrict__ codes, uint32_t k,
                                                           uint32_t alphabet, const uint32_t* __restrict__ label,
                                                           const uint32_t* __restrict__ row_of,
                                                           const uint32_t* __restrict__ row_off,
                                                           const uint32_t* __restrict__ member, uint32_t r0,
                                                           uint32_t r1, uint32_t ch, uint32_t lpm_shift,
                                                           const u64* __restrict__ u, u64* __restrict__ wcounts) {
  extern __shared__ u64 cp_hist[];  // [HS_SM_WAVES][cells]
  const uint32_t cells = k * alphabet;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  u64* const mine = cp_hist + (size_t)wave * cells;
  const uint32_t p_base = row_off[r0], p_end = row_off[r1];
  const uint32_t n_items = (p_end - p_base + ch - 1u) / ch;
  const uint32_t lpm = 1u << lpm_shift;        // lanes per member: the power of two >= k, at most 64
  const uint32_t per_wave = 64u >> lpm_shift;  // members a wave reads per step
  const uint32_t sub = lane & (lpm - 1u), slot = lane >> lpm_shift;
  for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const uint32_t p0 = p_base + item * ch, p1 = p_end - p0 < ch ? p_end : p0 + ch;
    const uint32_t rf = row_of[label[member[p0]]], rl = row_of[label[member[p1 - 1u]]];
    const uint32_t nseg = rl - rf + 1u;
    const bool shared = nseg == 1u;
    const uint32_t rounds = shared ? 1u : (nseg + HS_SM_WAVES - 1u) / HS_SM_WAVES;
    for (uint32_t round = 0; round < rounds; ++round) {
      const hs_sm_seg s = hs_sm_segment(row_off, rf, nseg, round, wave, p0, p1);
      for (uint32_t c = lane; c < cells; c += 64u) mine[c] = 0ull;
      __syncthreads();
      if (s.active) {
        const u64* const tab = u + (size_t)(s.row - r0) * cells;
        const uint32_t step = shared ? HS_SM_WAVES * per_wave : per_wave;
        // (the wave walks its members together, so that every lane takes part in the shuffles; a lane group past the
        // end carries zeros)
        for (uint32_t base = s.lo + (shared ? wave * per_wave : 0u); base < s.hi; base += step) {
          const uint32_t m = base + slot;
          const bool live = m < s.hi;
          const uint8_t* const row = codes + (live ? (size_t)member[m] * k : 0);
          u64 w = 0;
          if (live)
            for (uint32_t p = sub; p < k; p += lpm) {
              // (hs_index_build refuses a code >= alphabet, so the test never fails; it keeps the indices inside the
              // tables)
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
      u64* const dst = wcounts + (size_t)(s.row - r0) * cells;
      if (shared) {
        for (uint32_t c = threadIdx.x; c < cells; c += 256u) {
          const u64 v = cp_hist[c] + cp_hist[cells + c] + cp_hist[2u * cells + c] + cp_hist[3u * cells + c];
          if (s.whole)
            dst[c] = v;
          else if (v)
            atomicAdd(dst + c, v);
        }
      } else if (s.active) {
        for (uint32_t c = lane; c < cells; c += 64u) {
          const u64 v = mine[c];
          if (s.whole)
            dst[c] = v;
          else if (v)
            atomicAdd(dst + c, v);
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ u64 cp_wave_min(u64 v) {
  for (int o = 32; o; o >>= 1) {
    const u64 w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}

// The key of every member's score under its row's profile, by member slot, and the rows' minima.  Items and segments
// are hs_sm_radii_kernel's (over all rows: nothing here is batched).
__global__ __launch_bounds__(256) void hs_cp_cover_kernel(const uint8_t* __restrict__ codes, uint32_t k,
                                                          uint32_t alphabet, const double* __restrict__ S,
                                                          const uint32_t* __restrict__ label,
                                                          const uint32_t* __restrict__ row_of,
                                                          const uint32_t* __restrict__ row_off,
                                                          const uint32_t* __restrict__ member, uint32_t n_rows,
                                                          uint32_t ch, u64* __restrict__ key_of,
                                                          u64* __restrict__ min_key) {
  extern __shared__ double cp_prof[];  // [HS_SM_WAVES][cells]
  const uint32_t cells = k * alphabet;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  double* const tab = cp_prof + (size_t)wave * cells;
  const uint32_t p_end = row_off[n_rows];
  const uint32_t n_items = (p_end + ch - 1u) / ch;
  for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const uint32_t p0 = item * ch, p1 = p_end - p0 < ch ? p_end : p0 + ch;
    const uint32_t rf = row_of[label[member[p0]]], rl = row_of[label[member[p1 - 1u]]];
    const uint32_t nseg = rl - rf + 1u;
    const bool shared = nseg == 1u;
    const uint32_t rounds = shared ? 1u : (nseg + HS_SM_WAVES - 1u) / HS_SM_WAVES;
    for (uint32_t round = 0; round < rounds; ++round) {
      const hs_sm_seg s = hs_sm_segment(row_off, rf, nseg, round, wave, p0, p1);
      if (s.active)
        for (uint32_t c = lane; c < cells; c += 64u) tab[c] = S[(size_t)s.row * cells + c];
      __syncthreads();
      u64 mn = ~0ull;
      if (s.active) {
        const uint32_t step = shared ? HS_SM_WAVES * 64u : 64u;
        for (uint32_t m = s.lo + (shared ? wave * 64u : 0u) + lane; m < s.hi; m += step) {
          const uint8_t* const row = codes + (size_t)member[m] * k;
          double score = 0.0;
          for (uint32_t p = 0; p < k; ++p) {
            // (a code >= alphabet cannot be in a built index; the test keeps the index inside the staged profile)
            const uint32_t a = row[p];
            score = score + tab[p * alphabet + (a < alphabet ? a : 0u)];
          }
          const u64 key = hs_pssm_order_key((u64)__double_as_longlong(score));
          key_of[m] = key;
          mn = key < mn ? key : mn;
        }
      }
      mn = cp_wave_min(mn);
      if (s.active && lane == 0 && s.lo < s.hi) atomicMin(min_key + s.row, mn);
      __syncthreads();
    }
  }
}

// ... the argmin: the smallest id among the members whose key IS the row's minimum (hs_sm_medoid_kernel's shape: the
// minimum is final behind the kernel boundary)
__global__ __launch_bounds__(256) void hs_cp_argmin_kernel(const uint32_t* __restrict__ label,
                                                           const uint32_t* __restrict__ row_of,
                                                           const uint32_t* __restrict__ member, uint32_t n_kept,
                                                           uint32_t n_rows, const u64* __restrict__ key_of,
                                                           const u64* __restrict__ min_key,
                                                           uint32_t* __restrict__ argmin) {
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  if (m >= n_kept) return;
  const uint32_t i = member[m], r = row_of[label[i]];
  if (r < n_rows && key_of[m] == min_key[r]) atomicMin(argmin + r, i);
}

// ... and the scores back from their keys; the keys lived in the score array until here
__global__ __launch_bounds__(256) void hs_cp_score_kernel(u64* __restrict__ min_key, uint32_t n_rows) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r < n_rows) min_key[r] = hs_pssm_order_bits(min_key[r]);
}

// four wave-private tables: above 64 KB the kernel asks for the grant (the largest asked for so far is kept per kernel)
template <class Kernel>
hipError_t cp_grant_lds(Kernel kernel, size_t bytes, int* granted) {
  if (bytes <= 65536u || (int)bytes <= *granted) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) *granted = (int)bytes;
  return e;
}

}  // namespace

hipError_t hs_launch_cp_weights(const uint8_t* d_codes, int k, int alphabet, const uint32_t* d_label,
                                const uint32_t* d_row_of, const uint32_t* d_row_off, const uint32_t* d_member,
                                uint32_t r0, uint32_t r1, uint32_t ch, uint32_t n_kept, const uint64_t* d_u,
                                uint64_t* d_wcounts, int n_cu, hipStream_t s) {
  if (r1 <= r0 || !n_kept) return hipSuccess;
  const uint32_t cells = (uint32_t)(k * alphabet);
  const size_t lds = (size_t)HS_SM_WAVES * cells * 8;
  static int granted = 0;
  hipError_t e = cp_grant_lds(hs_cp_weight_kernel, lds, &granted);
  if (e != hipSuccess) return e;
  hs_cp_zero_split_kernel<<<r1 - r0, 256, 0, s>>>(d_row_off, r0, r1, ch, cells, reinterpret_cast<u64*>(d_wcounts));
  const uint64_t items = ((uint64_t)n_kept + ch - 1) / ch;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(items, (uint64_t)n_cu * 8));
  hs_cp_weight_kernel<<<grid, 256, lds, s>>>(d_codes, (uint32_t)k, (uint32_t)alphabet, d_label, d_row_of, d_row_off,
                                             d_member, r0, r1, ch, hs_sm_lpm_shift(k),
                                             reinterpret_cast<const u64*>(d_u), reinterpret_cast<u64*>(d_wcounts));
  return hipGetLastError();
}

hipError_t hs_launch_cp_cover(const uint8_t* d_codes, int k, int alphabet, const double* d_S, const uint32_t* d_label,
                              const uint32_t* d_row_of, const uint32_t* d_row_off, const uint32_t* d_member,
                              uint32_t n_rows, uint32_t n_kept, uint32_t ch, uint64_t* d_key, double* d_min_score,
                              uint32_t* d_argmin, int n_cu, hipStream_t s) {
  if (!n_rows || !n_kept) return hipSuccess;
  const uint32_t cells = (uint32_t)(k * alphabet);
  const size_t lds = (size_t)HS_SM_WAVES * cells * 8;
  static int granted = 0;
  hipError_t e = cp_grant_lds(hs_cp_cover_kernel, lds, &granted);
  if (e != hipSuccess) return e;
  u64* const mn = reinterpret_cast<u64*>(d_min_score);
  if ((e = hipMemsetAsync(d_min_score, 0xff, (size_t)n_rows * 8, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_argmin, 0xff, (size_t)n_rows * 4, s)) != hipSuccess) return e;
  const uint64_t items = ((uint64_t)n_kept + ch - 1) / ch;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(items, (uint64_t)n_cu * 8));
  hs_cp_cover_kernel<<<grid, 256, lds, s>>>(d_codes, (uint32_t)k, (uint32_t)alphabet, d_S, d_label, d_row_of, d_row_off,
                                            d_member, n_rows, ch, reinterpret_cast<u64*>(d_key), mn);
  hs_cp_argmin_kernel<<<cp_blocks(n_kept), 256, 0, s>>>(d_label, d_row_of, d_member, n_kept, n_rows,
                                                       reinterpret_cast<const u64*>(d_key), mn, d_argmin);
  hs_cp_score_kernel<<<cp_blocks(n_rows), 256, 0, s>>>(mn, n_rows);
  return hipGetLastError();
}

// ---- the same rules on the host (no GPU, no handle) ------------------------------------------------------
static hs_status cp_status(int r) {
  return r == 0 ? HS_OK : r == 2 ? HS_ERR_NOMEM : r == 3 ? HS_ERR_CAPACITY : HS_ERR_INVALID;
}

extern "C" hs_status hs_cluster_weights_codes(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet,
                                              const uint32_t* label, uint32_t min_size, uint32_t* out_label,
                                              uint32_t* out_size, uint32_t* counts, uint64_t* wcounts, uint64_t* wsum,
                                              uint32_t* distinct, uint64_t cap, uint64_t* n_out) {
  return cp_status(hs_cluster_weights_codes_host(codes, n, k, alphabet, label, min_size, out_label, out_size, counts,
                                                 wcounts, wsum, distinct, cap, n_out));
}

extern "C" hs_status hs_cluster_cover_codes(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet,
                                            const uint32_t* label, uint32_t min_size, const double* S, uint64_t n_rows,
                                            double* min_score, uint32_t* argmin) {
  return cp_status(hs_cluster_cover_codes_host(codes, n, k, alphabet, label, min_size, S, n_rows, min_score, argmin));
}
