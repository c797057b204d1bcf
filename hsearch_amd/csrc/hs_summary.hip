// hs_summary.hip -- cluster profiles, centroids and covering radii from a label array, reduced on the device
// (hs_cluster_profile, hs_cluster_radii, include/hsearch.h), and the same rule on the host (hs_cluster_summary_codes).
//
// Every reduction here is order-free: the counts are integers, max and min of the d2 bit patterns are exact (a d2
// is >= +0, so its bits order like the doubles), the medoid is the smallest id among the members AT the minimum.  So
// nothing is sorted, and the order in which the device groups the members never shows in a result.
//
// State of the handle, sized by the index (n k-mers), reset at the start of every call -- 36 bytes per k-mer:
//   size    [n + 1] u32  members per label value
//   tmp     [n + 1] u32  the flags, then the kept sizes, on their way into the two scans
//   row_of  [n + 1] u32  exclusive scan of (size >= min_size): the row of a label value; [n] = the number of rows
//   off_of  [n + 1] u32  exclusive scan of the kept sizes: the first member slot of a label value; [n] = the kept
//                        members.  The scatter then uses it as the rows' cursors
//   row_label [n], row_off [n + 1] u32  per ROW: its label and its range of member[]
//   member  [n] u32      the kept ids, row after row; the order inside a row is whatever the device produced
//   d2      [n] u64      hs_cluster_radii: the bits of every member's d2, by member slot
//
// Work items of the profile and radius kernels are CH consecutive member SLOTS (HS_OPT_SUMMARY_CHUNK), not rows: a
// row of 10^6 members is 10^6 / CH items, and an item over small rows holds many of them.  The pieces of rows inside
// an item (segments) are dealt to the workgroup's four waves, each with a histogram (a staged centre) of its own in
// LDS; an item that lies inside one row is shared by the four waves instead.  A segment that is its whole row is
// flushed with plain stores, any other with one global atomic per non-zero cell.  The decoding of an item's segments
// (hs_sm_segment) lives in hs_internal.h: hs_cluster_pssm.hip walks the same items over the same state.
//
// All stores are vector stores; no inline assembly.
#include <math.h>

#include <algorithm>
#include <new>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/hs_tables.h"
#include "hs_internal.h"

namespace {

constexpr uint32_t SM_WAVES = HS_SM_WAVES;  // waves per workgroup of the item kernels

inline unsigned sm_blocks(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

// `add` to *p for every lane with live set, each lane receiving the value before its own add.  A wave whose live
// lanes all name the same address (a cluster that holds everything: 10^6 k-mers, one label) issues ONE atomic.
__device__ __forceinline__ uint32_t sm_wave_add(uint32_t* base, uint32_t idx, bool live) {
  const uint64_t mask = __ballot(live);
  if (!mask) return 0;
  const int leader = __ffsll((long long)mask) - 1;
  const uint32_t idx0 = (uint32_t)__shfl((int)idx, leader);
  const bool uniform = __ballot(live && idx != idx0) == 0;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t old = 0;
  if (uniform) {
    if ((int)lane == leader) old = atomicAdd(base + idx0, (uint32_t)__popcll(mask));
    old = (uint32_t)__shfl((int)old, leader) + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  } else if (live) {
    old = atomicAdd(base + idx, 1u);
  }
  return old;
}

// 1. sizes and validation: a label is HS_NOISE or < n
__global__ __launch_bounds__(256) void hs_sm_size_kernel(const uint32_t* __restrict__ label, uint32_t n,
                                                         uint32_t* __restrict__ size, uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t lab = HS_NOISE;
  if (i < n) lab = label[i];
  const bool live = lab < n, bad = !live && lab != HS_NOISE;
  if (__ballot(bad) && (threadIdx.x & 63u) == 0) atomicOr(err, 1u);
  (void)sm_wave_add(size, lab, live);
}

// 2. what goes into the scans: v = 0 .. n (slot n closes them)
__global__ __launch_bounds__(256) void hs_sm_flag_kernel(const uint32_t* __restrict__ size, uint32_t n,
                                                         uint32_t min_size, int sizes, uint32_t* __restrict__ out) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v > n) return;
  const uint32_t s = v < n ? size[v] : 0u;
  out[v] = s >= min_size && v < n ? (sizes ? s : 1u) : 0u;
}

__global__ __launch_bounds__(256) void hs_sm_rows_kernel(const uint32_t* __restrict__ size,
                                                         const uint32_t* __restrict__ row_of,
                                                         const uint32_t* __restrict__ off_of, uint32_t n,
                                                         uint32_t min_size, uint32_t* __restrict__ row_label,
                                                         uint32_t* __restrict__ row_off) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v > n) return;
  const uint32_t r = row_of[v];
  if (r > n) return;
  if (v == n) {
    row_off[r] = off_of[n];
  } else if (size[v] >= min_size && r < n) {
    row_label[r] = v;
    row_off[r] = off_of[v];
  }
}

// 3. grouping: off_of[label] is the row's cursor from here on (row_off keeps the offsets)
__global__ __launch_bounds__(256) void hs_sm_scatter_kernel(const uint32_t* __restrict__ label, uint32_t n,
                                                            uint32_t min_size, const uint32_t* __restrict__ size,
                                                            uint32_t* __restrict__ cursor,
                                                            uint32_t* __restrict__ member) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t lab = HS_NOISE;
  if (i < n) lab = label[i];
  const bool live = lab < n && size[lab] >= min_size;
  const uint32_t pos = sm_wave_add(cursor, live ? lab : 0u, live);
  if (live && pos < n) member[pos] = i;
}

__global__ __launch_bounds__(256) void hs_sm_head_kernel(const uint32_t* __restrict__ row_label,
                                                         const uint32_t* __restrict__ row_off, uint32_t n_rows,
                                                         uint32_t* __restrict__ out_label,
                                                         uint32_t* __restrict__ out_size) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_rows) return;
  out_label[r] = row_label[r];
  out_size[r] = row_off[r + 1] - row_off[r];
}

// rows of the batch [r0, r1) that more than one item touches are summed with atomics: they start from zero
__global__ __launch_bounds__(256) void hs_sm_zero_split_kernel(const uint32_t* __restrict__ row_off, uint32_t r0,
                                                               uint32_t r1, uint32_t ch, uint32_t cells,
                                                               uint32_t* __restrict__ counts) {
  const uint32_t r = r0 + blockIdx.x;
  if (r >= r1) return;
  const uint32_t base = row_off[r0], lo = row_off[r] - base, hi = row_off[r + 1] - 1u - base;
  if (lo / ch == hi / ch) return;
  uint32_t* dst = counts + (size_t)(r - r0) * cells;
  for (uint32_t c = threadIdx.x; c < cells; c += 256u) dst[c] = 0u;
}

// 4. the profile of rows [r0, r1): counts[(row - r0)][k][alphabet]
__global__ __launch_bounds__(256) void hs_sm_profile_kernel(const uint8_t* __restrict__ codes, uint32_t k,
                                                            uint32_t alphabet, const uint32_t* __restrict__ label,
                                                            const uint32_t* __restrict__ row_of,
                                                            const uint32_t* __restrict__ row_off,
                                                            const uint32_t* __restrict__ member, uint32_t r0,
                                                            uint32_t r1, uint32_t ch, uint32_t lpm_shift,
                                                            uint32_t* __restrict__ counts) {
  extern __shared__ uint32_t sm_hist[];  // [SM_WAVES][cells]
  const uint32_t cells = k * alphabet;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  uint32_t* const mine = sm_hist + wave * cells;
  const uint32_t p_base = row_off[r0], p_end = row_off[r1];
  const uint32_t n_items = (p_end - p_base + ch - 1u) / ch;
  const uint32_t lpm = 1u << lpm_shift;             // lanes per member: the power of two >= k, at most 64
  const uint32_t per_wave = 64u >> lpm_shift;       // members a wave reads per step
  const uint32_t sub = lane & (lpm - 1u), slot = lane >> lpm_shift;
  for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const uint32_t p0 = p_base + item * ch, p1 = p_end - p0 < ch ? p_end : p0 + ch;
    const uint32_t rf = row_of[label[member[p0]]], rl = row_of[label[member[p1 - 1u]]];
    const uint32_t nseg = rl - rf + 1u;
    const bool shared = nseg == 1u;
    const uint32_t rounds = shared ? 1u : (nseg + SM_WAVES - 1u) / SM_WAVES;
    for (uint32_t round = 0; round < rounds; ++round) {
      const hs_sm_seg s = hs_sm_segment(row_off, rf, nseg, round, wave, p0, p1);
      for (uint32_t c = lane; c < cells; c += 64u) mine[c] = 0u;
      __syncthreads();
      if (s.active) {
        const uint32_t step = shared ? SM_WAVES * per_wave : per_wave;
        for (uint32_t m = s.lo + (shared ? wave * per_wave : 0u) + slot; m < s.hi; m += step) {
          const uint8_t* row = codes + (size_t)member[m] * k;
          for (uint32_t p = sub; p < k; p += lpm) {
            // (hs_index_build refuses a DB code >= alphabet, so the test never fails; it keeps the LDS index inside
            // the histogram whatever the codes array holds.  The host rule, which is handed its codes, rejects them.)
            const uint32_t a = row[p];
            if (a < alphabet) atomicAdd(mine + p * alphabet + a, 1u);
          }
        }
      }
      __syncthreads();
      uint32_t* const dst = counts + (size_t)(s.row - r0) * cells;
      if (shared) {
        for (uint32_t c = threadIdx.x; c < cells; c += 256u) {
          const uint32_t v = sm_hist[c] + sm_hist[cells + c] + sm_hist[2u * cells + c] + sm_hist[3u * cells + c];
          if (s.whole)
            dst[c] = v;
          else if (v)
            atomicAdd(dst + c, v);
        }
      } else if (s.active) {
        for (uint32_t c = lane; c < cells; c += 64u) {
          const uint32_t v = mine[c];
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

// 5. centroid[row][p * 8 + c] = (sum over a ascending of (double)count[p][a] * coords[a][c]) / size: every product
// and sum rounded (this file is compiled without contraction), one division
__global__ __launch_bounds__(256) void hs_sm_centroid_kernel(const uint32_t* __restrict__ counts,
                                                             const double* __restrict__ coords, uint32_t k,
                                                             uint32_t alphabet, const uint32_t* __restrict__ row_off,
                                                             uint32_t r0, uint32_t r1, double* __restrict__ centroid) {
  const uint32_t d = 8u * k;
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (e >= (uint64_t)(r1 - r0) * d) return;
  const uint32_t row = (uint32_t)(e / d), t = (uint32_t)(e % d), p = t >> 3, c = t & 7u;
  const uint32_t* cnt = counts + ((size_t)row * k + p) * alphabet;
  double sum = 0.0;
  for (uint32_t a = 0; a < alphabet; ++a) {
    const double prod = (double)cnt[a] * coords[a * 8u + c];
    sum = sum + prod;
  }
  const uint32_t size = row_off[r0 + row + 1u] - row_off[r0 + row];
  centroid[(size_t)(r0 + row) * d + t] = sum / (double)size;
}

__device__ __forceinline__ unsigned long long sm_wave_max(unsigned long long v) {
  for (int o = 32; o; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long sm_wave_min(unsigned long long v) {
  for (int o = 32; o; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}

// 6. d2 of every member to its row's centre, left to right; max and min per row on the bit patterns
__global__ __launch_bounds__(256) void hs_sm_radii_kernel(const uint8_t* __restrict__ codes, uint32_t k,
                                                          uint32_t alphabet, const double* __restrict__ coords,
                                                          const uint32_t* __restrict__ label,
                                                          const uint32_t* __restrict__ row_of,
                                                          const uint32_t* __restrict__ row_off,
                                                          const uint32_t* __restrict__ member, uint32_t n_rows,
                                                          uint32_t ch, const double* __restrict__ centers,
                                                          unsigned long long* __restrict__ d2_bits,
                                                          unsigned long long* __restrict__ max_bits,
                                                          unsigned long long* __restrict__ min_bits) {
  extern __shared__ double sm_f64[];  // coords [HS_ALPHABET_PAD][8], then a centre row [d] per wave
  const uint32_t d = 8u * k;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  double* const tab = sm_f64;
  double* const centre = sm_f64 + HS_ALPHABET_PAD * 8 + wave * d;
  for (uint32_t c = threadIdx.x; c < HS_ALPHABET_PAD * 8u; c += 256u) tab[c] = c < alphabet * 8u ? coords[c] : 0.0;
  const uint32_t p_end = row_off[n_rows];
  const uint32_t n_items = (p_end + ch - 1u) / ch;
  for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const uint32_t p0 = item * ch, p1 = p_end - p0 < ch ? p_end : p0 + ch;
    const uint32_t rf = row_of[label[member[p0]]], rl = row_of[label[member[p1 - 1u]]];
    const uint32_t nseg = rl - rf + 1u;
    const bool shared = nseg == 1u;
    const uint32_t rounds = shared ? 1u : (nseg + SM_WAVES - 1u) / SM_WAVES;
    for (uint32_t round = 0; round < rounds; ++round) {
      const hs_sm_seg s = hs_sm_segment(row_off, rf, nseg, round, wave, p0, p1);
      if (s.active)
        for (uint32_t t = lane; t < d; t += 64u) centre[t] = centers[(size_t)s.row * d + t];
      __syncthreads();
      unsigned long long mx = 0ull, mn = ~0ull;
      if (s.active) {
        const uint32_t step = shared ? SM_WAVES * 64u : 64u;
        for (uint32_t m = s.lo + (shared ? wave * 64u : 0u) + lane; m < s.hi; m += step) {
          const uint8_t* row = codes + (size_t)member[m] * k;
          double d2 = 0.0;
          for (uint32_t p = 0; p < k; ++p) {
            // (as in the profile kernel: a code >= alphabet cannot be in a built index; the mask keeps the index
            // inside the staged table, whose rows from `alphabet` on are zero)
            const uint32_t a = row[p] & (HS_ALPHABET_PAD - 1u);
#pragma unroll
            for (uint32_t c = 0; c < 8u; ++c) {
              const double df = tab[a * 8u + c] - centre[p * 8u + c];
              const double sq = df * df;
              d2 = d2 + sq;
            }
          }
          const unsigned long long b = (unsigned long long)__double_as_longlong(d2);
          d2_bits[m] = b;
          mx = b > mx ? b : mx;
          mn = b < mn ? b : mn;
        }
      }
      mx = sm_wave_max(mx);
      mn = sm_wave_min(mn);
      if (s.active && lane == 0 && mn != ~0ull) {
        atomicMax(max_bits + s.row, mx);
        atomicMin(min_bits + s.row, mn);
      }
      __syncthreads();
    }
  }
}

// ... the medoid: the smallest id among the members whose d2 IS the row's minimum (the two-pass shape of
// hs_annotate.hip: the minimum is final behind the kernel boundary)
__global__ __launch_bounds__(256) void hs_sm_medoid_kernel(const uint32_t* __restrict__ label,
                                                           const uint32_t* __restrict__ row_of,
                                                           const uint32_t* __restrict__ member, uint32_t n_kept,
                                                           uint32_t n_rows,
                                                           const unsigned long long* __restrict__ d2_bits,
                                                           const unsigned long long* __restrict__ min_bits,
                                                           uint32_t* __restrict__ medoid) {
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  if (m >= n_kept) return;
  const uint32_t i = member[m], r = row_of[label[i]];
  if (r < n_rows && d2_bits[m] == min_bits[r]) atomicMin(medoid + r, i);
}

__host__ __device__ inline double sm_radius_covering(double d2) {
  double r = sqrt(d2);
  if (r * r < d2) {  // the next double up (r > 0 here)
    unsigned long long b;
    memcpy(&b, &r, 8);
    ++b;
    memcpy(&r, &b, 8);
  }
  return r;
}

// ... and the radius per row; min_bits lived in the radius array until here
__global__ __launch_bounds__(256) void hs_sm_radius_kernel(const double* __restrict__ max_d2, uint32_t n_rows,
                                                           double* __restrict__ radius) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r < n_rows) radius[r] = sm_radius_covering(max_d2[r]);
}

}  // namespace

hipError_t hs_launch_sm_group(const uint32_t* d_label, uint32_t n, uint32_t min_size, uint32_t* d_size, uint32_t* d_tmp,
                              uint32_t* d_row_of, uint32_t* d_off_of, void* d_temp, size_t temp_bytes, uint32_t* d_err,
                              hipStream_t s) {
  hipError_t e = hipMemsetAsync(d_size, 0, ((size_t)n + 1) * 4, s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_err, 0, 4, s)) != hipSuccess) return e;
  if (n) hs_sm_size_kernel<<<sm_blocks(n), 256, 0, s>>>(d_label, n, d_size, d_err);
  hs_sm_flag_kernel<<<sm_blocks((uint64_t)n + 1), 256, 0, s>>>(d_size, n, min_size, 0, d_tmp);
  if ((e = hs_exclusive_scan_u32(d_temp, temp_bytes, d_tmp, d_row_of, (size_t)n + 1, s)) != hipSuccess) return e;
  hs_sm_flag_kernel<<<sm_blocks((uint64_t)n + 1), 256, 0, s>>>(d_size, n, min_size, 1, d_tmp);
  if ((e = hs_exclusive_scan_u32(d_temp, temp_bytes, d_tmp, d_off_of, (size_t)n + 1, s)) != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t hs_launch_sm_members(const uint32_t* d_label, uint32_t n, uint32_t min_size, const uint32_t* d_size,
                                const uint32_t* d_row_of, uint32_t* d_off_of, uint32_t* d_row_label,
                                uint32_t* d_row_off, uint32_t* d_member, hipStream_t s) {
  hs_sm_rows_kernel<<<sm_blocks((uint64_t)n + 1), 256, 0, s>>>(d_size, d_row_of, d_off_of, n, min_size, d_row_label,
                                                              d_row_off);
  if (n) hs_sm_scatter_kernel<<<sm_blocks(n), 256, 0, s>>>(d_label, n, min_size, d_size, d_off_of, d_member);
  return hipGetLastError();
}

hipError_t hs_launch_sm_head(const uint32_t* d_row_label, const uint32_t* d_row_off, uint32_t n_rows,
                             uint32_t* d_out_label, uint32_t* d_out_size, hipStream_t s) {
  if (!n_rows) return hipSuccess;
  hs_sm_head_kernel<<<sm_blocks(n_rows), 256, 0, s>>>(d_row_label, d_row_off, n_rows, d_out_label, d_out_size);
  return hipGetLastError();
}

hipError_t hs_launch_sm_profile(const uint8_t* d_codes, int k, int alphabet, const uint32_t* d_label,
                                const uint32_t* d_row_of, const uint32_t* d_row_off, const uint32_t* d_member,
                                uint32_t r0, uint32_t r1, uint32_t ch, uint32_t n_kept, uint32_t* d_counts,
                                int n_cu, hipStream_t s) {
  if (r1 <= r0 || !n_kept) return hipSuccess;
  const uint32_t cells = (uint32_t)(k * alphabet);
  hs_sm_zero_split_kernel<<<r1 - r0, 256, 0, s>>>(d_row_off, r0, r1, ch, cells, d_counts);
  const uint64_t items = ((uint64_t)n_kept + ch - 1) / ch;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(items, (uint64_t)n_cu * 8));
  hs_sm_profile_kernel<<<grid, 256, (size_t)SM_WAVES * cells * 4, s>>>(d_codes, (uint32_t)k, (uint32_t)alphabet, d_label,
                                                                      d_row_of, d_row_off, d_member, r0, r1, ch,
                                                                      hs_sm_lpm_shift(k), d_counts);
  return hipGetLastError();
}

hipError_t hs_launch_sm_centroid(const uint32_t* d_counts, const double* d_coords, int k, int alphabet,
                                 const uint32_t* d_row_off, uint32_t r0, uint32_t r1, double* d_centroid,
                                 hipStream_t s) {
  if (r1 <= r0) return hipSuccess;
  hs_sm_centroid_kernel<<<sm_blocks((uint64_t)(r1 - r0) * 8u * k), 256, 0, s>>>(
      d_counts, d_coords, (uint32_t)k, (uint32_t)alphabet, d_row_off, r0, r1, d_centroid);
  return hipGetLastError();
}

hipError_t hs_launch_sm_radii(const uint8_t* d_codes, int k, int alphabet, const double* d_coords,
                              const uint32_t* d_label, const uint32_t* d_row_of, const uint32_t* d_row_off,
                              const uint32_t* d_member, uint32_t n_rows, uint32_t n_kept, uint32_t ch,
                              const double* d_centers, uint64_t* d_d2, double* d_max_d2, double* d_radius,
                              uint32_t* d_medoid, int n_cu, hipStream_t s) {
  if (!n_rows || !n_kept) return hipSuccess;
  unsigned long long* const mx = reinterpret_cast<unsigned long long*>(d_max_d2);
  unsigned long long* const mn = reinterpret_cast<unsigned long long*>(d_radius);
  hipError_t e = hipMemsetAsync(d_max_d2, 0, (size_t)n_rows * 8, s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_radius, 0xff, (size_t)n_rows * 8, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_medoid, 0xff, (size_t)n_rows * 4, s)) != hipSuccess) return e;
  const uint64_t items = ((uint64_t)n_kept + ch - 1) / ch;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(items, (uint64_t)n_cu * 8));
  const size_t lds = ((size_t)HS_ALPHABET_PAD * 8 + (size_t)SM_WAVES * 8 * k) * 8;
  hs_sm_radii_kernel<<<grid, 256, lds, s>>>(d_codes, (uint32_t)k, (uint32_t)alphabet, d_coords, d_label, d_row_of,
                                            d_row_off, d_member, n_rows, ch, d_centers,
                                            reinterpret_cast<unsigned long long*>(d_d2), mx, mn);
  hs_sm_medoid_kernel<<<sm_blocks(n_kept), 256, 0, s>>>(d_label, d_row_of, d_member, n_kept, n_rows,
                                                       reinterpret_cast<unsigned long long*>(d_d2), mn, d_medoid);
  hs_sm_radius_kernel<<<sm_blocks(n_rows), 256, 0, s>>>(d_max_d2, n_rows, d_radius);
  return hipGetLastError();
}

// ---- the same rule on the host (no GPU, no handle) -------------------------------------------------------
extern "C" hs_status hs_cluster_summary_codes(const uint8_t* codes, uint64_t n, uint32_t k, const double* coords,
                                              uint32_t alphabet, const uint32_t* label, uint32_t min_size,
                                              const double* centers, uint64_t n_center_rows, uint32_t* out_label,
                                              uint32_t* out_size, uint32_t* counts, double* centroid, double* max_d2,
                                              double* radius, uint32_t* medoid, uint64_t cap, uint64_t* n_out) {
  if (!n_out) return HS_ERR_INVALID;
  *n_out = 0;
  if (!coords) {
    if (alphabet != 0 && alphabet != HS_ALPHABET) return HS_ERR_INVALID;
    coords = &HS_AA_COORDS[0][0];
    alphabet = HS_ALPHABET;
  }
  if (!min_size || k < 1 || k > 75 || alphabet < 1 || alphabet > HS_ALPHABET_PAD || n >= (1ull << 31) ||
      (n && (!codes || !label)))
    return HS_ERR_INVALID;
  const bool want_radii = max_d2 || radius || medoid;
  if (want_radii && !(max_d2 && radius && medoid)) return HS_ERR_INVALID;
  if (cap && (!out_label || !out_size || !centroid)) return HS_ERR_INVALID;
  for (uint64_t i = 0; i < n; ++i)
    if (label[i] != HS_NOISE && label[i] >= n) return HS_ERR_INVALID;
  for (uint64_t i = 0; i < n * k; ++i)
    if (codes[i] >= alphabet) return HS_ERR_INVALID;
  try {
    std::vector<uint32_t> size(n, 0), row_of(n, HS_NOISE);
    for (uint64_t i = 0; i < n; ++i)
      if (label[i] != HS_NOISE) ++size[label[i]];
    uint64_t rows = 0;
    for (uint64_t v = 0; v < n; ++v)
      if (size[v] >= min_size) row_of[v] = (uint32_t)rows++;
    *n_out = rows;
    if (centers && n_center_rows != rows) return HS_ERR_INVALID;
    if (rows > cap) return HS_ERR_CAPACITY;
    const uint32_t d = 8 * k;
    const size_t cells = (size_t)k * alphabet;
    std::vector<uint32_t> own_counts;
    if (!counts) {
      own_counts.resize(rows * cells);
      counts = own_counts.data();
    }
    std::fill(counts, counts + rows * cells, 0u);
    for (uint64_t v = 0; v < n; ++v)
      if (row_of[v] != HS_NOISE) {
        out_label[row_of[v]] = (uint32_t)v;
        out_size[row_of[v]] = size[v];
      }
    for (uint64_t i = 0; i < n; ++i) {
      if (label[i] == HS_NOISE || row_of[label[i]] == HS_NOISE) continue;
      uint32_t* cnt = counts + row_of[label[i]] * cells;
      for (uint32_t p = 0; p < k; ++p) ++cnt[(size_t)p * alphabet + codes[i * k + p]];
    }
    for (uint64_t r = 0; r < rows; ++r)
      for (uint32_t t = 0; t < d; ++t) {
        const uint32_t* cnt = counts + r * cells + (size_t)(t >> 3) * alphabet;
        double sum = 0.0;
        for (uint32_t a = 0; a < alphabet; ++a) {
          const double prod = (double)cnt[a] * coords[a * 8 + (t & 7)];
          sum = sum + prod;
        }
        centroid[r * d + t] = sum / (double)out_size[r];
      }
    if (want_radii) {
      const double* ctr = centers ? centers : centroid;
      std::vector<double> best(rows, 0.0);
      for (uint64_t r = 0; r < rows; ++r) {
        max_d2[r] = 0.0;
        medoid[r] = HS_NOISE;
      }
      for (uint64_t i = 0; i < n; ++i) {  // ascending id: the first member at the minimum is the medoid
        if (label[i] == HS_NOISE || row_of[label[i]] == HS_NOISE) continue;
        const uint64_t r = row_of[label[i]];
        double d2 = 0.0;
        for (uint32_t t = 0; t < d; ++t) {
          const double df = coords[codes[i * k + (t >> 3)] * 8 + (t & 7)] - ctr[r * d + t];
          const double sq = df * df;
          d2 = d2 + sq;
        }
        uint64_t b, bb, bm;
        memcpy(&b, &d2, 8);
        memcpy(&bb, &best[r], 8);
        memcpy(&bm, &max_d2[r], 8);
        if (medoid[r] == HS_NOISE || b < bb) {  // (compared as the device compares: on the bit patterns)
          best[r] = d2;
          medoid[r] = (uint32_t)i;
        }
        if (b > bm) max_d2[r] = d2;
      }
      for (uint64_t r = 0; r < rows; ++r) radius[r] = sm_radius_covering(max_d2[r]);
    }
  } catch (const std::bad_alloc&) {
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}
