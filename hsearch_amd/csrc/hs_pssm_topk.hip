// hs_pssm_topk.hip -- hs_pssm_topk: the topk best k-mers of every profile without a threshold (include/hsearch.h), and
// the same rule on the host for any list of tuples (hs_pssm_topk_hits).  The order and its argument: hs_pssm_topk.h.
//
// Why it is exact.  If t' is the topk-th largest contract score among ANY subset of the index, at least topk k-mers of
// the index score >= t', so every member of the true row scores >= t', ties included: a scan under hs_pssm_scan's
// rule at max(floor, t') returns a superset of the row, and the row is the best of that superset.  The subset only
// decides how much the scan returns, never what the row is.
//
// Per batch of profiles (a range of profiles against the whole index: all hits of a profile lie in one batch):
//   1. hs_pssm_sample_kernel   one workgroup of 4 waves per profile; the profile's S block sits in LDS; sample j is
//        k-mer floor(j * n / n_s) (64-bit; n_s <= n, so the ids are distinct), one exact contract score per lane from
//        `codes`.  Each wave keeps the 64 best scores it has seen, one per lane, as descending keys in ascending order:
//        a chunk of 64 with nothing better than the list's topk-th entry is dropped after one ballot, any other is
//        sorted by the bitonic network and merged (the network of hs_knn_select_kernel on a 64-bit key: scores may
//        repeat, the list is a multiset).  The four lists merge through LDS.  t' = entry topk - 1 if it is no padding;
//        t_used = max(floor, t'), or the floor when the sample holds fewer than topk scores.  No score is stored.
//        With few profiles (fewer than 1024) a profile's sample is cut into `parts` ranges of at least 1024 samples,
//        one workgroup each, so that about 1024 workgroups run; each leaves its list of 64 in a small buffer, and
//        hs_pssm_sample_merge_kernel, one wave per profile, merges them and writes t_used.  (One workgroup per
//        profile took 1.9 ms for 16 profiles at n_s = 2^18.)  A list's entries below its topk-th need not be the
//        range's best, but they are scores of the sample: merged lists have the sample's true topk-th entry.
//   2. the scan at t_used     hs_pssm.hip's tables, filter and exact pass, unchanged (hs_capi_pssm.hip pssm_batch)
//   3. the selection           the batch's unordered hits (m << 32 | id, score bits): counted per profile, the counts
//        scanned, the hits scattered by profile as (descending key, id); one wave per profile selects as
//        hs_knn_select_kernel does, on the 128-bit key, and writes its whole row -- entries, padding -- and top_count.
// The batch's hit list is never sorted, and no kernel initialises the outputs by nm x topk (hs_pssm_topk_fill_kernel
// runs only for a call that ran no batch).  All stores are vector stores.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_pssm_topk.h"

namespace {

typedef unsigned long long u64;

constexpr int SAMPLE_WAVES = 4;
constexpr double NO_FLOOR = -1.7976931348623157e308;  // -DBL_MAX: hs_pssm_finish passes everything below -2^108

inline unsigned pt_blocks(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

// ---- compare-exchange steps (hs_knn.hip's, restated: on one 64-bit key, and on (key, id)) ----------------------
__device__ __forceinline__ void pt_cx1(u64& d, int j, bool keep_min) {
  const u64 od = __shfl_xor(d, j, 64);
  if ((od < d) == keep_min) d = od;
}
__device__ __forceinline__ void pt_sort1(u64& d, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) pt_cx1(d, j, ((lane & j) == 0) == ((lane & k) == 0));
  }
}
// best, other: ascending lists of 64, one entry per lane -> the 64 smallest of both, ascending
__device__ __forceinline__ u64 pt_merge1(u64 best, u64 other, int lane) {
  const u64 r = __shfl(other, 63 - lane, 64);
  u64 d = best < r ? best : r;
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) pt_cx1(d, j, (lane & j) == 0);
  return d;
}

__device__ __forceinline__ bool pt_less(u64 d0, u64 w0, u64 d1, u64 w1) { return d0 < d1 || (d0 == d1 && w0 < w1); }
__device__ __forceinline__ void pt_cx2(u64& d, u64& w, int j, bool keep_min) {
  const u64 od = __shfl_xor(d, j, 64), ow = __shfl_xor(w, j, 64);
  const bool other_less = pt_less(od, ow, d, w);
  if (other_less == keep_min) {  // (equal keys -- two paddings -- stay where they are on both sides)
    d = od;
    w = ow;
  }
}

// ------------------------------------------------------------------------------------ 1. the sample pass
// t_used[m] from the list's topk-th entry (the caller is the lane that holds it)
__device__ __forceinline__ void pt_write_t_used(u64 best, const double* __restrict__ floor_t, uint32_t m,
                                                double* __restrict__ t_used) {
  const double fl = floor_t ? floor_t[m] : NO_FLOOR;
  double t = fl;
  if (best != HS_PSSM_TOPK_PAD) {
    const double ts = __longlong_as_double((long long)hs_pssm_desc_bits(best));
    if (ts > fl) t = ts;
  }
  t_used[m] = t;
}

// S, floor (may be null), t_used: the BATCH's profiles; `parts` workgroups per profile, workgroup m * parts + part
// over the samples [part * chunk, (part + 1) * chunk).  parts == 1: t_used is written here; else the workgroup's
// list goes to part_lists [mb * parts][64]
__global__ __launch_bounds__(64 * SAMPLE_WAVES) void hs_pssm_sample_kernel(const uint8_t* __restrict__ codes,
                                                                          const double* __restrict__ S,
                                                                          const double* __restrict__ floor_t, int k,
                                                                          int alphabet, uint32_t n, uint32_t n_s,
                                                                          uint32_t topk, uint32_t parts, uint32_t chunk,
                                                                          u64* __restrict__ part_lists,
                                                                          double* __restrict__ t_used) {
  extern __shared__ double s_lds[];  // the profile's [k][alphabet]
  __shared__ u64 lists[SAMPLE_WAVES][64];
  const uint32_t m = blockIdx.x / parts, part = blockIdx.x - m * parts;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ka = k * alphabet;
  const double* const Sm = S + (uint64_t)m * ka;
  for (int e = tid; e < ka; e += 64 * SAMPLE_WAVES) s_lds[e] = Sm[e];
  __syncthreads();

  u64 best = HS_PSSM_TOPK_PAD;
  const uint64_t j_lo = (uint64_t)part * chunk, j_hi = j_lo + chunk < n_s ? j_lo + chunk : (uint64_t)n_s;
  for (uint64_t j0 = j_lo + (uint64_t)wave * 64u; j0 < j_hi; j0 += 64u * SAMPLE_WAVES) {  // (wave-uniform)
    const uint64_t j = j0 + (uint32_t)lane;
    u64 key = HS_PSSM_TOPK_PAD;
    if (j < j_hi) {
      const uint64_t id = j * n / n_s;  // < n
      const uint8_t* const x = codes + id * (uint64_t)k;
      double sc = 0.0;
      for (int p = 0; p < k; ++p) sc = sc + s_lds[p * alphabet + x[p]];
      key = hs_pssm_desc_key((u64)__double_as_longlong(sc));
    }
    // the list's topk-th entry: a chunk with nothing above it cannot change that entry
    const u64 tk = __shfl(best, (int)topk - 1, 64);
    if (!__ballot(key < tk)) continue;
    pt_sort1(key, lane);
    best = pt_merge1(best, key, lane);
  }
  lists[wave][lane] = best;
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 1; w < SAMPLE_WAVES; ++w) best = pt_merge1(best, lists[w][lane], lane);
  if (parts > 1)
    part_lists[(uint64_t)blockIdx.x * 64u + (uint32_t)lane] = best;
  else if (lane == (int)topk - 1)
    pt_write_t_used(best, floor_t, m, t_used);
}

// 4 waves per block, one profile per wave: the profile's `parts` ascending lists merged, t_used written
__global__ __launch_bounds__(256) void hs_pssm_sample_merge_kernel(const u64* __restrict__ part_lists, uint32_t mb,
                                                                   uint32_t parts, uint32_t topk,
                                                                   const double* __restrict__ floor_t,
                                                                   double* __restrict__ t_used) {
  const uint32_t m = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (m >= mb) return;  // (a whole wave)
  const int lane = (int)(threadIdx.x & 63u);
  u64 best = HS_PSSM_TOPK_PAD;
  for (uint32_t p = 0; p < parts; ++p)
    best = pt_merge1(best, part_lists[((uint64_t)m * parts + p) * 64u + (uint32_t)lane], lane);
  if (lane == (int)topk - 1) pt_write_t_used(best, floor_t, m, t_used);
}

// ------------------------------------------------------------------------------------ 3. the selection
__global__ __launch_bounds__(256) void hs_pssm_topk_count_kernel(const uint64_t* __restrict__ key, uint32_t nh,
                                                                 uint32_t first, uint32_t count,
                                                                 uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nh) return;
  const uint32_t q = (uint32_t)(key[i] >> 32) - first;  // (unsigned: below the range wraps above it)
  if (q < count) atomicAdd(cnt + q, 1u);
}

__global__ __launch_bounds__(256) void hs_pssm_topk_cursor_kernel(const uint32_t* __restrict__ off, uint32_t count,
                                                                  uint32_t* __restrict__ cur) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < count) cur[t] = off[t];
}

__global__ __launch_bounds__(256) void hs_pssm_topk_scatter_kernel(const uint64_t* __restrict__ key,
                                                                   const uint64_t* __restrict__ val, uint32_t nh,
                                                                   uint32_t first, uint32_t count,
                                                                   uint32_t* __restrict__ cur, u64* __restrict__ seg_d,
                                                                   u64* __restrict__ seg_w) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nh) return;
  const uint64_t kk = key[i];
  const uint32_t q = (uint32_t)(kk >> 32) - first;
  if (q >= count) return;
  const uint32_t pos = atomicAdd(cur + q, 1u);
  // (the count pass saw the same hits, so pos stays inside the profile's segment; the compare keeps a store inside
  // the two arrays whatever the buffers hold)
  if (pos < nh) {
    seg_d[pos] = hs_pssm_desc_key(val[i]);
    seg_w[pos] = (u64)(uint32_t)kk;
  }
}

// 4 waves per block, one profile per wave.  floor_t (may be null), t_used: the batch's; top_*: the call's rows
__global__ __launch_bounds__(256) void hs_pssm_topk_select_kernel(const u64* __restrict__ seg_d,
                                                                  const u64* __restrict__ seg_w,
                                                                  const uint32_t* __restrict__ off, uint32_t count,
                                                                  uint32_t topk, uint64_t row0,
                                                                  const double* __restrict__ floor_t,
                                                                  const double* __restrict__ t_used,
                                                                  uint32_t* __restrict__ top_id,
                                                                  double* __restrict__ top_score,
                                                                  uint32_t* __restrict__ top_count,
                                                                  u64* __restrict__ raised) {
  const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (t >= count) return;  // (a whole wave: t is wave-uniform)
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t lo = off[t], hi = off[t + 1];
  u64 bd = HS_PSSM_TOPK_PAD, bw = HS_PSSM_TOPK_PAD;
  for (uint32_t base = lo; base < hi; base += 64u) {
    u64 d = HS_PSSM_TOPK_PAD, w = HS_PSSM_TOPK_PAD;
    if (base + (uint32_t)lane < hi) {
      d = seg_d[base + lane];
      w = seg_w[base + lane];
    }
    const u64 td = __shfl(bd, (int)topk - 1, 64), tw = __shfl(bw, (int)topk - 1, 64);
    if (!__ballot(pt_less(d, w, td, tw))) continue;
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) pt_cx2(d, w, j, ((lane & j) == 0) == ((lane & k) == 0));
    }
    if (base != lo) {
      // lower half of the two ascending lists: min(best[i], chunk[63 - i]) is bitonic and holds the 64 smallest
      const u64 rd = __shfl(d, 63 - lane, 64), rw = __shfl(w, 63 - lane, 64);
      if (pt_less(bd, bw, rd, rw)) {
        d = bd;
        w = bw;
      } else {
        d = rd;
        w = rw;
      }
#pragma unroll
      for (int j = 32; j > 0; j >>= 1) pt_cx2(d, w, j, (lane & j) == 0);
    }
    bd = d;
    bw = w;
  }
  const uint64_t row = row0 + t;
  if ((uint32_t)lane < topk) {
    const bool pad = bd == HS_PSSM_TOPK_PAD;
    const uint64_t at = row * topk + (uint32_t)lane;
    top_id[at] = pad ? 0xffffffffu : (uint32_t)bw;
    top_score[at] = pad ? -INFINITY : __longlong_as_double((long long)hs_pssm_desc_bits(bd));
  }
  if (lane == 0) {
    top_count[row] = hi - lo < topk ? hi - lo : topk;
    if (t_used[t] > (floor_t ? floor_t[t] : NO_FLOOR)) atomicAdd(raised, 1ull);
  }
}

// rows of padding, zero counts and t_used = the floor (a call that ran no batch)
__global__ __launch_bounds__(256) void hs_pssm_topk_fill_kernel(uint64_t rows, uint32_t topk,
                                                                const double* __restrict__ floor_t,
                                                                uint32_t* __restrict__ top_id,
                                                                double* __restrict__ top_score,
                                                                uint32_t* __restrict__ top_count,
                                                                double* __restrict__ t_used) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < rows * topk) {
    top_id[i] = 0xffffffffu;
    top_score[i] = -INFINITY;
  }
  if (i < rows) {
    top_count[i] = 0u;
    if (t_used) t_used[i] = floor_t ? floor_t[i] : NO_FLOOR;
  }
}

}  // namespace

size_t hs_pssm_topk_temp(uint32_t count) { return hs_scan_u32_temp((size_t)count + 1); }

// workgroups per profile: about 1024 workgroups in all, none with fewer than 1024 samples
uint32_t hs_pssm_sample_parts(uint32_t mb, uint32_t n_s) {
  if (!mb) return 1;
  const uint32_t want = (1024u + mb - 1) / mb, room = (n_s + 1023u) / 1024u;
  return std::max(1u, std::min(want, room));
}
size_t hs_pssm_sample_part_bytes(uint32_t mb, uint32_t n_s) {
  const uint32_t parts = hs_pssm_sample_parts(mb, n_s);
  return parts > 1 ? (size_t)mb * parts * 64 * 8 : 0;
}

hipError_t hs_launch_pssm_sample(const uint8_t* d_codes, const double* d_S, const double* d_floor, int k, int alphabet,
                                 uint32_t n, uint32_t n_s, uint32_t topk, uint32_t mb, void* d_part_lists,
                                 double* d_t_used, hipStream_t s) {
  if (!mb) return hipSuccess;
  const size_t shmem = (size_t)k * alphabet * 8;  // at most 75 * 32 * 8 = 19 200 bytes
  const uint32_t parts = hs_pssm_sample_parts(mb, n_s);
  // a part's samples: a multiple of the workgroup's 256 (the last part may be short, or empty)
  const uint32_t chunk = (uint32_t)((((uint64_t)n_s + parts - 1) / parts + 255u) & ~(uint64_t)255u);
  u64* const lists = reinterpret_cast<u64*>(d_part_lists);
  hs_pssm_sample_kernel<<<mb * parts, 64 * SAMPLE_WAVES, shmem, s>>>(d_codes, d_S, d_floor, k, alphabet, n, n_s, topk,
                                                                     parts, chunk, lists, d_t_used);
  if (parts > 1)
    hs_pssm_sample_merge_kernel<<<(mb + 3u) / 4u, 256, 0, s>>>(lists, mb, parts, topk, d_floor, d_t_used);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_topk_select(const uint64_t* d_key, const uint64_t* d_val, uint32_t nh, uint32_t first,
                                      uint32_t count, uint32_t* d_cnt, uint32_t* d_off, uint32_t* d_cur, void* d_temp,
                                      size_t temp_bytes, uint64_t* d_seg_d, uint64_t* d_seg_w, uint32_t topk,
                                      const double* d_floor, const double* d_t_used, uint32_t* d_top_id,
                                      double* d_top_score, uint32_t* d_top_count, uint64_t* d_raised, hipStream_t s) {
  if (!count) return hipSuccess;
  hipError_t e = hipMemsetAsync(d_cnt, 0, ((size_t)count + 1) * 4, s);
  if (e != hipSuccess) return e;
  if (nh) hs_pssm_topk_count_kernel<<<pt_blocks(nh), 256, 0, s>>>(d_key, nh, first, count, d_cnt);
  e = hs_exclusive_scan_u32(d_temp, temp_bytes, d_cnt, d_off, (size_t)count + 1, s);
  if (e != hipSuccess) return e;
  hs_pssm_topk_cursor_kernel<<<pt_blocks(count), 256, 0, s>>>(d_off, count, d_cur);
  if (nh)
    hs_pssm_topk_scatter_kernel<<<pt_blocks(nh), 256, 0, s>>>(d_key, d_val, nh, first, count, d_cur,
                                                             reinterpret_cast<u64*>(d_seg_d),
                                                             reinterpret_cast<u64*>(d_seg_w));
  hs_pssm_topk_select_kernel<<<(count + 3u) / 4u, 256, 0, s>>>(
      reinterpret_cast<const u64*>(d_seg_d), reinterpret_cast<const u64*>(d_seg_w), d_off, count, topk, first, d_floor,
      d_t_used, d_top_id, d_top_score, d_top_count, reinterpret_cast<u64*>(d_raised));
  return hipGetLastError();
}

hipError_t hs_launch_pssm_topk_fill(uint64_t rows, uint32_t topk, const double* d_floor, uint32_t* d_top_id,
                                    double* d_top_score, uint32_t* d_top_count, double* d_t_used, hipStream_t s) {
  if (!rows) return hipSuccess;
  hs_pssm_topk_fill_kernel<<<pt_blocks(rows * topk), 256, 0, s>>>(rows, topk, d_floor, d_top_id, d_top_score,
                                                                 d_top_count, d_t_used);
  return hipGetLastError();
}

// ---- the same rule on the host for any list of tuples (no GPU, no handle) ------------------------------
extern "C" hs_status hs_pssm_topk_hits(const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                       uint64_t nm, uint32_t topk, uint32_t* top_id, double* top_score,
                                       uint32_t* top_count) {
  const int r = hs_pssm_topk_hits_host(m, id, score, n_tuples, nm, topk, HS_TOPK_MAX, top_id, top_score, top_count);
  return r == 0 ? HS_OK : r == 1 ? HS_ERR_INVALID : HS_ERR_NOMEM;
}
