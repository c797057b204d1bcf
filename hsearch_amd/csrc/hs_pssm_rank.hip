// hs_pssm_rank.hip -- hs_pssm_rank: for every profile the exact score of its rank-th best k-mer over the index
// (include/hsearch.h), and the same rule on the host (hs_pssm_rank_scores, hs_pssm_rank_plan).  The order, the sample
// rule and its constants: hs_pssm_rank.h.
//
// Why it is exact.  A scan under hs_pssm_scan's rule at ANY threshold t returns every k-mer scoring >= t.  If it
// returns at least rank[m] hits for profile m, the rank-th largest score over the index is >= t, so every k-mer at or
// above that score is among the hits: the rank-th smallest descending key of the hits is t_rank, the hits with a
// smaller key are cnt_gt, those with an equal key are cnt_ge - cnt_gt.  The sample only proposes t; the hit count
// decides, and a profile with fewer hits than its rank goes to the next round at a lower t.  The last rung of the
// ladder is -DBL_MAX, which returns all n >= rank k-mers.  Nothing of the sample shows in the result.
//
// A round (hs_capi_pssm.hip pssm_rank_core; the scan and the selection of a round run under its pssm_batch_loop):
//   1. the sample    hs_pssm_rank_sample_kernel has hs_pssm_sample_kernel's structure (the profile's S block in LDS,
//        sample j = k-mer floor(j * n / n_s), one exact contract score per lane from `codes`) but stores every
//        descending key to keys[profile][n_s].  The pass runs in sub-batches of profiles so that the key buffer stays
//        within 2^27 bytes (one profile's n_s keys if they alone exceed that).  The select below, segment = a profile's
//        n_s keys, rank = the plan's r_s, gives t_scan; r_s > n_s gives -DBL_MAX without a select.
//   2. the scan at t_scan     hs_pssm.hip's tables, filter and exact pass, unchanged (hs_capi_pssm.hip pssm_batch); the
//        resolved profiles ride along at +DBL_MAX, which no score reaches.
//   3. the selection          the batch's unordered hits (m << 32 | id, score bits) are counted per profile, the counts
//        scanned, the descending keys scattered by profile (the passes of hs_pssm_topk.hip restated, counting in
//        LDS bins per workgroup: a batch here holds 10^5 - 10^8 hits; and no id travels).  The select runs on the
//        profiles with at least rank hits, and hs_pssm_rank_resolve_kernel writes their outputs and counts the others.
//
// The segmented radix select (rank-th smallest of every segment of 64-bit keys; 8 passes of 8 bits, high byte first).
// The keys of all segments lie side by side, off[count + 1] cuts them.  The FLAT array is cut into work items of
// RS_ITEM keys, one per workgroup, so a segment of n keys spreads over n / RS_ITEM workgroups; an item finds its
// first segment by a search in off[] and walks the segment runs inside it, one after the other (a known cost: an item
// that holds many short segments pays a search, two barriers and a 256-thread flush per run, serially).  Per run: the
// keys that match the segment's prefix so far are counted by digit in wave-private LDS histograms (a wave whose keys share the digit -- the exponent bytes, a constant profile -- adds one popcount from
// one lane after a ballot), the four histograms are summed, and the non-zero bins go to the segment's global histogram
// with integer atomics.  hs_pssm_rank_pick_kernel, one wave per segment, finds the bin that holds the remaining rank,
// extends the prefix, subtracts the keys passed over, adds them to the segment's `gt`, notes the bin's count and
// clears the histogram.  Prefix, remaining rank and counts stay on the device; after the low byte the prefix is the
// key, gt the keys before it, eq the keys equal to it.  Integer atomics only: the result does not depend on the order
// of anything.  A segment with remaining rank 0 is not selected from (its runs are skipped).
// Chosen: 8-bit digits (256 bins = one per thread of the workgroup, the flush is one compare and at most one atomic per
// thread).  No short-segment fast path and no bitonic finish: in a kernel trace of two hit-heavy calls (DESIGN.md
// section 25) the passes of both selects took 0.18 ms of an 18 ms call and 0.70 ms of a 170 ms one.  What did cost was
// the count and the scatter in front of the select at one global atomic per hit; they now count in LDS bins (below).
// All stores are vector stores.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_pssm_rank.h"

namespace {

typedef unsigned long long u64;

constexpr uint32_t RS_ITEM = 4096;          // keys per work item of the select's histogram pass
constexpr uint32_t RS_BINS = 4096;          // profiles of a batch the LDS-binned count / scatter passes take
constexpr uint32_t RS_HITS = 4096;          // hits per workgroup of those passes
constexpr uint32_t RS_SAMPLE_CHUNK = 4096;  // samples per workgroup of the sample pass
constexpr double RS_ALL = -1.7976931348623157e308;   // -DBL_MAX: every k-mer hits
constexpr double RS_NONE = 1.7976931348623157e308;   // +DBL_MAX: no k-mer hits (scores stay below 2^107)

inline unsigned pr_blocks(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

// the select's state for `count` segments: prefix, remaining rank, keys passed over, keys in the last bin (u64 each),
// then the global histograms [count][256] (u32)
struct SelState {
  u64 *prefix, *rem, *gt, *eq;
  uint32_t* hist;
};
__host__ __device__ inline SelState sel_state(void* base, uint32_t count) {
  u64* const p = reinterpret_cast<u64*>(base);
  SelState s;
  s.prefix = p;
  s.rem = p + count;
  s.gt = p + 2 * (size_t)count;
  s.eq = p + 3 * (size_t)count;
  s.hist = reinterpret_cast<uint32_t*>(p + 4 * (size_t)count);
  return s;
}

// ------------------------------------------------------------------------------------ the argument check
// flag |= 4 for a rank outside 1 .. n; *max_rank = the largest rank seen
__global__ __launch_bounds__(256) void hs_pssm_rank_check_kernel(const u64* __restrict__ rank, uint64_t nm, uint64_t n,
                                                                 uint32_t* __restrict__ flag,
                                                                 u64* __restrict__ max_rank) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  u64 r = i < nm ? rank[i] : 1;  // (1: neither refused nor a maximum; n == 0 is flagged by the lanes inside)
  const bool bad = i < nm && (r < 1 || r > n);
  // one atomic per wave: the wave's maximum by a butterfly, the flag after a ballot
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const u64 o = __shfl_xor(r, d, 64);
    if (o > r) r = o;
  }
  const bool any_bad = __ballot(bad) != 0;
  if ((threadIdx.x & 63u) == 0) {
    if (any_bad) atomicOr(flag, 4u);
    atomicMax(max_rank, r);
  }
}

// every profile unresolved (the flags of a call)
__global__ __launch_bounds__(256) void hs_pssm_rank_init_kernel(uint64_t nm, uint32_t* __restrict__ resolved,
                                                                uint32_t* __restrict__ unresolved_count) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < nm) resolved[i] = 0u;
  if (i == 0) *unresolved_count = 0u;
}

// ------------------------------------------------------------------------------------ 1. the sample pass
// S, resolved: the SUB-BATCH's profiles; workgroup m * parts + part scores the samples [part * RS_SAMPLE_CHUNK, ...)
// of profile m and stores their descending keys to keys[m * n_s + j].  A resolved profile is not scored.
__global__ __launch_bounds__(256) void hs_pssm_rank_sample_kernel(const uint8_t* __restrict__ codes,
                                                                  const double* __restrict__ S,
                                                                  const uint32_t* __restrict__ resolved, int k,
                                                                  int alphabet, uint32_t n, uint32_t n_s, uint32_t parts,
                                                                  u64* __restrict__ keys) {
  extern __shared__ double s_lds[];  // the profile's [k][alphabet]
  const uint32_t m = blockIdx.x / parts, part = blockIdx.x - m * parts;
  if (resolved[m]) return;  // (the whole workgroup)
  const int tid = (int)threadIdx.x;
  const int ka = k * alphabet;
  const double* const Sm = S + (uint64_t)m * ka;
  for (int e = tid; e < ka; e += 256) s_lds[e] = Sm[e];
  __syncthreads();
  const uint64_t j_lo = (uint64_t)part * RS_SAMPLE_CHUNK;
  const uint64_t j_hi = j_lo + RS_SAMPLE_CHUNK < n_s ? j_lo + RS_SAMPLE_CHUNK : (uint64_t)n_s;
  u64* const row = keys + (uint64_t)m * n_s;
  for (uint64_t j = j_lo + (uint32_t)tid; j < j_hi; j += 256u) {
    const uint64_t id = j * n / n_s;  // < n (j < n_s <= n: the product stays below 2^64)
    const uint8_t* const x = codes + id * (uint64_t)k;
    double sc = 0.0;
    for (int p = 0; p < k; ++p) sc = sc + s_lds[p * alphabet + x[p]];
    row[j] = hs_pssm_desc_key((u64)__double_as_longlong(sc));
  }
}

// off[i] = i * n_s: the segments of a sub-batch's key buffer
__global__ __launch_bounds__(256) void hs_pssm_rank_segoff_kernel(uint32_t count, uint32_t n_s,
                                                                  uint32_t* __restrict__ off) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i <= count) off[i] = i * n_s;  // (count * n_s < 2^32: the driver sizes the sub-batch)
}

// The select's start for the sample of profiles m0 .. m0 + count - 1: remaining rank = the plan's r_s, or 0 (no
// select) for a resolved profile and for r_s beyond the sample
__global__ __launch_bounds__(256) void hs_pssm_rank_sample_plan_kernel(const u64* __restrict__ rank,
                                                                       const uint32_t* __restrict__ resolved,
                                                                       uint32_t m0, uint32_t count, uint64_t n,
                                                                       uint64_t n_s, uint32_t round, void* state) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= count) return;
  const SelState st = sel_state(state, count);
  uint64_t r_s = 0;
  if (resolved[m0 + s] || hs_pssm_rank_plan_rule(rank[m0 + s], n, n_s, round, &r_s) || r_s > n_s) r_s = 0;
  st.prefix[s] = 0;
  st.rem[s] = r_s;
  st.gt[s] = 0;
  st.eq[s] = 0;
}

// t_scan of the round for profiles m0 .. m0 + count - 1 from the sample's select
__global__ __launch_bounds__(256) void hs_pssm_rank_tscan_kernel(const u64* __restrict__ rank,
                                                                 const uint32_t* __restrict__ resolved, uint32_t m0,
                                                                 uint32_t count, uint64_t n, uint64_t n_s,
                                                                 uint32_t round, const void* state,
                                                                 double* __restrict__ t_scan,
                                                                 double* __restrict__ t_scan_out) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= count) return;
  const uint32_t m = m0 + s;
  if (resolved[m]) {
    t_scan[m] = RS_NONE;
    return;
  }
  const SelState st = sel_state(const_cast<void*>(state), count);
  uint64_t r_s = 0;
  double t = RS_ALL;
  if (!hs_pssm_rank_plan_rule(rank[m], n, n_s, round, &r_s) && r_s <= n_s)
    t = __longlong_as_double((long long)hs_pssm_desc_bits(st.prefix[s]));
  t_scan[m] = t;
  if (t_scan_out) t_scan_out[m] = t;
}

// ------------------------------------------------------------------------------------ the segmented radix select
// the segment of flat position pos: the largest s < count with off[s] <= pos (off[0] == 0; empty segments share an
// offset, and the largest is the one whose end lies beyond pos)
__device__ __forceinline__ uint32_t rs_segment_of(const uint32_t* __restrict__ off, uint32_t count, uint32_t pos) {
  uint32_t lo = 0, hi = count;  // off[lo] <= pos; the answer is in [lo, hi)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= pos)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// One pass: workgroup b counts the digit `pass` (0: the high byte) of the keys [b * RS_ITEM, (b + 1) * RS_ITEM) that
// match their segment's prefix in the bytes above it.
__global__ __launch_bounds__(256) void hs_pssm_rank_hist_kernel(const u64* __restrict__ keys, uint32_t total,
                                                                const uint32_t* __restrict__ off, uint32_t count,
                                                                int pass, void* state) {
  __shared__ uint32_t h[4][256];
  const SelState st = sel_state(state, count);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t all = off[count] < total ? off[count] : total;  // (they agree; the compare keeps the loads inside)
  const uint64_t lo64 = (uint64_t)blockIdx.x * RS_ITEM;
  if (lo64 >= all) return;  // (the whole workgroup)
  const uint32_t lo = (uint32_t)lo64, hi = lo64 + RS_ITEM < all ? (uint32_t)(lo64 + RS_ITEM) : all;
  const int shift = 56 - 8 * pass;
  const u64 above = pass ? ~0ull << (shift + 8) : 0ull;  // the bytes the prefix has fixed
#pragma unroll
  for (int w = 0; w < 4; ++w) h[w][tid] = 0u;
  __syncthreads();
  uint32_t pos = lo;
  while (pos < hi) {  // (workgroup-uniform)
    const uint32_t seg = rs_segment_of(off, count, pos);
    const uint32_t seg_end = off[seg + 1];
    // (off ascends, so seg_end > pos; the compare ends the walk whatever off holds)
    const uint32_t end = seg_end > pos ? (seg_end < hi ? seg_end : hi) : hi;
    if (st.rem[seg] != 0) {
      const u64 prefix = st.prefix[seg];
      for (uint32_t base = pos + (uint32_t)wave * 64u; base < end; base += 256u) {  // (wave-uniform)
        const uint32_t i = base + (uint32_t)lane;
        bool act = false;
        uint32_t digit = 0;
        if (i < end) {
          const u64 key = keys[i];
          act = ((key ^ prefix) & above) == 0;
          digit = (uint32_t)(key >> shift) & 255u;
        }
        const u64 live = __ballot(act);
        if (live) {
          const int leader = __ffsll((long long)live) - 1;
          const uint32_t d0 = (uint32_t)__shfl((int)digit, leader, 64);
          const u64 same = __ballot(act && digit == d0);
          if (lane == leader)
            atomicAdd(&h[wave][d0], (uint32_t)__popcll(same));
          else if (act && digit != d0)
            atomicAdd(&h[wave][digit], 1u);
        }
      }
      __syncthreads();
      const uint32_t c = h[0][tid] + h[1][tid] + h[2][tid] + h[3][tid];
      if (c) {
        atomicAdd(st.hist + (size_t)seg * 256u + (uint32_t)tid, c);
#pragma unroll
        for (int w = 0; w < 4; ++w) h[w][tid] = 0u;
      }
      __syncthreads();
    }
    pos = end;
  }
}

// 4 waves per block, one segment per wave: the bin of the remaining rank, the state's update, the histogram cleared
__global__ __launch_bounds__(256) void hs_pssm_rank_pick_kernel(uint32_t count, int pass, void* state) {
  const uint32_t seg = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (seg >= count) return;  // (a whole wave)
  const SelState st = sel_state(state, count);
  const int lane = (int)(threadIdx.x & 63u);
  uint4* const bins = reinterpret_cast<uint4*>(st.hist + (size_t)seg * 256u) + lane;
  const uint4 c = *bins;
  const u64 r = st.rem[seg];
  if (r == 0) return;  // (wave-uniform: no select for this segment; nothing was added to its histogram)
  *bins = make_uint4(0u, 0u, 0u, 0u);
  const u64 mine = (u64)c.x + c.y + c.z + c.w;
  u64 incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  u64 before = incl - mine;
  if (before < r && r <= incl) {  // (one lane, as 1 <= r <= the matching keys)
    uint32_t b = 4u * (uint32_t)lane, cb = c.x;
    if (before + cb < r) {
      before += cb;
      ++b;
      cb = c.y;
      if (before + cb < r) {
        before += cb;
        ++b;
        cb = c.z;
        if (before + cb < r) {
          before += cb;
          ++b;
          cb = c.w;
        }
      }
    }
    const int shift = 56 - 8 * pass;
    st.prefix[seg] = st.prefix[seg] | ((u64)b << shift);
    st.rem[seg] = r - before;
    st.gt[seg] = st.gt[seg] + before;
    st.eq[seg] = cb;
  }
}

// ------------------------------------------------------------------------------------ 3. the selection over the hits
// (hs_pssm_topk.hip's count / cursor / scatter, restated; only the descending key travels.  These two take the batches
// of more than RS_BINS profiles, which only HS_OPT_QUERY_BATCH makes; the binned forms below take the others)
__global__ __launch_bounds__(256) void hs_pssm_rank_count_kernel(const uint64_t* __restrict__ key, uint32_t nh,
                                                                 uint32_t first, uint32_t count,
                                                                 uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nh) return;
  const uint32_t q = (uint32_t)(key[i] >> 32) - first;  // (unsigned: below the range wraps above it)
  if (q < count) atomicAdd(cnt + q, 1u);
}

__global__ __launch_bounds__(256) void hs_pssm_rank_cursor_kernel(const uint32_t* __restrict__ off, uint32_t count,
                                                                  uint32_t* __restrict__ cur) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < count) cur[t] = off[t];
}

__global__ __launch_bounds__(256) void hs_pssm_rank_scatter_kernel(const uint64_t* __restrict__ key,
                                                                   const uint64_t* __restrict__ val, uint32_t nh,
                                                                   uint32_t first, uint32_t count,
                                                                   uint32_t* __restrict__ cur, u64* __restrict__ seg_d) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nh) return;
  const uint32_t q = (uint32_t)(key[i] >> 32) - first;
  if (q >= count) return;
  const uint32_t pos = atomicAdd(cur + q, 1u);
  // (the count pass saw the same hits, so pos stays inside the profile's segment; the compare keeps the store inside
  // the array whatever the buffers hold)
  if (pos < nh) seg_d[pos] = hs_pssm_desc_key(val[i]);
}

// The same two passes for batches of at most RS_BINS profiles, which is every batch unless HS_OPT_QUERY_BATCH says more.
// A batch near a rank's threshold holds 10^5 - 10^8 hits of as few as 16 profiles, and one global atomic per hit on 16
// addresses serialises in the L2 (measured: 4.9 ms each for count and scatter at 1.9 x 10^6 hits of 16 profiles, beside
// an exact pass of 0.85 ms).  Here a workgroup takes RS_HITS hits and counts them in LDS bins, one per profile; a wave
// whose hits share the profile adds one popcount from one lane.  Count: the non-zero bins go to the global counts, one
// atomic per (workgroup, profile present).  Scatter: every non-zero bin reserves that many slots of its profile's
// segment with one global atomic, and the hits take their slots from the bin by LDS atomics.  The order of a
// segment's keys depends on scheduling; the select does not look at it.
__device__ __forceinline__ void rs_bin_hits(const uint64_t* __restrict__ key, uint32_t lo, uint32_t hi, uint32_t first,
                                            uint32_t count, uint32_t* bins, int lane, int wave) {
  for (uint32_t base = lo + (uint32_t)wave * 64u; base < hi; base += 256u) {  // (wave-uniform)
    const uint32_t i = base + (uint32_t)lane;
    const uint32_t q = i < hi ? (uint32_t)(key[i] >> 32) - first : 0xffffffffu;  // (unsigned: below the range wraps)
    const bool act = q < count;
    const u64 live = __ballot(act);
    if (!live) continue;
    const int leader = __ffsll((long long)live) - 1;
    const uint32_t q0 = (uint32_t)__shfl((int)q, leader, 64);
    const u64 same = __ballot(act && q == q0);
    if (lane == leader)
      atomicAdd(&bins[q0], (uint32_t)__popcll(same));
    else if (act && q != q0)
      atomicAdd(&bins[q], 1u);
  }
}

__global__ __launch_bounds__(256) void hs_pssm_rank_count_lds_kernel(const uint64_t* __restrict__ key, uint32_t nh,
                                                                     uint32_t first, uint32_t count,
                                                                     uint32_t* __restrict__ cnt) {
  __shared__ uint32_t bins[RS_BINS];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t lo64 = (uint64_t)blockIdx.x * RS_HITS;
  if (lo64 >= nh || count > RS_BINS) return;  // (the whole workgroup)
  const uint32_t lo = (uint32_t)lo64, hi = lo64 + RS_HITS < nh ? (uint32_t)(lo64 + RS_HITS) : nh;
  for (uint32_t b = (uint32_t)tid; b < count; b += 256u) bins[b] = 0u;
  __syncthreads();
  rs_bin_hits(key, lo, hi, first, count, bins, lane, wave);
  __syncthreads();
  for (uint32_t b = (uint32_t)tid; b < count; b += 256u) {
    const uint32_t c = bins[b];
    if (c) atomicAdd(cnt + b, c);
  }
}

__global__ __launch_bounds__(256) void hs_pssm_rank_scatter_lds_kernel(const uint64_t* __restrict__ key,
                                                                       const uint64_t* __restrict__ val, uint32_t nh,
                                                                       uint32_t first, uint32_t count,
                                                                       uint32_t* __restrict__ cur,
                                                                       u64* __restrict__ seg_d) {
  __shared__ uint32_t bins[RS_BINS];  // the workgroup's hits per profile; then the next free slot of its reservation
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t lo64 = (uint64_t)blockIdx.x * RS_HITS;
  if (lo64 >= nh || count > RS_BINS) return;  // (the whole workgroup)
  const uint32_t lo = (uint32_t)lo64, hi = lo64 + RS_HITS < nh ? (uint32_t)(lo64 + RS_HITS) : nh;
  for (uint32_t b = (uint32_t)tid; b < count; b += 256u) bins[b] = 0u;
  __syncthreads();
  rs_bin_hits(key, lo, hi, first, count, bins, lane, wave);
  __syncthreads();
  for (uint32_t b = (uint32_t)tid; b < count; b += 256u) {
    const uint32_t c = bins[b];
    if (c) bins[b] = atomicAdd(cur + b, c);
  }
  __syncthreads();
  for (uint32_t base = lo + (uint32_t)wave * 64u; base < hi; base += 256u) {  // (wave-uniform)
    const uint32_t i = base + (uint32_t)lane;
    const uint32_t q = i < hi ? (uint32_t)(key[i] >> 32) - first : 0xffffffffu;
    const bool act = q < count;
    const u64 live = __ballot(act);
    if (!live) continue;
    const int leader = __ffsll((long long)live) - 1;
    const uint32_t q0 = (uint32_t)__shfl((int)q, leader, 64);
    const u64 same = __ballot(act && q == q0);
    uint32_t pos = 0;
    if (lane == leader) pos = atomicAdd(&bins[q0], (uint32_t)__popcll(same));
    pos = (uint32_t)__shfl((int)pos, leader, 64);
    if (act && q == q0)
      pos += (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    else if (act)
      pos = atomicAdd(&bins[q], 1u);
    // (the count pass saw the same hits, so pos stays inside the profile's segment; the compare keeps the store inside
    // the array whatever the buffers hold)
    if (act && pos < nh) seg_d[pos] = hs_pssm_desc_key(val[i]);
  }
}

// The select's start for the hits of profiles m0 .. m0 + count - 1: remaining rank = rank[m] where the profile is
// unresolved and has at least that many hits, else 0 (no select)
__global__ __launch_bounds__(256) void hs_pssm_rank_hits_plan_kernel(const u64* __restrict__ rank,
                                                                     const uint32_t* __restrict__ resolved,
                                                                     const uint32_t* __restrict__ off, uint32_t m0,
                                                                     uint32_t count, void* state) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= count) return;
  const SelState st = sel_state(state, count);
  const u64 r = rank[m0 + t], len = off[t + 1] - off[t];
  st.prefix[t] = 0;
  st.rem[t] = (!resolved[m0 + t] && r >= 1 && len >= r) ? r : 0;
  st.gt[t] = 0;
  st.eq[t] = 0;
}

// The resolve step: the profiles the select ran for get their outputs and are resolved; the other unresolved ones are
// counted for the next round
__global__ __launch_bounds__(256) void hs_pssm_rank_resolve_kernel(const u64* __restrict__ rank,
                                                                   uint32_t* __restrict__ resolved,
                                                                   const uint32_t* __restrict__ off, uint32_t m0,
                                                                   uint32_t count, uint32_t round, const void* state,
                                                                   double* __restrict__ t_rank, u64* __restrict__ cnt_ge,
                                                                   u64* __restrict__ cnt_gt,
                                                                   uint32_t* __restrict__ rounds_out,
                                                                   uint32_t* __restrict__ unresolved_count) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= count) return;
  const uint32_t m = m0 + t;
  if (resolved[m]) return;
  const SelState st = sel_state(const_cast<void*>(state), count);
  const u64 r = rank[m], len = off[t + 1] - off[t];
  if (r >= 1 && len >= r) {
    t_rank[m] = __longlong_as_double((long long)hs_pssm_desc_bits(st.prefix[t]));
    cnt_gt[m] = st.gt[t];
    cnt_ge[m] = st.gt[t] + st.eq[t];
    if (rounds_out) rounds_out[m] = round;
    resolved[m] = 1u;
  } else {
    atomicAdd(unresolved_count, 1u);
  }
}

// the eight passes over `total` keys in `count` segments; the state's rem / prefix / gt / eq are set, its histograms zero
hipError_t rs_select(const u64* keys, uint32_t total, const uint32_t* off, uint32_t count, void* state, hipStream_t s) {
  if (!total || !count) return hipSuccess;
  const unsigned items = (unsigned)(((uint64_t)total + RS_ITEM - 1) / RS_ITEM);
  for (int pass = 0; pass < 8; ++pass) {
    hs_pssm_rank_hist_kernel<<<items, 256, 0, s>>>(keys, total, off, count, pass, state);
    hs_pssm_rank_pick_kernel<<<(count + 3u) / 4u, 256, 0, s>>>(count, pass, state);
  }
  return hipGetLastError();
}

}  // namespace

size_t hs_pssm_rank_state_bytes(uint32_t count) { return (size_t)count * (4 * 8 + 256 * 4) + 64; }
size_t hs_pssm_rank_temp(uint32_t count) { return hs_scan_u32_temp((size_t)count + 1); }

hipError_t hs_launch_pssm_rank_check(const uint64_t* d_rank, uint64_t nm, uint64_t n, uint32_t* d_flag,
                                     uint64_t* d_max_rank, hipStream_t s) {
  if (!nm) return hipSuccess;
  hs_pssm_rank_check_kernel<<<pr_blocks(nm), 256, 0, s>>>(reinterpret_cast<const u64*>(d_rank), nm, n, d_flag,
                                                         reinterpret_cast<u64*>(d_max_rank));
  return hipGetLastError();
}

hipError_t hs_launch_pssm_rank_init(uint64_t nm, uint32_t* d_resolved, uint32_t* d_unresolved, hipStream_t s) {
  hs_pssm_rank_init_kernel<<<std::max(1u, pr_blocks(nm)), 256, 0, s>>>(nm, d_resolved, d_unresolved);
  return hipGetLastError();
}

// profiles per sub-batch of the sample pass: their keys within 2^27 bytes, at most 4096, at least one
uint32_t hs_pssm_rank_sample_batch(uint32_t n_s) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4096, (1ull << 24) / std::max(1u, n_s)));
}

// The sample pass and its select for profiles m0 .. m0 + mb - 1 of the call (d_S: the CALL's first profile; d_rank,
// d_resolved, d_t_scan, d_t_scan_out: the call's arrays; d_t_scan_out may be null).  d_keys: mb * n_s keys; d_off:
// mb + 1 words; d_state: hs_pssm_rank_state_bytes(mb).  mb * n_s < 2^32.
hipError_t hs_launch_pssm_rank_sample(const uint8_t* d_codes, const double* d_S, const uint64_t* d_rank,
                                      const uint32_t* d_resolved, int k, int alphabet, uint32_t n, uint32_t n_s,
                                      uint32_t round, uint32_t m0, uint32_t mb, uint64_t* d_keys, uint32_t* d_off,
                                      void* d_state, double* d_t_scan, double* d_t_scan_out, hipStream_t s) {
  if (!mb || !n_s) return hipSuccess;
  const u64* const rank = reinterpret_cast<const u64*>(d_rank);
  const size_t shmem = (size_t)k * alphabet * 8;  // at most 75 * 32 * 8 = 19 200 bytes
  const uint32_t parts = (n_s + RS_SAMPLE_CHUNK - 1) / RS_SAMPLE_CHUNK;
  hipError_t e = hipMemsetAsync(d_state, 0, hs_pssm_rank_state_bytes(mb), s);
  if (e != hipSuccess) return e;
  hs_pssm_rank_sample_kernel<<<mb * parts, 256, shmem, s>>>(d_codes, d_S + (size_t)m0 * k * alphabet, d_resolved + m0, k,
                                                           alphabet, n, n_s, parts, reinterpret_cast<u64*>(d_keys));
  hs_pssm_rank_segoff_kernel<<<pr_blocks((uint64_t)mb + 1), 256, 0, s>>>(mb, n_s, d_off);
  hs_pssm_rank_sample_plan_kernel<<<pr_blocks(mb), 256, 0, s>>>(rank, d_resolved, m0, mb, n, n_s, round, d_state);
  e = rs_select(reinterpret_cast<const u64*>(d_keys), mb * n_s, d_off, mb, d_state, s);
  if (e != hipSuccess) return e;
  hs_pssm_rank_tscan_kernel<<<pr_blocks(mb), 256, 0, s>>>(rank, d_resolved, m0, mb, n, n_s, round, d_state, d_t_scan,
                                                         d_t_scan_out);
  return hipGetLastError();
}

// The selection over a scanned batch's nh hits (d_key / d_val: hs_pssm_exact's lists) for profiles first .. first +
// count - 1, and the resolve step.  d_cnt, d_off, d_cur: count + 1 words each; d_seg: max(1, nh) keys; d_state:
// hs_pssm_rank_state_bytes(count).
hipError_t hs_launch_pssm_rank_select(const uint64_t* d_key, const uint64_t* d_val, uint32_t nh, uint32_t first,
                                      uint32_t count, uint32_t* d_cnt, uint32_t* d_off, uint32_t* d_cur, void* d_temp,
                                      size_t temp_bytes, uint64_t* d_seg, void* d_state, const uint64_t* d_rank,
                                      uint32_t* d_resolved, uint32_t round, double* d_t_rank, uint64_t* d_cnt_ge,
                                      uint64_t* d_cnt_gt, uint32_t* d_rounds, uint32_t* d_unresolved, hipStream_t s) {
  if (!count) return hipSuccess;
  const u64* const rank = reinterpret_cast<const u64*>(d_rank);
  hipError_t e = hipMemsetAsync(d_cnt, 0, ((size_t)count + 1) * 4, s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(d_state, 0, hs_pssm_rank_state_bytes(count), s);
  if (e != hipSuccess) return e;
  const bool binned = count <= RS_BINS;
  const unsigned chunks = (unsigned)(((uint64_t)nh + RS_HITS - 1) / RS_HITS);
  if (nh && binned) hs_pssm_rank_count_lds_kernel<<<chunks, 256, 0, s>>>(d_key, nh, first, count, d_cnt);
  if (nh && !binned) hs_pssm_rank_count_kernel<<<pr_blocks(nh), 256, 0, s>>>(d_key, nh, first, count, d_cnt);
  e = hs_exclusive_scan_u32(d_temp, temp_bytes, d_cnt, d_off, (size_t)count + 1, s);
  if (e != hipSuccess) return e;
  hs_pssm_rank_cursor_kernel<<<pr_blocks(count), 256, 0, s>>>(d_off, count, d_cur);
  if (nh && binned)
    hs_pssm_rank_scatter_lds_kernel<<<chunks, 256, 0, s>>>(d_key, d_val, nh, first, count, d_cur,
                                                          reinterpret_cast<u64*>(d_seg));
  if (nh && !binned)
    hs_pssm_rank_scatter_kernel<<<pr_blocks(nh), 256, 0, s>>>(d_key, d_val, nh, first, count, d_cur,
                                                             reinterpret_cast<u64*>(d_seg));
  hs_pssm_rank_hits_plan_kernel<<<pr_blocks(count), 256, 0, s>>>(rank, d_resolved, d_off, first, count, d_state);
  e = rs_select(reinterpret_cast<const u64*>(d_seg), nh, d_off, count, d_state, s);
  if (e != hipSuccess) return e;
  hs_pssm_rank_resolve_kernel<<<pr_blocks(count), 256, 0, s>>>(rank, d_resolved, d_off, first, count, round, d_state,
                                                              d_t_rank, reinterpret_cast<u64*>(d_cnt_ge),
                                                              reinterpret_cast<u64*>(d_cnt_gt), d_rounds, d_unresolved);
  return hipGetLastError();
}

// ---- the same rules on the host (no GPU, no handle) ---------------------------------------------------
extern "C" hs_status hs_pssm_rank_scores(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet,
                                         const double* S, uint64_t nm, const uint64_t* rank, double* t_rank,
                                         uint64_t* cnt_ge, uint64_t* cnt_gt) {
  const int r = hs_pssm_rank_scores_host(codes, n, k, alphabet, S, nm, rank, t_rank, cnt_ge, cnt_gt);
  return r == 0 ? HS_OK : r == 1 ? HS_ERR_INVALID : HS_ERR_NOMEM;
}

extern "C" hs_status hs_pssm_rank_plan(uint64_t rank, uint64_t n, uint64_t n_s, uint32_t round,
                                         uint64_t* sample_rank) {
  return hs_pssm_rank_plan_rule(rank, n, n_s, round, sample_rank) ? HS_ERR_INVALID : HS_OK;
}
