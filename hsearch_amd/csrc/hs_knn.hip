// hs_knn.hip -- the topk best hits of every query, selected on the device (hs_query_topk, hs_self_knn,
// include/hsearch.h), and the same rule on the host for any list of tuples (hs_topk_merge).
//
// The rule.  Of the hits N(q) of one query -- each id once -- the min(topk, |N(q)|) that are smallest under
// (dist, id), ascending; the rest of the row padded with id = table = 0xffffffff, dist = +inf; nn_count[q] = |N(q)|.
// Distances are >= +0 and never a NaN (the argument at the head of hs_density.hip), so their bit patterns order like
// the doubles, and ids within a query are distinct: the order is strict and total and the row is a pure function of
// the SET of hits.  Nothing below depends on the order the hits arrive in.
//
// The invariant it stands on (hs_capi.hip reduce_batch, run_query; the one hs_density.hip's core pass uses): ALL hits
// of one query lie in ONE batch, each exactly once -- a batch is a range of queries and is handed on only once it came
// through whole; a multi-probe chunk's merged list is a range of queries too.  So the selection runs per batch, over
// the batch's hit buffers while they are live, and every piece of scratch is sized by the batch:
//   cnt [count + 1] u32   hits per query of the batch's range [first, first + count)
//   off [count + 1] u32   their exclusive scan (hs_prims.hip); off[count] = the batch's hits
//   cur [count]     u32   the scatter's cursors, off to begin with
//   seg_d, seg_w [nh] u64 the hits grouped by query: distance bits, id << 32 | table (hit_key2 / hit_val2, which only
//                         a batch that sorts its hit LIST uses)
// Four passes per batch, each behind a kernel boundary:
//   1. count    one hit per lane, one atomicAdd per hit on its query's counter
//   2. scan     off = exclusive scan of cnt; cur = off, and the batch's hits added to the call's total
//   3. scatter  one hit per lane to seg[atomicAdd(cur + q, 1)]: the order inside a segment depends on scheduling
//   4. select   one wave per query: the running best list sits one entry per lane, ascending.  The segment is read 64
//               entries at a time; a chunk none of whose entries is below the list's topk-th entry is dropped after one
//               ballot; any other is sorted across the wave by the bitonic network over __shfl_xor (21
//               compare-exchange steps on the 128-bit key (distance bits, id << 32 | table): ids are distinct, so the
//               table never decides) and merged by the bitonic merge that keeps the lower half (lane i takes the
//               smaller of best[i] and chunk[63 - i], six more steps sort the result).  Then the wave writes its row
//               in full -- entries and padding -- and nn_count: no kernel initialises the outputs by rows x topk
//               (hs_knn_fill_kernel runs only for a call that ran no batch).
// The hits of the batch are never sorted as a whole: only min(topk, count) entries per query matter.
// All stores are vector stores.
#include <algorithm>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include <hip/hip_runtime.h>

#include "hs_internal.h"

namespace {

typedef unsigned long long u64;

#define KNN_PAD 0xffffffffffffffffull  // above every key: the distance bits of no double a hit carries
#define KNN_INF 0x7ff0000000000000ull

inline unsigned knn_blocks(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

struct KnnHit {
  uint32_t q;  // within the batch's range; >= count: not a hit of this batch (dropped)
  u64 d, w;
};

// hit i of a batch (key / val) or of a merged list (q, id, table, dist); a self-join's pair of a k-mer with itself
// and anything outside the range are marked dead
__device__ __forceinline__ KnnHit knn_load(const uint64_t* __restrict__ key, const uint64_t* __restrict__ val,
                                           const uint32_t* __restrict__ q, const uint32_t* __restrict__ id,
                                           const uint32_t* __restrict__ table, const double* __restrict__ dist,
                                           uint32_t i, uint32_t self_first, uint32_t first, uint32_t count) {
  KnnHit h;
  uint32_t qq, ii, tt;
  if (key) {
    const uint64_t kk = key[i];
    qq = (uint32_t)(kk >> 37);
    tt = (uint32_t)(kk >> 32) & 31u;
    ii = (uint32_t)kk;
    h.d = val[i];
  } else {
    qq = q[i];
    ii = id[i];
    tt = table[i];
    h.d = (u64)__double_as_longlong(dist[i]);
  }
  h.w = (u64)ii << 32 | tt;
  h.q = qq - first;  // (unsigned: below the range wraps above it)
  if (self_first != HS_NO_SELF && self_first + qq == ii) h.q = 0xffffffffu;
  if (h.q >= count) h.q = 0xffffffffu;
  return h;
}

__global__ __launch_bounds__(256) void hs_knn_count_kernel(const uint64_t* __restrict__ key,
                                                           const uint64_t* __restrict__ val,
                                                           const uint32_t* __restrict__ q,
                                                           const uint32_t* __restrict__ id,
                                                           const uint32_t* __restrict__ table,
                                                           const double* __restrict__ dist, uint32_t n_hits,
                                                           uint32_t self_first, uint32_t first, uint32_t count,
                                                           uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_hits) return;
  const KnnHit h = knn_load(key, val, q, id, table, dist, i, self_first, first, count);
  if (h.q != 0xffffffffu) atomicAdd(cnt + h.q, 1u);
}

// cur = off over the batch's queries; the batch's hits (off[count]) onto the call's total
__global__ __launch_bounds__(256) void hs_knn_cursor_kernel(const uint32_t* __restrict__ off, uint32_t count,
                                                            uint32_t* __restrict__ cur, u64* __restrict__ total) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < count) cur[t] = off[t];
  if (t == 0) *total += (u64)off[count];  // (one thread of one launch at a time: the launches are stream-ordered)
}

__global__ __launch_bounds__(256) void hs_knn_scatter_kernel(const uint64_t* __restrict__ key,
                                                             const uint64_t* __restrict__ val,
                                                             const uint32_t* __restrict__ q,
                                                             const uint32_t* __restrict__ id,
                                                             const uint32_t* __restrict__ table,
                                                             const double* __restrict__ dist, uint32_t n_hits,
                                                             uint32_t self_first, uint32_t first, uint32_t count,
                                                             uint32_t* __restrict__ cur, u64* __restrict__ seg_d,
                                                             u64* __restrict__ seg_w) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_hits) return;
  const KnnHit h = knn_load(key, val, q, id, table, dist, i, self_first, first, count);
  if (h.q == 0xffffffffu) return;
  const uint32_t pos = atomicAdd(cur + h.q, 1u);
  // (the count pass saw the same hits, so pos stays inside the query's segment; the compare -- no load -- keeps a
  // store inside the two arrays whatever the buffers hold)
  if (pos < n_hits) {
    seg_d[pos] = h.d;
    seg_w[pos] = h.w;
  }
}

__device__ __forceinline__ bool knn_less(u64 d0, u64 w0, u64 d1, u64 w1) { return d0 < d1 || (d0 == d1 && w0 < w1); }

// one compare-exchange step with the lane at distance j; keep_min: this lane keeps the smaller key
__device__ __forceinline__ void knn_cx(u64& d, u64& w, int j, bool keep_min) {
  const u64 od = __shfl_xor(d, j, 64), ow = __shfl_xor(w, j, 64);
  const bool other_less = knn_less(od, ow, d, w);
  if (other_less == keep_min) {  // (equal keys -- two paddings -- stay where they are on both sides)
    d = od;
    w = ow;
  }
}

// 4 waves per block, one query per wave
__global__ __launch_bounds__(256) void hs_knn_select_kernel(const u64* __restrict__ seg_d, const u64* __restrict__ seg_w,
                                                            const uint32_t* __restrict__ off, uint32_t count,
                                                            uint32_t topk, uint64_t row0, uint32_t* __restrict__ nn_id,
                                                            uint32_t* __restrict__ nn_table, double* __restrict__ nn_dist,
                                                            uint32_t* __restrict__ nn_count) {
  const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (t >= count) return;  // (a whole wave: t is wave-uniform)
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t lo = off[t], hi = off[t + 1];
  u64 bd = KNN_PAD, bw = KNN_PAD;
  for (uint32_t base = lo; base < hi; base += 64u) {
    u64 d = KNN_PAD, w = KNN_PAD;
    if (base + (uint32_t)lane < hi) {
      d = seg_d[base + lane];
      w = seg_w[base + lane];
    }
    // the list's topk-th entry: a chunk with nothing below it changes no entry that is written
    const u64 td = __shfl(bd, (int)topk - 1, 64), tw = __shfl(bw, (int)topk - 1, 64);
    if (!__ballot(knn_less(d, w, td, tw))) continue;
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) knn_cx(d, w, j, ((lane & j) == 0) == ((lane & k) == 0));
    }
    if (base != lo) {
      // lower half of the two ascending lists: min(best[i], chunk[63 - i]) is bitonic and holds the 64 smallest
      const u64 rd = __shfl(d, 63 - lane, 64), rw = __shfl(w, 63 - lane, 64);
      if (knn_less(bd, bw, rd, rw)) {
        d = bd;
        w = bw;
      } else {
        d = rd;
        w = rw;
      }
#pragma unroll
      for (int j = 32; j > 0; j >>= 1) knn_cx(d, w, j, (lane & j) == 0);
    }
    bd = d;
    bw = w;
  }
  const uint64_t row = row0 + t;
  if ((uint32_t)lane < topk) {
    const bool pad = bd == KNN_PAD;
    const uint64_t at = row * topk + (uint32_t)lane;
    nn_id[at] = pad ? 0xffffffffu : (uint32_t)(bw >> 32);
    if (nn_table) nn_table[at] = pad ? 0xffffffffu : (uint32_t)bw;
    nn_dist[at] = __longlong_as_double((long long)(pad ? KNN_INF : bd));
  }
  if (lane == 0) nn_count[row] = hi - lo;
}

// rows of padding and zero counts (a call that ran no batch)
__global__ __launch_bounds__(256) void hs_knn_fill_kernel(uint64_t rows, uint32_t topk, uint32_t* __restrict__ nn_id,
                                                          uint32_t* __restrict__ nn_table, double* __restrict__ nn_dist,
                                                          uint32_t* __restrict__ nn_count) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < rows * topk) {
    nn_id[i] = 0xffffffffu;
    if (nn_table) nn_table[i] = 0xffffffffu;
    nn_dist[i] = __longlong_as_double((long long)KNN_INF);
  }
  if (i < rows) nn_count[i] = 0u;
}

}  // namespace

size_t hs_knn_temp(uint32_t count) { return hs_scan_u32_temp((size_t)count + 1); }

hipError_t hs_launch_knn_batch(const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_q, const uint32_t* d_id,
                               const uint32_t* d_table, const double* d_dist, uint32_t n_hits, uint32_t self_first,
                               uint32_t first, uint32_t count, uint32_t* d_cnt, uint32_t* d_off, uint32_t* d_cur,
                               void* d_temp, size_t temp_bytes, uint64_t* d_seg_d, uint64_t* d_seg_w, uint64_t* d_total,
                               uint32_t topk, uint64_t row0, uint32_t* d_nn_id, uint32_t* d_nn_table, double* d_nn_dist,
                               uint32_t* d_nn_count, hipStream_t s) {
  if (!count) return hipSuccess;
  hipError_t e = hipMemsetAsync(d_cnt, 0, ((size_t)count + 1) * 4, s);
  if (e != hipSuccess) return e;
  if (n_hits)
    hs_knn_count_kernel<<<knn_blocks(n_hits), 256, 0, s>>>(d_key, d_val, d_q, d_id, d_table, d_dist, n_hits, self_first,
                                                          first, count, d_cnt);
  e = hs_exclusive_scan_u32(d_temp, temp_bytes, d_cnt, d_off, (size_t)count + 1, s);
  if (e != hipSuccess) return e;
  hs_knn_cursor_kernel<<<knn_blocks(count), 256, 0, s>>>(d_off, count, d_cur, reinterpret_cast<u64*>(d_total));
  if (n_hits)
    hs_knn_scatter_kernel<<<knn_blocks(n_hits), 256, 0, s>>>(d_key, d_val, d_q, d_id, d_table, d_dist, n_hits,
                                                            self_first, first, count, d_cur,
                                                            reinterpret_cast<u64*>(d_seg_d),
                                                            reinterpret_cast<u64*>(d_seg_w));
  hs_knn_select_kernel<<<(count + 3u) / 4u, 256, 0, s>>>(reinterpret_cast<const u64*>(d_seg_d),
                                                        reinterpret_cast<const u64*>(d_seg_w), d_off, count, topk,
                                                        row0 + first, d_nn_id, d_nn_table, d_nn_dist, d_nn_count);
  return hipGetLastError();
}

hipError_t hs_launch_knn_fill(uint64_t rows, uint32_t topk, uint32_t* d_nn_id, uint32_t* d_nn_table, double* d_nn_dist,
                              uint32_t* d_nn_count, hipStream_t s) {
  if (!rows) return hipSuccess;
  hs_knn_fill_kernel<<<knn_blocks(rows * topk), 256, 0, s>>>(rows, topk, d_nn_id, d_nn_table, d_nn_dist, d_nn_count);
  return hipGetLastError();
}

// ---- the same rule on the host for any list of tuples (no GPU, no handle) ------------------------------
extern "C" hs_status hs_topk_merge(const uint32_t* q, const uint32_t* id, const uint32_t* table, const double* dist,
                                   uint64_t n_tuples, uint64_t nq, uint32_t topk, uint32_t* nn_id, uint32_t* nn_table,
                                   double* nn_dist, uint32_t* nn_count) {
  if (topk < 1 || topk > HS_TOPK_MAX) return HS_ERR_INVALID;
  if (n_tuples && (!q || !id || !dist)) return HS_ERR_INVALID;  // (table == null: every table reads 0xffffffff)
  if (nq && (!nn_id || !nn_dist || !nn_count)) return HS_ERR_INVALID;
  try {
    std::vector<uint64_t> live;
    std::vector<uint64_t> bits(n_tuples);
    for (uint64_t i = 0; i < n_tuples; ++i) {
      if (id[i] == 0xffffffffu) continue;  // padding of a row fed back in
      if (q[i] >= nq || !(dist[i] >= 0.0)) return HS_ERR_INVALID;  // (a NaN compares false)
      const double d = dist[i] == 0.0 ? 0.0 : dist[i];  // -0.0 is read as +0.0
      memcpy(&bits[i], &d, 8);
      live.push_back(i);
    }
    const auto tab = [&](uint64_t i) { return table ? table[i] : 0xffffffffu; };
    // per (q, id) one tuple: the smallest table; two distances for one (q, id) are an error
    std::sort(live.begin(), live.end(), [&](uint64_t x, uint64_t y) {
      if (q[x] != q[y]) return q[x] < q[y];
      if (id[x] != id[y]) return id[x] < id[y];
      if (bits[x] != bits[y]) return bits[x] < bits[y];
      return tab(x) < tab(y);
    });
    size_t kept = 0;
    for (size_t i = 0; i < live.size(); ++i) {
      if (i && q[live[i]] == q[live[i - 1]] && id[live[i]] == id[live[i - 1]]) {
        if (bits[live[i]] != bits[live[i - 1]]) return HS_ERR_INVALID;
        continue;
      }
      live[kept++] = live[i];
    }
    live.resize(kept);
    std::sort(live.begin(), live.end(), [&](uint64_t x, uint64_t y) {
      if (q[x] != q[y]) return q[x] < q[y];
      if (bits[x] != bits[y]) return bits[x] < bits[y];
      return id[x] < id[y];
    });
    // everything is checked: the rows
    const double inf = std::numeric_limits<double>::infinity();
    for (uint64_t i = 0; i < nq * topk; ++i) {
      nn_id[i] = 0xffffffffu;
      if (nn_table) nn_table[i] = 0xffffffffu;
      nn_dist[i] = inf;
    }
    for (uint64_t i = 0; i < nq; ++i) nn_count[i] = 0u;
    for (size_t i = 0; i < live.size(); ++i) {
      const uint64_t j = live[i], row = q[j];
      const uint32_t r = nn_count[row]++;
      if (r < topk) {
        nn_id[row * topk + r] = id[j];
        if (nn_table) nn_table[row * topk + r] = tab(j);
        memcpy(&nn_dist[row * topk + r], &bits[j], 8);
      }
    }
  } catch (const std::bad_alloc&) {
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}
