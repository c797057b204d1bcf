// hs_seqmatch.hip -- a search's hits reduced per (query group, database sequence, diagonal) on the device
// (hs_seq_match, include/hsearch.h), and the same rule on the host for any list of tuples (hs_seq_match_hits) or of
// rows (hs_seq_match_merge).
//
// The rule.  A hit (q, id) has the key (g, s, diag): g = q_group[q] (or q), s the sequence whose id range
// [id_start[s], id_start[s + 1]) holds id, off = id - id_start[s], diag = off - q_off[q] (or 0).  One row per distinct
// key, ascending: the number of hits, the hit smallest under (dist, q, id), the smallest and the largest off.  Every
// reduction is an integer sum, min or max (a distance is >= +0 and never a NaN, so its bits order like the doubles):
// nothing below depends on the order the hits arrive in.
//
// The key is sparse -- n_groups x n_seq x diagonals slots exist, a handful are hit -- and a row's hits span batches (a
// group's queries need not lie in one batch), so the rows are found by sorting, never by addressing:
//   key   one hit per lane: q and id from the packed pair (or a merged list's arrays), s by a search in id_start whose
//         top 8 levels are 256 samples staged in LDS per workgroup (every lane reads id_start; the samples cut the
//         global part of the search to log2(n_seq / 256) dependent loads), the 64-bit key
//         g << (ws + wd) | s << wd | diag + max_qoff, and the hit's index
//   sort  hs_sort_pairs_u64_u32 over bits [0, wg + ws + wd): from bit 0, the safe side of hs_prims.hip's note
//   head  head[i] = the sorted key differs from its predecessor's; its exclusive scan numbers the rows, and the total
//         is read back (the stream is idle between batches) to grow the list the rows go to
//   reduce  one sorted element per lane.  A segmented inclusive scan over __shfl_up (six steps) carries (count, distance
//         bits, q << 32 | id, lo, hi) along runs of one row number.  Only a lane that ENDS its run -- inside the wave or
//         at the wave's last lane -- touches memory: a run that lies whole inside the wave is stored plainly, a run that
//         crosses a wave's edge is combined into the row's slot by integer atomics.  One row holding a whole batch costs
//         one set of atomics per wave; a batch of single-hit rows costs one plain store per row and no atomic.
//   best  the 96-bit best (distance bits, q << 32 | id) does not fit one atomic.  hs_annotate.hip's two-step rule: the
//         reduce kernel takes atomicMin of the distance bits and leaves each cut run's (row, distance, q << 32 | id)
//         in the wave's two partial slots (a cut run touches lane 0 or lane 63); behind the kernel boundary, the
//         partials whose distance IS the slot's take atomicMin of q << 32 | id.
// The batch's rows are appended to a list of the handle (40 bytes per row, grown by doubling).  At the end of a call
// to which more than one batch contributed the list is sorted and reduced once more by the same kernels with rows as
// their input; a last kernel decodes the keys into the output arrays.  All scratch is sized by a batch or by the rows
// found so far.  All stores are vector stores.
#include <algorithm>
#include <cstring>
#include <new>
#include <tuple>
#include <vector>

#include <hip/hip_runtime.h>

#include "hs_internal.h"

namespace {

typedef unsigned long long u64;

#define SM_NO_ROW 0xffffffffu
#define SM_SAMPLES 256u

inline unsigned sm_blocks(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

__host__ __device__ __forceinline__ u64 sm_shl(u64 x, int sh) { return sh >= 64 ? 0ull : x << sh; }
__host__ __device__ __forceinline__ u64 sm_mask(int bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1ull; }

struct SmHit {
  uint32_t q, id;
  u64 d;
};

// hit i of a batch (key / val) or of a merged list (q, id, dist)
__device__ __forceinline__ SmHit sm_load(const uint64_t* __restrict__ key, const uint64_t* __restrict__ val,
                                         const uint32_t* __restrict__ q, const uint32_t* __restrict__ id,
                                         const double* __restrict__ dist, uint32_t i) {
  SmHit h;
  if (key) {
    const uint64_t kk = key[i];
    h.q = (uint32_t)(kk >> 37);
    h.id = (uint32_t)kk;
    h.d = val[i];
  } else {
    h.q = q[i];
    h.id = id[i];
    h.d = (u64)__double_as_longlong(dist[i]);
  }
  return h;
}

// ---- the arguments checked on the device: out = {flags, max q_off, max ids of a sequence} ----------------------
// flags: 1 id_start not ascending, 2 id_start[0] != 0, 4 id_start[n_seq] != n, 8 a group >= n_groups
__global__ __launch_bounds__(256) void hs_sm_check_kernel(const uint32_t* __restrict__ q_group,
                                                          const uint32_t* __restrict__ q_off, uint64_t nq,
                                                          uint64_t n_groups, const uint64_t* __restrict__ id_start,
                                                          uint64_t n_seq, uint64_t n, u64* __restrict__ out) {
  const uint64_t t0 = (uint64_t)blockIdx.x * 256u + threadIdx.x, step = (uint64_t)gridDim.x * 256u;
  u64 flags = 0, mo = 0, ml = 0;
  for (uint64_t q = t0; q < nq; q += step) {
    if (q_group && q_group[q] >= n_groups) flags |= 8;
    if (q_off) mo = max(mo, (u64)q_off[q]);
  }
  for (uint64_t s = t0; s < n_seq; s += step) {
    const uint64_t a = id_start[s], b = id_start[s + 1];
    if (b < a) flags |= 1;
    else ml = max(ml, (u64)(b - a));
  }
  if (t0 == 0) {
    if (id_start[0] != 0) flags |= 2;
    if (id_start[n_seq] != n) flags |= 4;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    flags |= __shfl_xor(flags, m, 64);
    mo = max(mo, (u64)__shfl_xor(mo, m, 64));
    ml = max(ml, (u64)__shfl_xor(ml, m, 64));
  }
  if ((threadIdx.x & 63u) == 0) {
    if (flags) atomicOr(out, flags);
    if (mo) atomicMax(out + 1, mo);
    if (ml) atomicMax(out + 2, ml);
  }
}

// ---- key ------------------------------------------------------------------------------------------------------
// s with id_start[s] <= id < id_start[s + 1] (id < id_start[n_seq], checked before the call): the samples are
// id_start[min(t stride, n_seq)], t = 0 .. 255; equal neighbours (a sequence without ids) leave the LAST s that
// starts at or below id, the one that owns it
__global__ __launch_bounds__(256) void hs_sm_key_kernel(const uint64_t* __restrict__ key, const uint64_t* __restrict__ val,
                                                        const uint32_t* __restrict__ q, const uint32_t* __restrict__ id,
                                                        const double* __restrict__ dist, uint32_t n_hits,
                                                        const uint32_t* __restrict__ q_group,
                                                        const uint32_t* __restrict__ q_off,
                                                        const uint64_t* __restrict__ id_start, u64 n_seq,
                                                        uint32_t stride, int ws, int wd, u64 max_qoff,
                                                        u64* __restrict__ out_key, uint32_t* __restrict__ out_idx) {
  __shared__ uint32_t sample[SM_SAMPLES];
  {
    const u64 at = min((u64)threadIdx.x * stride, n_seq);
    sample[threadIdx.x] = (uint32_t)min(id_start[at], (uint64_t)0xffffffffu);
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_hits) return;
  const SmHit h = sm_load(key, val, q, id, dist, i);
  uint32_t a = 0, b = SM_SAMPLES;  // sample[a] <= id (sample[0] = 0), sample[b] > id or b = 256
  while (b - a > 1) {
    const uint32_t m = (a + b) >> 1;
    if (sample[m] <= h.id) a = m; else b = m;
  }
  u64 lo = min((u64)a * stride, n_seq), hi = min(((u64)a + 1) * stride, n_seq);
  if (lo >= hi) lo = hi ? hi - 1 : 0;  // (an id at or past id_start[n_seq]: cannot happen, and reads nothing out of bounds)
  while (hi - lo > 1) {
    const u64 m = (lo + hi) >> 1;
    if (id_start[m] <= (uint64_t)h.id) lo = m; else hi = m;
  }
  const u64 s = lo;
  const u64 off = (u64)h.id - id_start[s];
  const u64 g = q_group ? q_group[h.q] : h.q;
  const u64 dg = q_off ? off - (u64)q_off[h.q] + max_qoff : 0ull;
  out_key[i] = sm_shl(g, ws + wd) | sm_shl(s, wd) | (dg & sm_mask(wd));
  out_idx[i] = i;
}

__global__ __launch_bounds__(256) void hs_sm_iota_kernel(uint32_t n, uint32_t* __restrict__ idx) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) idx[i] = i;
}

// head[i], i < n: the sorted key starts a run; head[n] = 0 (its scan slot receives the number of runs)
__global__ __launch_bounds__(256) void hs_sm_head_kernel(const u64* __restrict__ skey, uint32_t n,
                                                         uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  head[i] = i < n && (i == 0 || skey[i] != skey[i - 1]) ? 1u : 0u;
}

// rows [0, n) of a list to the state the atomics start from
__global__ __launch_bounds__(256) void hs_sm_fill_kernel(uint32_t n, u64* __restrict__ r_cnt, u64* __restrict__ r_d,
                                                         u64* __restrict__ r_qid, uint32_t* __restrict__ r_lo,
                                                         uint32_t* __restrict__ r_hi) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  r_cnt[i] = 0;
  r_d[i] = ~0ull;
  r_qid[i] = ~0ull;
  r_lo[i] = 0xffffffffu;
  r_hi[i] = 0;
}

// ---- reduce -----------------------------------------------------------------------------------------------------
// Sorted element i (key skey[i], source index sidx[i], row excl[i] + head[i] - 1) per lane.  The source is a batch's
// hits (src.cnt == null: key / val or q / id / dist, off = id - id_start[s] with s from the key) or the rows of a
// list.  The rows go to dst at their row number.  part_* [2 x waves]: the wave's cut runs (slot 2w: the run that
// came in over lane 0, slot 2w + 1: the run that leaves over lane 63), SM_NO_ROW where there is none.
struct SmRows {
  u64 *key, *cnt, *d, *qid;
  uint32_t *lo, *hi;
};

__global__ __launch_bounds__(256) void hs_sm_reduce_kernel(const u64* __restrict__ skey, const uint32_t* __restrict__ sidx,
                                                           const uint32_t* __restrict__ excl,
                                                           const uint32_t* __restrict__ head, uint32_t n,
                                                           const uint64_t* __restrict__ key, const uint64_t* __restrict__ val,
                                                           const uint32_t* __restrict__ q, const uint32_t* __restrict__ id,
                                                           const double* __restrict__ dist,
                                                           const uint64_t* __restrict__ id_start, int ws, int wd,
                                                           SmRows src, SmRows dst, uint32_t* __restrict__ part_row,
                                                           u64* __restrict__ part_d, u64* __restrict__ part_qid) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = i >> 6;
  const bool valid = i < n;
  uint32_t r = SM_NO_ROW, lo = 0xffffffffu, hi = 0;
  u64 cnt = 0, d = ~0ull, qid = ~0ull;
  bool hh = false, tail = false;
  if (valid) {
    const uint32_t hd = head[i], j = sidx[i];
    const u64 k = skey[i];
    r = excl[i] + hd - 1u;
    hh = hd != 0;
    tail = i + 1 >= n || head[i + 1] != 0;
    if (src.cnt) {
      cnt = src.cnt[j];
      d = src.d[j];
      qid = src.qid[j];
      lo = src.lo[j];
      hi = src.hi[j];
    } else {
      const SmHit h = sm_load(key, val, q, id, dist, j);
      const u64 s = (k >> wd) & sm_mask(ws);
      cnt = 1;
      d = h.d;
      qid = (u64)h.q << 32 | h.id;
      lo = hi = (uint32_t)((u64)h.id - id_start[s]);
    }
    if (hh) dst.key[r] = k;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const uint32_t r2 = __shfl_up(r, m, 64), lo2 = __shfl_up(lo, m, 64), hi2 = __shfl_up(hi, m, 64);
    const u64 cnt2 = __shfl_up(cnt, m, 64), d2 = __shfl_up(d, m, 64), qid2 = __shfl_up(qid, m, 64);
    const int hh2 = __shfl_up((int)hh, m, 64);
    if (lane >= (uint32_t)m && r2 == r && valid) {
      cnt += cnt2;
      if (d2 < d || (d2 == d && qid2 < qid)) {
        d = d2;
        qid = qid2;
      }
      lo = min(lo, lo2);
      hi = max(hi, hi2);
      hh = hh || hh2 != 0;
    }
  }
  const bool cut_in = valid && tail && !hh;            // came in over lane 0, ends here
  const bool cut_out = valid && lane == 63u && !tail;  // leaves over lane 63 (it may have come in over lane 0 too)
  if (valid && tail && hh) {
    dst.cnt[r] = cnt;
    dst.d[r] = d;
    dst.qid[r] = qid;
    dst.lo[r] = lo;
    dst.hi[r] = hi;
  } else if (cut_in || cut_out) {
    atomicAdd(dst.cnt + r, cnt);
    atomicMin(dst.d + r, d);
    atomicMin(dst.lo + r, lo);
    atomicMax(dst.hi + r, hi);
    const uint32_t slot = 2u * wave + (cut_out ? 1u : 0u);
    part_row[slot] = r;
    part_d[slot] = d;
    part_qid[slot] = qid;
  }
  // (a wave has at most one lane of each kind; the slot nobody claimed is marked by lane 0)
  const bool any_in = __ballot(cut_in) != 0ull, any_out = __ballot(cut_out) != 0ull;
  if (lane == 0 && wave * 64u < n) {
    if (!any_in) part_row[2u * wave] = SM_NO_ROW;
    if (!any_out) part_row[2u * wave + 1u] = SM_NO_ROW;
  }
}

// every slot's distance is final (the reduce kernel has ended): the cut runs AT that distance compete for the slot's
// q << 32 | id
__global__ __launch_bounds__(256) void hs_sm_best_kernel(const uint32_t* __restrict__ part_row,
                                                         const u64* __restrict__ part_d,
                                                         const u64* __restrict__ part_qid, uint32_t n_part,
                                                         uint32_t n_rows, const u64* __restrict__ r_d,
                                                         u64* __restrict__ r_qid) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_part) return;
  const uint32_t r = part_row[p];
  if (r >= n_rows) return;
  if (r_d[r] == part_d[p]) atomicMin(r_qid + r, part_qid[p]);
}

// rows of a list into the output arrays; *flag |= 1 where a count does not fit 32 bits
__global__ __launch_bounds__(256) void hs_sm_decode_kernel(SmRows rows, uint32_t n, int ws, int wd, u64 max_qoff,
                                                           uint32_t* __restrict__ out_group,
                                                           uint32_t* __restrict__ out_seq, int32_t* __restrict__ out_diag,
                                                           uint32_t* __restrict__ out_count,
                                                           double* __restrict__ out_best_dist,
                                                           uint32_t* __restrict__ out_best_q,
                                                           uint32_t* __restrict__ out_best_id,
                                                           uint32_t* __restrict__ out_lo, uint32_t* __restrict__ out_hi,
                                                           uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const u64 k = rows.key[i], c = rows.cnt[i], qid = rows.qid[i];
  if (c > 0xffffffffull) atomicOr(flag, 1u);
  out_group[i] = (uint32_t)(ws + wd >= 64 ? 0ull : k >> (ws + wd));
  out_seq[i] = (uint32_t)((k >> wd) & sm_mask(ws));
  out_diag[i] = (int32_t)(uint32_t)((k & sm_mask(wd)) - max_qoff);
  out_count[i] = (uint32_t)c;
  out_best_dist[i] = __longlong_as_double((long long)rows.d[i]);
  out_best_q[i] = (uint32_t)(qid >> 32);
  out_best_id[i] = (uint32_t)qid;
  out_lo[i] = rows.lo[i];
  out_hi[i] = rows.hi[i];
}

SmRows sm_rows_at(void* base, uint64_t cap, uint64_t row0) {
  char* const p = static_cast<char*>(base);
  SmRows r;
  r.key = reinterpret_cast<u64*>(p) + row0;
  r.cnt = reinterpret_cast<u64*>(p + cap * 8) + row0;
  r.d = reinterpret_cast<u64*>(p + cap * 16) + row0;
  r.qid = reinterpret_cast<u64*>(p + cap * 24) + row0;
  r.lo = reinterpret_cast<uint32_t*>(p + cap * 32) + row0;
  r.hi = reinterpret_cast<uint32_t*>(p + cap * 36) + row0;
  return r;
}

}  // namespace

hipError_t hs_launch_sm_check(const uint32_t* d_q_group, const uint32_t* d_q_off, uint64_t nq, uint64_t n_groups,
                              const uint64_t* d_id_start, uint64_t n_seq, uint64_t n, uint64_t* d_out, hipStream_t s) {
  const uint64_t work = std::max<uint64_t>(std::max(nq, n_seq), 1);
  const unsigned blocks = (unsigned)std::min<uint64_t>(1024, (work + 255) / 256);
  hs_sm_check_kernel<<<blocks, 256, 0, s>>>(d_q_group, d_q_off, nq, n_groups, d_id_start, n_seq, n,
                                            reinterpret_cast<u64*>(d_out));
  return hipGetLastError();
}

hipError_t hs_launch_sm_key(const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_q, const uint32_t* d_id,
                            const double* d_dist, uint32_t n_hits, const uint32_t* d_q_group, const uint32_t* d_q_off,
                            const uint64_t* d_id_start, uint64_t n_seq, int ws, int wd, uint64_t max_qoff,
                            uint64_t* d_out_key, uint32_t* d_out_idx, hipStream_t s) {
  if (!n_hits) return hipSuccess;
  const uint32_t stride = (uint32_t)((n_seq + SM_SAMPLES) / SM_SAMPLES);  // ceil((n_seq + 1) / 256)
  hs_sm_key_kernel<<<sm_blocks(n_hits), 256, 0, s>>>(d_key, d_val, d_q, d_id, d_dist, n_hits, d_q_group, d_q_off,
                                                     d_id_start, n_seq, stride, ws, wd, max_qoff,
                                                     reinterpret_cast<u64*>(d_out_key), d_out_idx);
  return hipGetLastError();
}

hipError_t hs_launch_sm_iota(uint32_t n, uint32_t* d_idx, hipStream_t s) {
  if (!n) return hipSuccess;
  hs_sm_iota_kernel<<<sm_blocks(n), 256, 0, s>>>(n, d_idx);
  return hipGetLastError();
}

hipError_t hs_launch_sm_head(const uint64_t* d_skey, uint32_t n, uint32_t* d_head, hipStream_t s) {
  hs_sm_head_kernel<<<sm_blocks((uint64_t)n + 1), 256, 0, s>>>(reinterpret_cast<const u64*>(d_skey), n, d_head);
  return hipGetLastError();
}

size_t hs_sm_part_bytes(uint32_t n) { return (size_t)2 * ((n + 63u) / 64u) * 20 + 16; }

hipError_t hs_launch_sm_reduce(const uint64_t* d_skey, const uint32_t* d_sidx, const uint32_t* d_excl,
                               const uint32_t* d_head, uint32_t n, const uint64_t* d_key, const uint64_t* d_val,
                               const uint32_t* d_q, const uint32_t* d_id, const double* d_dist,
                               const uint64_t* d_id_start, int ws, int wd, const void* d_src_rows, uint64_t src_cap,
                               void* d_dst_rows, uint64_t dst_cap, uint64_t dst_row0, uint32_t n_rows, void* d_part,
                               hipStream_t s) {
  if (!n || !n_rows) return hipSuccess;
  SmRows src = {};
  if (d_src_rows) src = sm_rows_at(const_cast<void*>(d_src_rows), src_cap, 0);
  const SmRows dst = sm_rows_at(d_dst_rows, dst_cap, dst_row0);
  const uint32_t n_part = 2u * ((n + 63u) / 64u);
  u64* const part_d = static_cast<u64*>(d_part);
  u64* const part_qid = part_d + n_part;
  uint32_t* const part_row = reinterpret_cast<uint32_t*>(part_qid + n_part);
  hs_sm_fill_kernel<<<sm_blocks(n_rows), 256, 0, s>>>(n_rows, dst.cnt, dst.d, dst.qid, dst.lo, dst.hi);
  hs_sm_reduce_kernel<<<sm_blocks(n), 256, 0, s>>>(reinterpret_cast<const u64*>(d_skey), d_sidx, d_excl, d_head, n, d_key,
                                                   d_val, d_q, d_id, d_dist, d_id_start, ws, wd, src, dst, part_row,
                                                   part_d, part_qid);
  hs_sm_best_kernel<<<sm_blocks(n_part), 256, 0, s>>>(part_row, part_d, part_qid, n_part, n_rows, dst.d, dst.qid);
  return hipGetLastError();
}

hipError_t hs_launch_sm_decode(const void* d_rows, uint64_t cap, uint32_t n, int ws, int wd, uint64_t max_qoff,
                               uint32_t* d_group, uint32_t* d_seq, int32_t* d_diag, uint32_t* d_count,
                               double* d_best_dist, uint32_t* d_best_q, uint32_t* d_best_id, uint32_t* d_lo,
                               uint32_t* d_hi, uint32_t* d_flag, hipStream_t s) {
  if (!n) return hipSuccess;
  hs_sm_decode_kernel<<<sm_blocks(n), 256, 0, s>>>(sm_rows_at(const_cast<void*>(d_rows), cap, 0), n, ws, wd, max_qoff,
                                                   d_group, d_seq, d_diag, d_count, d_best_dist, d_best_q, d_best_id,
                                                   d_lo, d_hi, d_flag);
  return hipGetLastError();
}

// ---- the same rule on the host (no GPU, no handle) ------------------------------------------------------------
static int sm_bits(uint64_t x) {
  int b = 0;
  while (x) {
    ++b;
    x >>= 1;
  }
  return b;
}

// the width rule over checked arguments: false when the key would not fit 64 bits
bool hs_sm_widths(uint64_t n_groups, uint64_t n_seq, uint64_t max_len, uint64_t max_qoff, int* wg, int* ws, int* wd) {
  *wg = sm_bits(n_groups ? n_groups - 1 : 0);
  *ws = sm_bits(n_seq ? n_seq - 1 : 0);
  *wd = max_len + max_qoff ? sm_bits(max_len + max_qoff - 1) : 0;
  return *wg + *ws + *wd <= 64;
}

// q_group / q_off / id_start as the contract wants them (id_start's end is the caller's to compare with n)
static bool sm_check_host(uint64_t nq, const uint32_t* q_group, uint64_t n_groups, const uint32_t* q_off,
                          const uint64_t* id_start, uint64_t n_seq) {
  if (!id_start || id_start[0] != 0) return false;
  if (n_groups > (1ull << 32) || n_seq > (1ull << 32)) return false;
  if (!q_group && n_groups != nq) return false;
  uint64_t max_len = 0, max_qoff = 0;
  for (uint64_t s = 0; s < n_seq; ++s) {
    if (id_start[s + 1] < id_start[s]) return false;
    max_len = std::max(max_len, id_start[s + 1] - id_start[s]);
  }
  if (id_start[n_seq] > 0xffffffffull) return false;
  for (uint64_t q = 0; q < nq; ++q) {
    if (q_group && q_group[q] >= n_groups) return false;
    if (q_off) max_qoff = std::max<uint64_t>(max_qoff, q_off[q]);
  }
  int wg, ws, wd;
  return hs_sm_widths(n_groups, n_seq, max_len, max_qoff, &wg, &ws, &wd);
}

namespace {
struct SmRow {
  uint32_t g, s;
  int64_t diag;
  uint64_t cnt, d;
  uint32_t q, id, lo, hi;
};
inline bool sm_key_less(const SmRow& a, const SmRow& b) {
  return std::tie(a.g, a.s, a.diag) < std::tie(b.g, b.s, b.diag);
}
inline bool sm_key_equal(const SmRow& a, const SmRow& b) { return a.g == b.g && a.s == b.s && a.diag == b.diag; }

// rows sorted by key (and anything after it) combined in place; false: a count passes 2^32 - 1
bool sm_combine(std::vector<SmRow>& v) {
  size_t kept = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    if (kept && sm_key_equal(v[kept - 1], v[i])) {
      SmRow& a = v[kept - 1];
      const SmRow& b = v[i];
      a.cnt += b.cnt;
      if (a.cnt > 0xffffffffull) return false;
      if (std::tie(b.d, b.q, b.id) < std::tie(a.d, a.q, a.id)) {
        a.d = b.d;
        a.q = b.q;
        a.id = b.id;
      }
      a.lo = std::min(a.lo, b.lo);
      a.hi = std::max(a.hi, b.hi);
    } else {
      v[kept++] = v[i];
    }
  }
  v.resize(kept);
  return true;
}

void sm_write(const std::vector<SmRow>& v, uint32_t* out_group, uint32_t* out_seq, int32_t* out_diag,
              uint32_t* out_count, double* out_best_dist, uint32_t* out_best_q, uint32_t* out_best_id, uint32_t* out_lo,
              uint32_t* out_hi) {
  for (size_t i = 0; i < v.size(); ++i) {
    out_group[i] = v[i].g;
    out_seq[i] = v[i].s;
    out_diag[i] = (int32_t)(uint32_t)(uint64_t)v[i].diag;
    out_count[i] = (uint32_t)v[i].cnt;
    memcpy(out_best_dist + i, &v[i].d, 8);
    out_best_q[i] = v[i].q;
    out_best_id[i] = v[i].id;
    out_lo[i] = v[i].lo;
    out_hi[i] = v[i].hi;
  }
}
}  // namespace

extern "C" hs_status hs_window_id_start(const uint64_t* seq_start, uint64_t n_seq, uint32_t k, uint64_t* id_start) {
  if (!seq_start || !id_start || !k) return HS_ERR_INVALID;
  for (uint64_t s = 0; s < n_seq; ++s)
    if (seq_start[s + 1] < seq_start[s]) return HS_ERR_INVALID;
  uint64_t at = 0;
  for (uint64_t s = 0; s < n_seq; ++s) {
    id_start[s] = at;
    const uint64_t len = seq_start[s + 1] - seq_start[s];
    if (len >= k) at += len - k + 1;
  }
  id_start[n_seq] = at;
  return HS_OK;
}

extern "C" hs_status hs_seq_match_hits(const uint32_t* q, const uint32_t* id, const double* dist, uint64_t n_tuples,
                                       uint64_t nq, const uint32_t* q_group, uint64_t n_groups, const uint32_t* q_off,
                                       const uint64_t* id_start, uint64_t n_seq, uint32_t* out_group, uint32_t* out_seq,
                                       int32_t* out_diag, uint32_t* out_count, double* out_best_dist,
                                       uint32_t* out_best_q, uint32_t* out_best_id, uint32_t* out_lo, uint32_t* out_hi,
                                       uint64_t cap, uint64_t* n_out) {
  if (!n_out) return HS_ERR_INVALID;
  *n_out = 0;
  if (n_tuples && (!q || !id || !dist)) return HS_ERR_INVALID;
  if (cap && (!out_group || !out_seq || !out_diag || !out_count || !out_best_dist || !out_best_q || !out_best_id ||
              !out_lo || !out_hi))
    return HS_ERR_INVALID;
  if (!sm_check_host(nq, q_group, n_groups, q_off, id_start, n_seq)) return HS_ERR_INVALID;
  try {
    std::vector<SmRow> v(n_tuples);
    for (uint64_t i = 0; i < n_tuples; ++i) {
      if (q[i] >= nq || id[i] >= id_start[n_seq]) return HS_ERR_INVALID;
      if (!(dist[i] >= 0.0)) return HS_ERR_INVALID;  // (a NaN too)
      const double dd = dist[i] + 0.0;               // -0.0 -> +0.0
      SmRow& r = v[i];
      r.g = q_group ? q_group[q[i]] : q[i];
      r.s = (uint32_t)(std::upper_bound(id_start, id_start + n_seq + 1, (uint64_t)id[i]) - id_start - 1);
      const uint64_t off = id[i] - id_start[r.s];
      r.diag = q_off ? (int64_t)off - (int64_t)q_off[q[i]] : 0;
      r.cnt = 1;
      memcpy(&r.d, &dd, 8);
      r.q = q[i];
      r.id = id[i];
      r.lo = r.hi = (uint32_t)off;
    }
    std::sort(v.begin(), v.end(), [](const SmRow& a, const SmRow& b) {
      return std::tie(a.g, a.s, a.diag, a.q, a.id, a.d) < std::tie(b.g, b.s, b.diag, b.q, b.id, b.d);
    });
    // a (q, id) given several times counts once and carries one distance
    size_t kept = 0;
    for (size_t i = 0; i < v.size(); ++i) {
      if (kept && v[kept - 1].q == v[i].q && v[kept - 1].id == v[i].id) {
        if (v[kept - 1].d != v[i].d) return HS_ERR_INVALID;
        continue;
      }
      v[kept++] = v[i];
    }
    v.resize(kept);
    if (!sm_combine(v)) return HS_ERR_INVALID;
    *n_out = v.size();
    if (v.size() > cap) return HS_ERR_CAPACITY;
    sm_write(v, out_group, out_seq, out_diag, out_count, out_best_dist, out_best_q, out_best_id, out_lo, out_hi);
  } catch (const std::bad_alloc&) {
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}

extern "C" hs_status hs_seq_match_merge(const uint32_t* group, const uint32_t* seq, const int32_t* diag,
                                        const uint32_t* count, const double* best_dist, const uint32_t* best_q,
                                        const uint32_t* best_id, const uint32_t* lo, const uint32_t* hi, uint64_t n_rows,
                                        uint32_t* out_group, uint32_t* out_seq, int32_t* out_diag, uint32_t* out_count,
                                        double* out_best_dist, uint32_t* out_best_q, uint32_t* out_best_id,
                                        uint32_t* out_lo, uint32_t* out_hi, uint64_t cap, uint64_t* n_out) {
  if (!n_out) return HS_ERR_INVALID;
  *n_out = 0;
  if (n_rows && (!group || !seq || !diag || !count || !best_dist || !best_q || !best_id || !lo || !hi))
    return HS_ERR_INVALID;
  if (cap && (!out_group || !out_seq || !out_diag || !out_count || !out_best_dist || !out_best_q || !out_best_id ||
              !out_lo || !out_hi))
    return HS_ERR_INVALID;
  try {
    std::vector<SmRow> v(n_rows);
    for (uint64_t i = 0; i < n_rows; ++i) {
      if (!(best_dist[i] >= 0.0) || !count[i] || lo[i] > hi[i]) return HS_ERR_INVALID;
      const double dd = best_dist[i] + 0.0;
      SmRow& r = v[i];
      r.g = group[i];
      r.s = seq[i];
      r.diag = diag[i];
      r.cnt = count[i];
      memcpy(&r.d, &dd, 8);
      r.q = best_q[i];
      r.id = best_id[i];
      r.lo = lo[i];
      r.hi = hi[i];
    }
    std::stable_sort(v.begin(), v.end(), sm_key_less);
    if (!sm_combine(v)) return HS_ERR_INVALID;
    *n_out = v.size();
    if (v.size() > cap) return HS_ERR_CAPACITY;
    sm_write(v, out_group, out_seq, out_diag, out_count, out_best_dist, out_best_q, out_best_id, out_lo, out_hi);
  } catch (const std::bad_alloc&) {
    return HS_ERR_NOMEM;
  }
  return HS_OK;
}
