// hs_pssm_family.hip -- hs_pssm_family_scan: a profile scan's hits reduced per (family, database sequence, diagonal) on
// the device (include/hsearch.h), and the rules on the host (hs_pssm_family_hits, hs_pssm_family_layout:
// hs_pssm_family.h).
//
// Batches are cut at GROUP boundaries (hs_capi_pssm.hip), so every hit of a family lies in one batch, every row is
// complete inside it, and the batches' rows follow one another in output order: no row list on the handle, no merge.
// Per batch of nh hits sorted by m << 32 | id (the scan's own sort; val = the score's bits):
//   seq     the sequence of every hit: hs_pssm_seq.hip's search
//   key     one hit per lane: the row key  (g << ws | s) << wd | (off + max_off - m_off[m])  -- the last field is the
//           diagonal shifted to be non-negative, so the key's order is (g, s, signed diag) -- and the hit's index.
//           The lanes at the two ends of a profile's run add the run's length to cnt[m] (two atomics per profile).
//   sort    hs_sort_pairs_u64_u32 (row key -> hit index) over the key's bits: rocPRIM's radix sort is stable, so the
//           hits of a row stay in ascending (m, id), the order the sum is defined in
//   head    run heads of the sorted keys (hs_seqmatch.hip's kernel), their exclusive scan, the rows read back
//   start   every head lane notes where its run starts
//   row     one row per lane, its run read once from first to last: count, the sequential fp64 sum, the best hit
//           under the ordered key (a strictly better score wins, so ties keep the earlier (m, id)), the smallest and
//           largest offset; then the two filters.  A row of L hits costs L dependent loads and fp64 adds in one lane:
//           the order of the sum is the contract, so a long row is not spread over lanes.
//   keep    the exclusive scan of the filters' flags, the kept rows read back
//   write   one row per lane: a kept row goes to the caller's arrays at the call's running offset plus its number
//           among the kept, and adds one to grp_rows[g].  Without room only grp_rows is counted.
// Scratch is sized by a batch's hits and rows.  All stores are vector stores.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_pssm_family.h"

namespace {

typedef unsigned long long u64;

inline unsigned pf_blocks(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

// the HS_FAM_BAD_* bits of m_group [nm], m_off [nm], t_group [n_groups] (each may be null) into *flag
__global__ __launch_bounds__(256) void hs_pssm_family_check_kernel(const uint32_t* __restrict__ m_group,
                                                                   const uint32_t* __restrict__ m_off,
                                                                   const double* __restrict__ t_group, uint64_t nm,
                                                                   uint64_t n_groups, uint32_t* __restrict__ flag) {
  const uint64_t t0 = (uint64_t)blockIdx.x * 256u + threadIdx.x, step = (uint64_t)gridDim.x * 256u;
  uint32_t bad = 0;
  for (uint64_t m = t0; m < nm; m += step) {
    if (m_group) {
      const uint32_t g = m_group[m];
      if (m && g < m_group[m - 1]) bad |= HS_FAM_BAD_GROUP_ORDER;
      if (g >= n_groups) bad |= HS_FAM_BAD_GROUP_VALUE;
      if (m >= HS_PSSM_FAMILY_MAX_GROUP && g == m_group[m - HS_PSSM_FAMILY_MAX_GROUP]) bad |= HS_FAM_BAD_GROUP_SIZE;
    }
    if (m_off && m_off[m] > HS_PSSM_FAMILY_MAX_OFF) bad |= HS_FAM_BAD_OFF;
    if (m_off && m_group && m && m_group[m] == m_group[m - 1] && m_off[m] < m_off[m - 1]) bad |= HS_FAM_BAD_OFF_ORDER;
  }
  for (uint64_t g = t0; t_group && g < n_groups; g += step) {
    const double t = t_group[g];
    if (t != t || t - t != 0.0) bad |= HS_FAM_BAD_T_GROUP;
  }
  for (int m = 32; m >= 1; m >>= 1) bad |= __shfl_xor(bad, m, 64);
  if ((threadIdx.x & 63u) == 0 && bad) atomicOr(flag, bad);
}

// hit i (sorted by m << 32 | id) -> its row key and index; cnt[m] += the length of every profile's run
__global__ __launch_bounds__(256) void hs_pssm_family_key_kernel(const uint64_t* __restrict__ key,
                                                                 const uint32_t* __restrict__ seq, uint32_t n,
                                                                 const uint32_t* __restrict__ m_group,
                                                                 const uint32_t* __restrict__ m_off,
                                                                 const uint64_t* __restrict__ id_start, int ws, int wd,
                                                                 u64 max_off, u64* __restrict__ row_key,
                                                                 uint32_t* __restrict__ idx, u64* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t kk = key[i];
  const uint32_t m = (uint32_t)(kk >> 32), id = (uint32_t)kk, s = seq[i];
  const u64 g = m_group ? m_group[m] : m;
  const u64 field = m_off ? ((u64)id - id_start[s]) + max_off - (u64)m_off[m] : 0ull;
  // ws <= 32 (n_seq <= 2^32) and wd <= 33 (an index holds at most 2^32 ids, an m_off is below 2^31), and the callers
  // have checked wg + ws + wd <= 64: every shift here and in the row kernel's decode is below 64 and loses no bit
  row_key[i] = (((g << ws) | (u64)s) << wd) | field;
  idx[i] = i;
  if (cnt) {  // (u64 arithmetic wraps: -i from the run's first lane, i + 1 from its last)
    if (i + 1 == n || (uint32_t)(key[i + 1] >> 32) != m) atomicAdd(cnt + m, (u64)i + 1ull);
    if (i && (uint32_t)(key[i - 1] >> 32) != m) atomicAdd(cnt + m, 0ull - (u64)i);
  }
}

// row_start [rows + 1]: where every run of the sorted keys begins, and n
__global__ __launch_bounds__(256) void hs_pssm_family_start_kernel(const uint32_t* __restrict__ head,
                                                                   const uint32_t* __restrict__ excl, uint32_t n,
                                                                   uint32_t* __restrict__ row_start) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  if (i == n) row_start[excl[n]] = n;
  else if (head[i]) row_start[excl[i]] = i;
}

struct PfRows {
  uint32_t *group, *seq;
  int32_t* diag;
  uint32_t* count;
  double *sum, *best_score;
  uint32_t *best_m, *best_id, *lo, *hi;
};

// Row r per lane: its run [row_start[r], row_start[r + 1]) of the sorted (row key, hit index) pairs walked in order.
// keep [n_rows + 1]: the filters' flag, and 0 behind the last row (its scan slot receives the kept rows).
__global__ __launch_bounds__(256) void hs_pssm_family_row_kernel(const u64* __restrict__ skey,
                                                                 const uint32_t* __restrict__ sidx,
                                                                 const uint32_t* __restrict__ row_start, uint32_t n_rows,
                                                                 const uint64_t* __restrict__ key,
                                                                 const uint64_t* __restrict__ val,
                                                                 const uint64_t* __restrict__ id_start, int ws, int wd,
                                                                 u64 max_off, uint32_t min_count,
                                                                 const double* __restrict__ t_group, PfRows rows,
                                                                 uint32_t* __restrict__ keep) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r > n_rows) return;
  if (r == n_rows) {
    keep[r] = 0;
    return;
  }
  const uint32_t a = row_start[r], b = row_start[r + 1];
  const u64 rk = skey[a];
  // the key kernel's fields back out (its bounds: ws <= 32, wd <= 33)
  const u64 field = rk & ((1ull << wd) - 1ull), gs = rk >> wd;
  const uint32_t s = (uint32_t)(gs & ((1ull << ws) - 1ull)), g = (uint32_t)(gs >> ws);
  const uint64_t base = id_start[s];
  double sum = 0.0;
  u64 best_u = 0;
  uint32_t best_m = 0, best_id = 0, lo = 0xffffffffu, hi = 0;
  for (uint32_t i = a; i < b; ++i) {
    const uint32_t j = sidx[i];
    const uint64_t kk = key[j], bits = val[j];
    const uint32_t off = (uint32_t)((uint64_t)(uint32_t)kk - base);
    sum = sum + __longlong_as_double((long long)bits);
    const u64 u = hs_pssm_order_key(bits);
    if (i == a || u > best_u) {
      best_u = u;
      best_m = (uint32_t)(kk >> 32);
      best_id = (uint32_t)kk;
    }
    lo = min(lo, off);
    hi = max(hi, off);
  }
  rows.group[r] = g;
  rows.seq[r] = s;
  rows.diag[r] = (int32_t)(uint32_t)(field - max_off);
  rows.count[r] = b - a;
  rows.sum[r] = sum;
  rows.best_score[r] = __longlong_as_double((long long)hs_pssm_order_bits(best_u));
  rows.best_m[r] = best_m;
  rows.best_id[r] = best_id;
  rows.lo[r] = lo;
  rows.hi[r] = hi;
  keep[r] = (b - a >= min_count && (!t_group || sum >= t_group[g])) ? 1u : 0u;
}

// kept row r -> slot pos[r] of the output (write != 0), and grp_rows[g] += 1
__global__ __launch_bounds__(256) void hs_pssm_family_write_kernel(PfRows rows, const uint32_t* __restrict__ keep,
                                                                   const uint32_t* __restrict__ pos, uint32_t n_rows,
                                                                   int write, PfRows out, u64* __restrict__ grp_rows) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_rows || !keep[r]) return;
  if (grp_rows) atomicAdd(grp_rows + rows.group[r], 1ull);
  if (!write) return;
  const uint32_t at = pos[r];
  out.group[at] = rows.group[r];
  out.seq[at] = rows.seq[r];
  out.diag[at] = rows.diag[r];
  out.count[at] = rows.count[r];
  out.sum[at] = rows.sum[r];
  out.best_score[at] = rows.best_score[r];
  out.best_m[at] = rows.best_m[r];
  out.best_id[at] = rows.best_id[r];
  out.lo[at] = rows.lo[r];
  out.hi[at] = rows.hi[r];
}

PfRows pf_rows(const HsFamilyOut& o) {
  return PfRows{o.group, o.seq, o.diag, o.count, o.sum, o.best_score, o.best_m, o.best_id, o.lo, o.hi};
}

}  // namespace

hipError_t hs_launch_pssm_family_check(const uint32_t* d_m_group, const uint32_t* d_m_off, const double* d_t_group,
                                       uint64_t nm, uint64_t n_groups, uint32_t* d_flag, hipStream_t s) {
  const uint64_t work = std::max<uint64_t>(std::max(nm, d_t_group ? n_groups : 0), 1);
  const unsigned blocks = (unsigned)std::min<uint64_t>(1024, (work + 255) / 256);
  hs_pssm_family_check_kernel<<<blocks, 256, 0, s>>>(d_m_group, d_m_off, d_t_group, nm, n_groups, d_flag);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_family_key(const uint64_t* d_key, const uint32_t* d_seq, uint32_t n, const uint32_t* d_m_group,
                                     const uint32_t* d_m_off, const uint64_t* d_id_start, int ws, int wd,
                                     uint64_t max_off, uint64_t* d_row_key, uint32_t* d_idx, uint64_t* d_cnt,
                                     hipStream_t s) {
  if (!n) return hipSuccess;
  hs_pssm_family_key_kernel<<<pf_blocks(n), 256, 0, s>>>(d_key, d_seq, n, d_m_group, d_m_off, d_id_start, ws, wd, max_off,
                                                         reinterpret_cast<u64*>(d_row_key), d_idx,
                                                         reinterpret_cast<u64*>(d_cnt));
  return hipGetLastError();
}

hipError_t hs_launch_pssm_family_rows(const uint64_t* d_skey, const uint32_t* d_sidx, const uint32_t* d_head,
                                      const uint32_t* d_excl, uint32_t n, uint32_t n_rows, const uint64_t* d_key,
                                      const uint64_t* d_val, const uint64_t* d_id_start, int ws, int wd,
                                      uint64_t max_off, uint32_t min_count, const double* d_t_group,
                                      uint32_t* d_row_start, void* d_rows, uint32_t* d_keep, hipStream_t s) {
  if (!n || !n_rows) return hipSuccess;
  hs_pssm_family_start_kernel<<<pf_blocks((uint64_t)n + 1), 256, 0, s>>>(d_head, d_excl, n, d_row_start);
  hs_pssm_family_row_kernel<<<pf_blocks((uint64_t)n_rows + 1), 256, 0, s>>>(
      reinterpret_cast<const u64*>(d_skey), d_sidx, d_row_start, n_rows, d_key, d_val, d_id_start, ws, wd, max_off,
      min_count, d_t_group, pf_rows(HsFamilyOut::in(static_cast<char*>(d_rows), n_rows)), d_keep);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_family_write(const void* d_rows, const uint32_t* d_keep, const uint32_t* d_pos,
                                       uint32_t n_rows, bool write, const HsFamilyOut& out, uint64_t* d_grp_rows,
                                       hipStream_t s) {
  if (!n_rows || (!write && !d_grp_rows)) return hipSuccess;
  hs_pssm_family_write_kernel<<<pf_blocks(n_rows), 256, 0, s>>>(
      pf_rows(HsFamilyOut::in(static_cast<char*>(const_cast<void*>(d_rows)), n_rows)), d_keep, d_pos, n_rows,
      write ? 1 : 0, pf_rows(out), reinterpret_cast<u64*>(d_grp_rows));
  return hipGetLastError();
}

extern "C" hs_status hs_pssm_family_hits(const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                         uint64_t nm, const uint32_t* m_group, uint64_t n_groups, const uint32_t* m_off,
                                         const uint64_t* id_start, uint64_t n_seq, uint32_t min_count,
                                         const double* t_group, uint32_t* out_group, uint32_t* out_seq,
                                         int32_t* out_diag, uint32_t* out_count, double* out_sum, double* out_best_score,
                                         uint32_t* out_best_m, uint32_t* out_best_id, uint32_t* out_lo, uint32_t* out_hi,
                                         uint64_t cap, uint64_t* n_out) {
  const HsFamilyOut out{out_group,      out_seq,    out_diag,    out_count, out_sum,
                        out_best_score, out_best_m, out_best_id, out_lo,    out_hi};
  const int r = hs_pssm_family_hits_host(m, id, score, n_tuples, nm, m_group, n_groups, m_off, id_start, n_seq,
                                         min_count, t_group, out, cap, n_out);
  return r == 0 ? HS_OK : r == 1 ? HS_ERR_INVALID : r == 2 ? HS_ERR_NOMEM : HS_ERR_CAPACITY;
}

extern "C" hs_status hs_pssm_family_layout(const uint32_t* hit_x, const uint32_t* hit_y, const int32_t* hit_d,
                                           uint64_t n_hits, uint64_t nm, uint32_t* out_group, uint32_t* out_off,
                                           uint32_t* out_order, uint64_t* n_groups, uint64_t* n_conflicts) {
  const int r = hs_pssm_family_layout_host(hit_x, hit_y, hit_d, n_hits, nm, out_group, out_off, out_order, n_groups,
                                           n_conflicts);
  return r == 0 ? HS_OK : r == 1 ? HS_ERR_INVALID : HS_ERR_NOMEM;
}
