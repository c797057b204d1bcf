// hs_pssm_seq.hip -- hs_pssm_seq_scan: a profile scan's hits reduced per (profile, database sequence) on the device
// (include/hsearch.h), and the same rule on the host for any list of tuples (hs_pssm_seq_hits; the rule: hs_pssm_seq.h).
//
// What makes this sink simpler than hs_seqmatch.hip's.  Batches are cut by PROFILE, so every hit of a profile lies in
// one batch (after a survivor split too: the same profiles run again in smaller batches), and a sequence owns a
// contiguous id range.  After the scan's own sort on m << 32 | id every row (m, s) is therefore one contiguous run, the
// runs lie in output order, and the batches' rows follow one another: no second sort, no row list on the handle, no
// merge at the end of the call.  Per batch of nh sorted hits (key = m << 32 | id, val = the score's bits):
//   seq     one hit per lane: s by a search in id_start whose top 8 levels are 256 samples staged in LDS per workgroup
//           (hs_seqmatch.hip's search: the global part is log2(n_seq / 256) dependent loads)
//   head    head[i] = hit i's (m, s) differs from its predecessor's; the caller's exclusive scan numbers the batch's
//           rows and its total is read back (rows are written only while the call's running total fits cap)
//   reduce  a row is a run sorted by id: its length is the count, its first and last elements give lo and hi, so every
//           head lane only notes where its run starts (row_start).  The best (score, id) alone is reduced: a segmented
//           inclusive scan over __shfl_up (six steps) carries (ascending score key, id) along runs of one row number.
//           Only a lane that ENDS its run -- inside the wave or at lane 63 -- touches memory: a run that lies whole
//           inside the wave is stored plainly, a run cut by a wave's edge takes atomicMax of the key and leaves
//           (row, key, id) in one of the wave's two partial slots.  One row holding a whole batch costs one atomic per
//           wave, never one lane per row.
//   best    behind the kernel boundary every slot's key is final: the partials whose key IS the slot's take atomicMin
//           of the id (the two-step rule of hs_annotate.hip / hs_seqmatch.hip for a best that fits no single atomic)
//   write   one row per lane, straight into the caller's arrays at the call's running offset; cnt and seq_cnt take
//           one atomic add per row.  Without room for the rows only the counts are taken (reduce and best do not run).
// Scratch is sized by a batch's hits and rows.  All stores are vector stores.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_pssm_seq.h"

namespace {

typedef unsigned long long u64;

#define PS_NO_ROW 0xffffffffu
#define PS_SAMPLES 256u

inline unsigned ps_blocks(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

// s with id_start[s] <= id < id_start[s + 1] for the id of every hit (id < id_start[n_seq] = n: every id of the index
// is); the samples are id_start[min(t stride, n_seq)], t = 0 .. 255; equal neighbours leave the LAST s at or below id
__global__ __launch_bounds__(256) void hs_pssm_seq_kernel(const uint64_t* __restrict__ key, uint32_t n,
                                                          const uint64_t* __restrict__ id_start, u64 n_seq,
                                                          uint32_t stride, uint32_t* __restrict__ seq) {
  __shared__ uint32_t sample[PS_SAMPLES];
  {
    const u64 at = min((u64)threadIdx.x * stride, n_seq);
    sample[threadIdx.x] = (uint32_t)min(id_start[at], (uint64_t)0xffffffffu);
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t id = (uint32_t)key[i];
  uint32_t a = 0, b = PS_SAMPLES;  // sample[a] <= id (sample[0] = 0), sample[b] > id or b = 256
  while (b - a > 1) {
    const uint32_t m = (a + b) >> 1;
    if (sample[m] <= id) a = m; else b = m;
  }
  u64 lo = min((u64)a * stride, n_seq), hi = min(((u64)a + 1) * stride, n_seq);
  if (lo >= hi) lo = hi ? hi - 1 : 0;  // (an id at or past id_start[n_seq]: cannot happen, and reads nothing out of bounds)
  while (hi - lo > 1) {
    const u64 m = (lo + hi) >> 1;
    if (id_start[m] <= (uint64_t)id) lo = m; else hi = m;
  }
  seq[i] = (uint32_t)lo;
}

// head[i], i < n: hit i starts a row; head[n] = 0 (its scan slot receives the number of rows)
__global__ __launch_bounds__(256) void hs_pssm_seq_head_kernel(const uint64_t* __restrict__ key,
                                                               const uint32_t* __restrict__ seq, uint32_t n,
                                                               uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  head[i] = i < n && (i == 0 || (key[i] >> 32) != (key[i - 1] >> 32) || seq[i] != seq[i - 1]) ? 1u : 0u;
}

// rows [0, n) to the state the atomics start from: no key (an ascending key of 0 would be a NaN's), no id
__global__ __launch_bounds__(256) void hs_pssm_seq_fill_kernel(uint32_t n, u64* __restrict__ row_key,
                                                               uint32_t* __restrict__ row_id) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  row_key[i] = 0;
  row_id[i] = 0xffffffffu;
}

// Sorted hit i per lane, row excl[i] + head[i] - 1.  row_start [rows + 1]: where every row's run begins, and n.
// best != 0: the rows' best (key, id) too.  part_* [2 x waves]: the wave's cut runs (slot 2w: the run that came in over
// lane 0, slot 2w + 1: the run that leaves over lane 63), PS_NO_ROW where there is none.
__global__ __launch_bounds__(256) void hs_pssm_seq_reduce_kernel(const uint64_t* __restrict__ key,
                                                                 const uint64_t* __restrict__ val,
                                                                 const uint32_t* __restrict__ head,
                                                                 const uint32_t* __restrict__ excl, uint32_t n, int best,
                                                                 uint32_t* __restrict__ row_start,
                                                                 u64* __restrict__ row_key, uint32_t* __restrict__ row_id,
                                                                 uint32_t* __restrict__ part_row,
                                                                 u64* __restrict__ part_key,
                                                                 uint32_t* __restrict__ part_id) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = i >> 6;
  const bool valid = i < n;
  uint32_t r = PS_NO_ROW, id = 0xffffffffu;
  u64 u = 0;
  bool hh = false, tail = false;
  if (valid) {
    const uint32_t hd = head[i];
    r = excl[i] + hd - 1u;
    hh = hd != 0;
    tail = i + 1 >= n || head[i + 1] != 0;
    if (hh) row_start[r] = i;
    if (i + 1 >= n) row_start[r + 1] = n;
    if (best) {
      u = hs_pssm_order_key(val[i]);
      id = (uint32_t)key[i];
    }
  }
  if (!best) return;  // (uniform: a kernel argument)
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const uint32_t r2 = __shfl_up(r, m, 64), id2 = __shfl_up(id, m, 64);
    const u64 u2 = __shfl_up(u, m, 64);
    const int hh2 = __shfl_up((int)hh, m, 64);
    if (lane >= (uint32_t)m && r2 == r && valid) {
      if (u2 > u || (u2 == u && id2 < id)) {
        u = u2;
        id = id2;
      }
      hh = hh || hh2 != 0;
    }
  }
  const bool cut_in = valid && tail && !hh;            // came in over lane 0, ends here
  const bool cut_out = valid && lane == 63u && !tail;  // leaves over lane 63 (it may have come in over lane 0 too)
  if (valid && tail && hh) {
    row_key[r] = u;
    row_id[r] = id;
  } else if (cut_in || cut_out) {
    atomicMax(row_key + r, u);
    const uint32_t slot = 2u * wave + (cut_out ? 1u : 0u);
    part_row[slot] = r;
    part_key[slot] = u;
    part_id[slot] = id;
  }
  // (a wave has at most one lane of each kind; the slot nobody claimed is marked by lane 0)
  const bool any_in = __ballot(cut_in) != 0ull, any_out = __ballot(cut_out) != 0ull;
  if (lane == 0 && valid) {
    if (!any_in) part_row[2u * wave] = PS_NO_ROW;
    if (!any_out) part_row[2u * wave + 1u] = PS_NO_ROW;
  }
}

// every slot's key is final (the reduce kernel has ended): the cut runs AT that key compete for the slot's id
__global__ __launch_bounds__(256) void hs_pssm_seq_best_kernel(const uint32_t* __restrict__ part_row,
                                                               const u64* __restrict__ part_key,
                                                               const uint32_t* __restrict__ part_id, uint32_t n_part,
                                                               uint32_t n_rows, const u64* __restrict__ row_key,
                                                               uint32_t* __restrict__ row_id) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_part) return;
  const uint32_t r = part_row[p];
  if (r >= n_rows) return;
  if (row_key[r] == part_key[p]) atomicMin(row_id + r, part_id[p]);
}

// row r per lane: the counts, and with write != 0 the row
__global__ __launch_bounds__(256) void hs_pssm_seq_write_kernel(const uint64_t* __restrict__ key,
                                                                const uint32_t* __restrict__ seq,
                                                                const uint32_t* __restrict__ row_start,
                                                                const u64* __restrict__ row_key,
                                                                const uint32_t* __restrict__ row_id, uint32_t n_rows,
                                                                const uint64_t* __restrict__ id_start, int write,
                                                                uint32_t* __restrict__ out_m, uint32_t* __restrict__ out_seq,
                                                                uint32_t* __restrict__ out_count,
                                                                double* __restrict__ out_best_score,
                                                                uint32_t* __restrict__ out_best_id,
                                                                uint32_t* __restrict__ out_lo, uint32_t* __restrict__ out_hi,
                                                                u64* __restrict__ cnt, u64* __restrict__ seq_cnt) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_rows) return;
  const uint32_t a = row_start[r], b = row_start[r + 1];
  const uint64_t ka = key[a];
  const uint32_t m = (uint32_t)(ka >> 32), s = seq[a];
  if (cnt) atomicAdd(cnt + m, (u64)(b - a));
  if (seq_cnt) atomicAdd(seq_cnt + m, 1ull);
  if (!write) return;
  const uint64_t base = id_start[s];
  out_m[r] = m;
  out_seq[r] = s;
  out_count[r] = b - a;
  out_best_score[r] = __longlong_as_double((long long)hs_pssm_order_bits(row_key[r]));
  out_best_id[r] = row_id[r];
  out_lo[r] = (uint32_t)((uint64_t)(uint32_t)ka - base);
  out_hi[r] = (uint32_t)((uint64_t)(uint32_t)key[b - 1] - base);
}

}  // namespace

hipError_t hs_launch_pssm_seq_head(const uint64_t* d_key, uint32_t n, const uint64_t* d_id_start, uint64_t n_seq,
                                   uint32_t* d_seq, uint32_t* d_head, hipStream_t s) {
  if (!n) return hipSuccess;
  const uint32_t stride = (uint32_t)((n_seq + PS_SAMPLES) / PS_SAMPLES);  // ceil((n_seq + 1) / 256)
  hs_pssm_seq_kernel<<<ps_blocks(n), 256, 0, s>>>(d_key, n, d_id_start, n_seq, stride, d_seq);
  hs_pssm_seq_head_kernel<<<ps_blocks((uint64_t)n + 1), 256, 0, s>>>(d_key, d_seq, n, d_head);
  return hipGetLastError();
}

// the search alone (hs_pssm_family.hip keys its rows on more than the sequence and finds its own heads)
hipError_t hs_launch_pssm_seq_of(const uint64_t* d_key, uint32_t n, const uint64_t* d_id_start, uint64_t n_seq,
                                 uint32_t* d_seq, hipStream_t s) {
  if (!n) return hipSuccess;
  const uint32_t stride = (uint32_t)((n_seq + PS_SAMPLES) / PS_SAMPLES);
  hs_pssm_seq_kernel<<<ps_blocks(n), 256, 0, s>>>(d_key, n, d_id_start, n_seq, stride, d_seq);
  return hipGetLastError();
}

size_t hs_pssm_seq_part_bytes(uint32_t n) { return (size_t)2 * ((n + 63u) / 64u) * 16 + 16; }

hipError_t hs_launch_pssm_seq_rows(const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_seq,
                                   const uint32_t* d_head, const uint32_t* d_excl, uint32_t n, uint32_t n_rows,
                                   const uint64_t* d_id_start, bool write, uint32_t* d_row_start, uint64_t* d_row_key,
                                   uint32_t* d_row_id, void* d_part, uint32_t* d_out_m, uint32_t* d_out_seq,
                                   uint32_t* d_out_count, double* d_out_best_score, uint32_t* d_out_best_id,
                                   uint32_t* d_out_lo, uint32_t* d_out_hi, uint64_t* d_cnt, uint64_t* d_seq_cnt,
                                   hipStream_t s) {
  if (!n || !n_rows) return hipSuccess;
  const uint32_t n_part = 2u * ((n + 63u) / 64u);
  u64* const row_key = reinterpret_cast<u64*>(d_row_key);
  u64* const part_key = static_cast<u64*>(d_part);
  uint32_t* const part_id = reinterpret_cast<uint32_t*>(part_key + n_part);
  uint32_t* const part_row = part_id + n_part;
  if (write) hs_pssm_seq_fill_kernel<<<ps_blocks(n_rows), 256, 0, s>>>(n_rows, row_key, d_row_id);
  hs_pssm_seq_reduce_kernel<<<ps_blocks(n), 256, 0, s>>>(d_key, d_val, d_head, d_excl, n, write ? 1 : 0, d_row_start,
                                                         row_key, d_row_id, part_row, part_key, part_id);
  if (write)
    hs_pssm_seq_best_kernel<<<ps_blocks(n_part), 256, 0, s>>>(part_row, part_key, part_id, n_part, n_rows, row_key,
                                                              d_row_id);
  hs_pssm_seq_write_kernel<<<ps_blocks(n_rows), 256, 0, s>>>(d_key, d_seq, d_row_start, row_key, d_row_id, n_rows,
                                                             d_id_start, write ? 1 : 0, d_out_m, d_out_seq, d_out_count,
                                                             d_out_best_score, d_out_best_id, d_out_lo, d_out_hi,
                                                             reinterpret_cast<u64*>(d_cnt),
                                                             reinterpret_cast<u64*>(d_seq_cnt));
  return hipGetLastError();
}

extern "C" hs_status hs_pssm_seq_hits(const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                      uint64_t nm, const uint64_t* id_start, uint64_t n_seq, uint32_t* out_m,
                                      uint32_t* out_seq, uint32_t* out_count, double* out_best_score,
                                      uint32_t* out_best_id, uint32_t* out_lo, uint32_t* out_hi, uint64_t cap,
                                      uint64_t* n_out) {
  const int r = hs_pssm_seq_hits_host(m, id, score, n_tuples, nm, id_start, n_seq, out_m, out_seq, out_count,
                                      out_best_score, out_best_id, out_lo, out_hi, cap, n_out);
  return r == 0 ? HS_OK : r == 1 ? HS_ERR_INVALID : r == 2 ? HS_ERR_NOMEM : HS_ERR_CAPACITY;
}
