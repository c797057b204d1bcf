// hs_pssm_chain.hip -- hs_pssm_family_chain: the best gapped chain of a family's profile hits per (family, database
// sequence) on the device (include/hsearch.h), and the rule on the host (hs_pssm_family_chain_hits: hs_pssm_chain.h).
//
// Batches are cut at GROUP boundaries (hs_capi_pssm.hip), so every hit of a family lies in one batch and every
// (family, sequence) segment is complete inside it.  Per batch of nh hits sorted by m << 32 | id (the scan's own sort;
// val = the score's bits):
//   seq     the sequence of every hit: hs_pssm_seq.hip's search
//   key     hs_pssm_family.hip's key kernel without a diagonal field: g << ws | s and the hit's index (and cnt[m])
//   sort    hs_sort_pairs_u64_u32 over wg + ws bits; it is stable, so a segment's hits stay in (m, id): runs by profile,
//           off ascending inside a run
//   head    run heads of the sorted keys (hs_seqmatch.hip's kernel), their exclusive scan, the segments read back
//   start   every head lane notes where its segment starts
//   chain   one wave (a workgroup of 64) per segment:
//             gather  the lanes stride over the segment: off, m and the run starts (a ballot compaction) by position
//             levels  a run is one DP level.  Its hits go to the lanes in strides of 64; a lane visits the earlier runs
//                     in order, bisects the admissible off range and takes the best of at most 2 max_shift + 1 entries
//                     under (v, n descending, m descending, id ascending) -- a later run wins a tie, an earlier entry
//                     of one run keeps it.  The maximum is an exact comparison, so its order of evaluation does not
//                     show.  Level r + 1 reads what level r wrote: a workgroup barrier (one wave) between levels.
//             end     every lane keeps the best candidate end among its hits under (C, n descending, position
//                     ascending); the wave reduces them with shuffles through hs_pssm_topk.h's order key.
//           State (C, n, first, gaps, off, m, run starts) lies in LDS for segments of at most CH_LDS hits and in the
//           batch's global scratch otherwise (the same code over other pointers).  A segment of H hits over r runs
//           costs about H r (log H + 2 max_shift + 1) / 64 steps of one wave: a huge segment is slow by design.
//   keep    the exclusive scan of the filters' flags, the kept rows read back
//   write   one segment per lane: a kept row goes to the caller's arrays at the call's running offset plus its number
//           among the kept, and adds one to grp_rows[g]
// Scratch is sized by a batch's hits and segments.  All stores are vector stores; the penalty and the sums are single
// rounded fp64 operations (the library is built with -ffp-contract=off).
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_pssm_chain.h"

namespace {

typedef unsigned long long u64;

constexpr uint32_t CH_GRID = 1u << 22;  // workgroups of the chain kernel at most
constexpr uint32_t CH_LDS = 256;   // hits of a segment whose state fits the workgroup's LDS (7 KB)

inline unsigned pch_blocks(uint64_t n) { return (unsigned)((n + 255u) / 256u); }

// seg_start [segs + 1]: where every run of the sorted keys begins, and n
__global__ __launch_bounds__(256) void hs_pssm_chain_start_kernel(const uint32_t* __restrict__ head,
                                                                  const uint32_t* __restrict__ excl, uint32_t n,
                                                                  uint32_t* __restrict__ seg_start) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  if (i == n) seg_start[excl[n]] = n;
  else if (head[i]) seg_start[excl[i]] = i;
}

struct PchRows {
  uint32_t *group, *seq, *count, *gaps;
  double* score;
  uint32_t *first_m, *first_id, *last_m, *last_id;
  int32_t* shift;
};

struct PchArgs {
  const u64* skey;           // [n] the sorted segment keys
  const uint32_t* sidx;      // [n] their hit indices
  const uint32_t* seg_start; // [n_segs + 1]
  uint32_t n_segs;
  const uint64_t* key;       // [n] m << 32 | id, ascending
  const uint64_t* val;       // [n] the scores' bits
  const uint64_t* id_start;
  const uint32_t* m_off;
  int ws;
  uint32_t max_shift;
  double gap_open, gap_ext;
  uint32_t min_count;
  const double* t_group;
  // global state of the batch, by sorted position
  double* gC;
  uint32_t *gN, *gFirst, *gGaps, *gOff, *gM, *gRun;
};

struct PchState {
  double* C;
  uint32_t *N, *First, *Gaps, *Off, *M, *Run;
};

// the first position in [x, y) of off whose value is >= lo
__device__ __forceinline__ uint32_t pch_lower(const uint32_t* off, uint32_t x, uint32_t y, int64_t lo) {
  while (x < y) {
    const uint32_t mid = x + ((y - x) >> 1);
    if ((int64_t)off[mid] < lo) x = mid + 1;
    else y = mid;
  }
  return x;
}

// The segment [a, a + len) of the sorted pairs; st indexes by position - a.  Every lane of the wave runs every loop the
// same number of times (the barriers are uniform); a lane without a hit only skips the body.
__device__ __forceinline__ void pch_segment(const PchArgs& A, const PchState& st, uint32_t a, uint32_t len, uint32_t g,
                                            uint32_t s, const PchRows& rows, uint32_t* __restrict__ keep, uint32_t seg) {
  const uint32_t lane = threadIdx.x;
  const uint64_t base = A.id_start[s];
  // gather: off, m and the run starts
  uint32_t n_runs = 0;
  for (uint32_t p0 = 0; p0 < len; p0 += 64) {
    const uint32_t p = p0 + lane;
    bool head = false;
    if (p < len) {
      const uint64_t kk = A.key[A.sidx[a + p]];
      const uint32_t m = (uint32_t)(kk >> 32);
      st.Off[p] = (uint32_t)((uint64_t)(uint32_t)kk - base);
      st.M[p] = m;
      head = p == 0 || (uint32_t)(A.key[A.sidx[a + p - 1]] >> 32) != m;
    }
    const u64 mask = __ballot(head);
    if (head) st.Run[n_runs + __popcll(mask & ((1ull << lane) - 1ull))] = p;
    n_runs += (uint32_t)__popcll(mask);
  }
  __syncthreads();
  // the levels
  double eC = 0.0;
  uint32_t eN = 0, eP = 0xffffffffu;  // this lane's best candidate end
  const double tg = A.t_group ? A.t_group[g] : 0.0;
  for (uint32_t r = 0; r < n_runs; ++r) {
    const uint32_t rs = st.Run[r], re = r + 1 < n_runs ? st.Run[r + 1] : len;
    const int64_t moff_i = (int64_t)A.m_off[st.M[rs]];
    for (uint32_t p0 = rs; p0 < re; p0 += 64) {
      const uint32_t i = p0 + lane;
      if (i < re) {
        const uint32_t off_i = st.Off[i];
        const int64_t diag_i = (int64_t)off_i - moff_i;
        double bv = 0.0;
        uint32_t bj = 0xffffffffu, bn = 0, bd = 0;
        for (uint32_t q = 0; q < r; ++q) {
          const uint32_t qs = st.Run[q], qe = st.Run[q + 1];
          const int64_t moff = (int64_t)A.m_off[st.M[qs]];
          const int64_t lo0 = diag_i - (int64_t)A.max_shift + moff, hi0 = diag_i + (int64_t)A.max_shift + moff;
          const int64_t lo = lo0 < 0 ? 0 : lo0, hi = hi0 < (int64_t)off_i - 1 ? hi0 : (int64_t)off_i - 1;
          if (hi < lo) continue;
          for (uint32_t j = pch_lower(st.Off, qs, qe, lo); j < qe; ++j) {
            const int64_t off_j = (int64_t)st.Off[j];
            if (off_j > hi) break;
            const int64_t dd = diag_i - (off_j - moff);
            const uint32_t d = (uint32_t)(dd < 0 ? -dd : dd);
            double v = st.C[j];
            if (d) {
              const double step = A.gap_ext * (double)d;
              const double pen = A.gap_open + step;
              v = v - pen;
            }
            if (!(v > 0.0)) continue;
            const uint32_t nj = st.N[j];
            // q ascends, so an equal (v, n) of a later run wins; inside a run the earlier entry keeps a tie
            if (bj == 0xffffffffu || v > bv || (v == bv && (nj > bn || (nj == bn && bj < qs)))) {
              bv = v;
              bj = j;
              bn = nj;
              bd = d;
            }
          }
        }
        const double sc = __longlong_as_double((long long)A.val[A.sidx[a + i]]);
        double Ci;
        uint32_t Ni;
        if (bj != 0xffffffffu) {
          Ci = bv + sc;
          Ni = bn + 1;
          st.First[i] = st.First[bj];
          st.Gaps[i] = st.Gaps[bj] + (bd ? 1u : 0u);
        } else {
          Ci = 0.0 + sc;
          Ni = 1;
          st.First[i] = i;
          st.Gaps[i] = 0;
        }
        st.C[i] = Ci;
        st.N[i] = Ni;
        if (Ni >= A.min_count && (!A.t_group || Ci >= tg)) {
          // this lane's positions ascend, so an equal (C, n) keeps the earlier one
          if (eP == 0xffffffffu || Ci > eC || (Ci == eC && Ni > eN)) {
            eC = Ci;
            eN = Ni;
            eP = i;
          }
        }
      }
    }
    __syncthreads();  // level r + 1 reads what level r wrote (LDS or global: one workgroup)
  }
  // the end: the best (C descending, n descending, position ascending) over the lanes; no candidate: key 0 (a NaN's,
  // which no C has)
  u64 eU = eP == 0xffffffffu ? 0ull : hs_pssm_order_key((u64)__double_as_longlong(eC));
  for (int x = 32; x >= 1; x >>= 1) {
    const uint32_t oh = __shfl_xor((uint32_t)(eU >> 32), x, 64), ol = __shfl_xor((uint32_t)eU, x, 64);
    const uint32_t oN = __shfl_xor(eN, x, 64), oP = __shfl_xor(eP, x, 64);
    const u64 oU = ((u64)oh << 32) | ol;
    if (oU > eU || (oU == eU && (oN > eN || (oN == eN && oP < eP)))) {
      eU = oU;
      eN = oN;
      eP = oP;
    }
  }
  if (lane == 0) {
    const bool has = eP != 0xffffffffu;
    keep[seg] = has ? 1u : 0u;
    if (has) {
      const uint32_t f = st.First[eP];
      const uint64_t kf = A.key[A.sidx[a + f]], ke = A.key[A.sidx[a + eP]];
      const int64_t diag_f = (int64_t)st.Off[f] - (int64_t)A.m_off[(uint32_t)(kf >> 32)];
      const int64_t diag_e = (int64_t)st.Off[eP] - (int64_t)A.m_off[(uint32_t)(ke >> 32)];
      rows.group[seg] = g;
      rows.seq[seg] = s;
      rows.count[seg] = eN;
      rows.gaps[seg] = st.Gaps[eP];
      rows.score[seg] = st.C[eP];
      rows.first_m[seg] = (uint32_t)(kf >> 32);
      rows.first_id[seg] = (uint32_t)kf;
      rows.last_m[seg] = (uint32_t)(ke >> 32);
      rows.last_id[seg] = (uint32_t)ke;
      rows.shift[seg] = (int32_t)(diag_e - diag_f);
    }
  }
}

// One workgroup of one wave per segment (a grid-stride loop above CH_GRID segments).  keep [n_segs + 1]: whether the segment reports a row, and 0 behind the last
// (its scan slot receives the kept rows).
__global__ __launch_bounds__(64) void hs_pssm_chain_kernel(PchArgs A, PchRows rows, uint32_t* __restrict__ keep) {
  __shared__ double sC[CH_LDS];
  __shared__ uint32_t sN[CH_LDS], sFirst[CH_LDS], sGaps[CH_LDS], sOff[CH_LDS], sM[CH_LDS], sRun[CH_LDS + 1];
  for (uint32_t seg = blockIdx.x; seg <= A.n_segs; seg += gridDim.x) {
    if (seg == A.n_segs) {
      if (threadIdx.x == 0) keep[seg] = 0;
      break;
    }
    const uint32_t a = A.seg_start[seg], len = A.seg_start[seg + 1] - a;
    const u64 gs = A.skey[a];
    const uint32_t s = (uint32_t)(gs & ((1ull << A.ws) - 1ull)), g = (uint32_t)(gs >> A.ws);  // ws <= 32
    if (len <= CH_LDS) {
      const PchState st{sC, sN, sFirst, sGaps, sOff, sM, sRun};
      pch_segment(A, st, a, len, g, s, rows, keep, seg);
    } else {
      // (a + len <= n: the segment's slice of the batch's state)
      const PchState st{A.gC + a, A.gN + a, A.gFirst + a, A.gGaps + a, A.gOff + a, A.gM + a, A.gRun + a};
      pch_segment(A, st, a, len, g, s, rows, keep, seg);
    }
    __syncthreads();  // lane 0 has read the state before the next segment overwrites it
  }
}

// kept segment r -> slot pos[r] of the output (write != 0), and grp_rows[g] += 1
__global__ __launch_bounds__(256) void hs_pssm_chain_write_kernel(PchRows rows, const uint32_t* __restrict__ keep,
                                                                  const uint32_t* __restrict__ pos, uint32_t n_segs,
                                                                  int write, PchRows out, u64* __restrict__ grp_rows) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_segs || !keep[r]) return;
  if (grp_rows) atomicAdd(grp_rows + rows.group[r], 1ull);
  if (!write) return;
  const uint32_t at = pos[r];
  out.group[at] = rows.group[r];
  out.seq[at] = rows.seq[r];
  out.count[at] = rows.count[r];
  out.gaps[at] = rows.gaps[r];
  out.score[at] = rows.score[r];
  out.first_m[at] = rows.first_m[r];
  out.first_id[at] = rows.first_id[r];
  out.last_m[at] = rows.last_m[r];
  out.last_id[at] = rows.last_id[r];
  out.shift[at] = rows.shift[r];
}

PchRows pch_rows(const HsChainOut& o) {
  return PchRows{o.group, o.seq, o.count, o.gaps, o.score, o.first_m, o.first_id, o.last_m, o.last_id, o.shift};
}

}  // namespace

size_t hs_pssm_chain_state_bytes(uint32_t n) { return ((size_t)n + 2) * 32; }

hipError_t hs_launch_pssm_chain(const uint64_t* d_skey, const uint32_t* d_sidx, const uint32_t* d_head,
                                const uint32_t* d_excl, uint32_t n, uint32_t n_segs, const uint64_t* d_key,
                                const uint64_t* d_val, const uint64_t* d_id_start, const uint32_t* d_m_off, int ws,
                                uint32_t max_shift, double gap_open, double gap_ext, uint32_t min_count,
                                const double* d_t_group, uint32_t* d_seg_start, void* d_state, void* d_rows,
                                uint32_t* d_keep, hipStream_t s) {
  if (!n || !n_segs) return hipSuccess;
  hs_pssm_chain_start_kernel<<<pch_blocks((uint64_t)n + 1), 256, 0, s>>>(d_head, d_excl, n, d_seg_start);
  PchArgs A;
  A.skey = reinterpret_cast<const u64*>(d_skey);
  A.sidx = d_sidx;
  A.seg_start = d_seg_start;
  A.n_segs = n_segs;
  A.key = d_key;
  A.val = d_val;
  A.id_start = d_id_start;
  A.m_off = d_m_off;
  A.ws = ws;
  A.max_shift = max_shift;
  A.gap_open = hs_pssm_chain_zero(gap_open);
  A.gap_ext = hs_pssm_chain_zero(gap_ext);
  A.min_count = min_count;
  A.t_group = d_t_group;
  // the state of hs_pssm_chain_state_bytes(n): C [n + 2], then six 32-bit arrays of n + 2 each
  const size_t e = (size_t)n + 2;
  A.gC = static_cast<double*>(d_state);
  uint32_t* const w = reinterpret_cast<uint32_t*>(A.gC + e);
  A.gN = w;
  A.gFirst = w + e;
  A.gGaps = w + 2 * e;
  A.gOff = w + 3 * e;
  A.gM = w + 4 * e;
  A.gRun = w + 5 * e;
  hs_pssm_chain_kernel<<<(unsigned)std::min<uint64_t>((uint64_t)n_segs + 1, CH_GRID), 64, 0, s>>>(A, pch_rows(HsChainOut::in(static_cast<char*>(d_rows), n_segs)),
                                                 d_keep);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_chain_write(const void* d_rows, const uint32_t* d_keep, const uint32_t* d_pos, uint32_t n_segs,
                                      bool write, const HsChainOut& out, uint64_t* d_grp_rows, hipStream_t s) {
  if (!n_segs || (!write && !d_grp_rows)) return hipSuccess;
  hs_pssm_chain_write_kernel<<<pch_blocks(n_segs), 256, 0, s>>>(
      pch_rows(HsChainOut::in(static_cast<char*>(const_cast<void*>(d_rows)), n_segs)), d_keep, d_pos, n_segs,
      write ? 1 : 0, pch_rows(out), reinterpret_cast<u64*>(d_grp_rows));
  return hipGetLastError();
}

extern "C" hs_status hs_pssm_family_chain_hits(const uint32_t* m, const uint32_t* id, const double* score,
                                               uint64_t n_tuples, uint64_t nm, const uint32_t* m_group,
                                               uint64_t n_groups, const uint32_t* m_off, const uint64_t* id_start,
                                               uint64_t n_seq, uint32_t max_shift, double gap_open, double gap_ext,
                                               uint32_t min_count, const double* t_group, uint32_t* out_group,
                                               uint32_t* out_seq, uint32_t* out_count, uint32_t* out_gaps,
                                               double* out_score, uint32_t* out_first_m, uint32_t* out_first_id,
                                               uint32_t* out_last_m, uint32_t* out_last_id, int32_t* out_shift,
                                               uint64_t cap, uint64_t* n_out, uint64_t* out_path_start,
                                               uint32_t* out_path_m, uint32_t* out_path_id, uint64_t path_cap,
                                               uint64_t* n_path) {
  const HsChainOut out{out_group,   out_seq,      out_count,  out_gaps,    out_score,
                       out_first_m, out_first_id, out_last_m, out_last_id, out_shift};
  HsChainPath path;
  path.start = out_path_start;
  path.m = out_path_m;
  path.id = out_path_id;
  path.cap = path_cap;
  path.n_path = n_path;
  const int r = hs_pssm_family_chain_hits_host(m, id, score, n_tuples, nm, m_group, n_groups, m_off, id_start, n_seq,
                                               max_shift, gap_open, gap_ext, min_count, t_group, out, cap, n_out, path);
  return r == 0 ? HS_OK : r == 1 ? HS_ERR_INVALID : r == 2 ? HS_ERR_NOMEM : HS_ERR_CAPACITY;
}
