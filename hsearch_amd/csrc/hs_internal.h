// hs_internal.h -- declarations shared by the translation units of libhsearch_amd.so.
// gfx950 (MI355X) only; no CPU fallback anywhere in this directory.
#ifndef HS_INTERNAL_H
#define HS_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/hsearch.h"

#define HS_MAX_L 32
#define HS_MAX_K 32
#define HS_ALPHABET_PAD 32  // table rows addressable by a 5-bit residue code
#define HS_TROW 32          // floats per row of a per-query distance table (20 used)
// survivor entries {probe, entry position}: probe = q_local * L + table, or -- from the join
// kernels -- HS_PROV_INDIRECT | position of the probe in segment order (index into sorted_ql)
#define HS_PROV_INDIRECT 0x80000000u
#define HS_SLICE 4096u      // candidates one wavefront scans per work item
#define HS_KEY_CHARS (11 * HS_MAX_K + 1)

#include "hs_key.h"

// ---- device view of one hash table --------------------------------------------------------------
// The survivor list's counter is 32 bits (the batch's counters block, word 0).  A batch whose filters
// pass more than ~4e9 pairs (a radius close to the typical distance of bucket mates) would wrap it
// silently: every reservation that lands in the last 2^28 slots raises HS_CNT_SURVIVOR_OVERFLOW in
// the same block -- reservations are <= 256 slots (hs_join8.hip JRES), so one does before the counter
// wraps -- and the host repeats the batch in halves (hs_capi.hip run_query).
#define HS_CNT_SURVIVOR_OVERFLOW 21
// hs_query_codes: a query's residue code lay outside the alphabet (hs_check_codes_kernel)
#define HS_CNT_BAD_QUERY_CODE 22
// Words of the counter block that hold what the host reads after a pass and no kernel counts in: written by
// the kernels that produce the values, so that ONE copy of the block brings everything back (they were four).
// Behind the item counters (words 32..47), which a repeated pass clears; cleared by the batch's reset only.
#define HS_CNT_PROJ 48   // [2] the MFMA projection of the batch's queries: {slots reserved, values flagged}
#define HS_CNT_SPLIT 50  // [2] hs_item_desc_kernel: first item of the few-query class, items (the real count)
#define HS_CNT_WORDS 64  // words of the block, all read back
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t hs_reserve_survivors(uint32_t* prov_count, uint32_t n) {
  const uint32_t base = atomicAdd(prov_count, n);
  if (base >= 0xF0000000u) atomicOr(prov_count + HS_CNT_SURVIVOR_OVERFLOW, 1u);
  return base;
}
#endif

struct hs_table_dev {
  const uint64_t* dir_key;   // [nb] sorted fingerprints of the distinct keys
  const uint32_t* dir_start; // [nb+1] first sorted position of each bucket
  const int32_t* dir_tuple;  // [nb][K] bucket ints of the bucket's first member
  const uint4* packed;       // [n][PW] 5-bit packed residue codes in bucket order
  const uint32_t* ids;       // [n] DB ids in bucket order (ascending inside a bucket)
  const uint32_t* pos_of;    // [n] inverse of ids: sorted position of DB id i in this table
  const uint32_t* dir_jump;  // [2^J + 1] first directory entry whose fingerprint's top J bits are >= the slot
  const uint64_t* giant_key; // [n_giant] ascending TUPLE HASHES (hs_tuple_hash of the bucket ints) of the buckets with
  uint32_t n_giant;          // more than hs_giant_threshold members (bucket partition: shared among the parts by QUERY)
  const uint4* dir_rec;      // [nb][4] or null: one 64-byte line per bucket with all a probe reads of it --
                             // {fingerprint, start, count} and the K <= HS_REC_MAX_K bucket ints as int16
                             // (null: K larger, an int outside 16 bits, or the option is off)
  uint32_t nb;
  uint32_t jump_shift;       // 64 - J
};
struct hs_tables_dev {
  hs_table_dev t[HS_MAX_L];
  // bucket partition (hs_set_bucket_partition): the probe kernel looks only for the (query, bucket) probes
  // that fall to `part` of `n_parts` (hs_probe_part); n_parts <= 1: all of them.  q_first: number, in the
  // call, of the batch's first query.  probe_list != null: the kernel probes these n_list (query, table) pairs
  // only -- the part's own, found ahead of it (hs_launch_part_owned).
  uint32_t part, n_parts, q_first;
  const uint32_t* probe_list;
  uint32_t n_list;
  // multi-probe (hs_set_multiprobe): probe_valid[ql] == 0 marks an empty probe, which finds no bucket; null: all valid
  const uint8_t* probe_valid = nullptr;
};
// A cheap hash of a probe's K bucket ints (t[0], t[stride], ...): what decides the part of a probe.  (Not the
// key fingerprint: that one walks the decimal characters of every int, ~ 10 x the instructions, and seven
// probes in eight of a batch belong to other parts.  Tuples whose key STRINGS coincide may fall to different
// parts -- each probe still belongs to exactly one.)
__host__ __device__ inline uint64_t hs_tuple_hash(const int32_t* t, int K, int stride) {
  uint64_t h = 0x243f6a8885a308d3ull;
  for (int j = 0; j < K; ++j) {
    h = (h ^ (uint32_t)t[(size_t)j * stride]) * 0x9e3779b97f4a7c15ull;
    h ^= h >> 29;
  }
  return h;
}
// The part a probe belongs to, of n_parts: a function of its bucket ints -- every rank the same answer, the
// parts even whatever the tables look like -- and, for the few GIANT buckets alone, of the query's number in
// the call as well: a table's largest buckets each hold per cents of all (member, query) pairs (configs[2]:
// 600 buckets of > 10^5 members hold half of them), and whole they would land on the parts like rocks; shared
// by query every part gets its n-th of each.
__host__ __device__ inline uint32_t hs_probe_part(uint64_t tuple_hash, bool giant, uint32_t q, uint32_t n_parts) {
  if (giant) tuple_hash ^= (uint64_t)(q + 1u) * 0x9e3779b97f4a7c15ull;
  return (uint32_t)(((tuple_hash >> 20) & 0xffffffffull) % n_parts);
}
// more members than this make a bucket a giant (n = k-mers of the index)
static inline uint32_t hs_giant_threshold(uint64_t n) { return (uint32_t)(n / 1024 > 4096 ? n / 1024 : 4096); }

// ---- per-query radii (hs_query_radii) ----------------------------------------------------------------
// The fp32 filters' bound for a squared radius r2 >= 0: the smallest float >= r2 (1 + 1e-5), then one more
// ulp -- one-sided, the bound must never undercut.  The same value on the host (a call's one radius) and on the
// device (a query's own radius).
__host__ __device__ inline float hs_filter_bound(double r2) {
  const double hi = r2 * (1.0 + 1e-5) + 1e-30;
  float f = (float)hi;  // (round to nearest; +inf from 2^128 on)
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((double)f < hi) ++u;      // f >= 0 and finite here: the next float up is the next bit pattern
  if (u < 0x7f800000u) ++u;
  memcpy(&f, &u, 4);
  return f;
}
// The squared radius of query q: radii == null, the call's one R * R (r2); else radii[q] * radii[q], rounded
// once like it (motif_both_points.cpp:204)
__host__ __device__ inline double hs_r2_of(const double* radii, uint32_t q, double r2) {
  return radii ? radii[q] * radii[q] : r2;
}

// 16-byte words per packed k-mer
// 25 residues x 5 bits per 16-byte word
static inline int hs_packed_words(int k) { return (k + 24) / 25; }

// ---- primitive wrappers (hs_prims.hip, rocPRIM behind them) --------------------------------------
size_t hs_sort_pairs_u64_u32_temp(size_t n);
// keys ordered by their bits [begin_bit, end_bit) only; begin_bit > 0 is refused (hipErrorInvalidValue)
// unless hs_sort_partial_bits_ok(n): only rocPRIM's onesweep path handles such a range (hs_prims.hip)
bool hs_sort_partial_bits_ok(size_t n);
hipError_t hs_sort_pairs_u64_u32(void* temp, size_t temp_bytes, const uint64_t* kin, uint64_t* kout,
                                 const uint32_t* vin, uint32_t* vout, size_t n, int begin_bit, int end_bit,
                                 hipStream_t s);
size_t hs_sort_pairs_u32_u32_temp(size_t n);
hipError_t hs_sort_pairs_u32_u32(void* temp, size_t temp_bytes, const uint32_t* kin, uint32_t* kout,
                                 const uint32_t* vin, uint32_t* vout, size_t n, int end_bit, hipStream_t s);
size_t hs_sort_keys_u32_temp(size_t n);
hipError_t hs_sort_keys_u32(void* temp, size_t temp_bytes, const uint32_t* kin, uint32_t* kout, size_t n, int end_bit,
                            hipStream_t s);
size_t hs_sort_pairs_u64_u64_temp(size_t n);
hipError_t hs_sort_pairs_u64_u64(void* temp, size_t temp_bytes, const uint64_t* kin, uint64_t* kout,
                                 const uint64_t* vin, uint64_t* vout, size_t n, int end_bit,
                                 hipStream_t s);
size_t hs_scan_u32_temp(size_t n);  // (workspace of any of the scans below over n elements)
// two 32-bit scans in one: the halves of the 64-bit sums (the low one must stay below 2^32)
hipError_t hs_exclusive_scan_u64(void* temp, size_t temp_bytes, const uint64_t* in, uint64_t* out, size_t n,
                                 hipStream_t s);
// out[i] = sum of in[j] | (number of in[j] != 0) << 32 over j < i
hipError_t hs_exclusive_scan_count_flag(void* temp, size_t temp_bytes, const uint32_t* in, uint64_t* out, size_t n,
                                        hipStream_t s);
hipError_t hs_exclusive_scan_u32(void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out,
                                 size_t n, hipStream_t s);
size_t hs_rle_u64_temp(size_t n);
// unique_out[n], counts_out[n], runs_out[1] (device)
hipError_t hs_rle_u64(void* temp, size_t temp_bytes, const uint64_t* in, uint64_t* unique_out,
                      uint32_t* counts_out, uint32_t* runs_out, size_t n, hipStream_t s);

// ---- grouping a table's k-mers by key without sorting fingerprints (hs_group.hip) -----------------
// bucket ints -> slots of an open-addressing table d_table[C] of 64-bit fingerprints (C =
// hs_group_table_slots(n) slots): d_slot_of[i] = slot of k-mer i's key.  *d_flag |= 16: the table filled up (or
// a fingerprint equals its empty marker) -- the caller takes the sorting path for this table.
// hs_launch_group_check, once the buckets have their tuples: the exact-membership proof of every k-mer (its
// bucket ints against the tuple of the bucket of rank d_rank_of[i]); *d_flag |= 1: one fingerprint, two HashKey
// strings (rebuild with another seed).
uint32_t hs_group_table_slots(uint64_t n);
hipError_t hs_launch_iota_u32(uint32_t* d_out, uint32_t n, hipStream_t s);
hipError_t hs_launch_group_insert(const int32_t* d_ints, uint64_t n, int K, uint32_t seed, uint64_t* d_table,
                                  uint32_t C, uint32_t* d_slot_of, uint32_t* d_flag, hipStream_t s);
hipError_t hs_launch_group_check(const int32_t* d_ints, uint64_t n, int K, const uint32_t* d_rank_of,
                                 const int32_t* d_dir_tuple, uint32_t* d_flag, hipStream_t s);
// distinct keys per block of 1024 slots; after an exclusive scan of those counts (d_blk_off, with the
// total at [n_blocks]): the distinct keys' fingerprints d_dk and their slots d_ds in slot order
hipError_t hs_launch_fp_count(const uint64_t* d_table, uint32_t C, uint32_t* d_blk_cnt, hipStream_t s);
hipError_t hs_launch_fp_compact(const uint64_t* d_table, uint32_t C, const uint32_t* d_blk_off, uint64_t* d_dk,
                                uint32_t* d_ds, hipStream_t s);
// d_rank_of_slot[d_ds_sorted[r]] = r; then d_slot_of[i] <- rank of k-mer i's key, in place
hipError_t hs_launch_rank_slots(const uint32_t* d_ds_sorted, uint32_t nb, uint32_t* d_rank_of_slot, hipStream_t s);
hipError_t hs_launch_rank_kmers(uint32_t* d_slot_of, uint64_t n, const uint32_t* d_rank_of_slot, hipStream_t s);
// one stable LSD radix pass (8 bits from `shift`) over (key, id): histogram [256][hs_rs_blocks(n)], the
// caller's exclusive scan over it, scatter (d_ids_in null: ids 0 .. n - 1)
uint32_t hs_rs_blocks(uint64_t n);
hipError_t hs_launch_rs_hist(const uint32_t* d_keys, uint32_t n, int shift, uint32_t* d_hist, hipStream_t s);
hipError_t hs_launch_rs_scatter(const uint32_t* d_keys_in, const uint32_t* d_ids_in, uint32_t n, int shift,
                                const uint32_t* d_hist_scanned, uint32_t* d_keys_out, uint32_t* d_ids_out,
                                hipStream_t s);
// bucket boundaries from the sorted ranks (d_dir_start[nb + 1]) and the largest bucket (atomicMax into *d_max)
hipError_t hs_launch_dir_start(const uint32_t* d_ranks_sorted, uint32_t n, uint32_t nb, uint32_t* d_dir_start,
                               uint32_t* d_max, hipStream_t s);

// index build with the hashing spread over ranks: d_tuples[nb][K] = the bucket ints of every bucket whose
// first member lies in this rank's block [lo, lo + cnt) (zeros elsewhere); the exact-membership proof of
// the block's k-mers against the buckets' tuples (*d_flag |= 1: one fingerprint, two HashKey strings)
hipError_t hs_launch_shard_first_tuples(const uint32_t* d_dir_start, const uint32_t* d_ids, const int32_t* d_ints_block,
                                        uint32_t lo, uint32_t cnt, uint32_t nb, int K, int32_t* d_tuples,
                                        hipStream_t s);
hipError_t hs_launch_shard_check(const int32_t* d_ints_block, uint32_t lo, uint32_t cnt, int K,
                                 const uint32_t* d_pos_of, const uint32_t* d_dir_start, uint32_t nb,
                                 const int32_t* d_dir_tuple, uint32_t* d_flag, hipStream_t s);

// ---- projection on the matrix cores (hs_proj.hip) ------------------------------------------------
// The coordinate table in 16-bit fixed point for the codes path: per residue the high and low digit
// bytes of its 8 coordinates, an upper bound of its 1-norm, the scale 2^-ex and dx = 2^-(ex+1).
struct hs_proj_table {
  uint4 dig[HS_ALPHABET_PAD];   // {X1[0..3], X1[4..7], X0[0..3], X0[4..7]}
  double l1[HS_ALPHABET_PAD];
  double sx, dx, l1max;
  uint32_t unsafe, pad;
};
// k-steps (of 32 dimensions) the MFMA pass is compiled for: 4, 7, 10 or 13; 0 = k too long (> 52)
int hs_proj_steps(int k);
hipError_t hs_launch_quant_table(const double* d_coords, int alphabet, hs_proj_table* d_tab, hipStream_t s);
// planes -> digit fragments for the all-functions tiling (d_aq_all: ceil(F/32) tiles) and the
// per-table tiling (d_aq_tab: one tile per table; both zero-filled by the caller, S*2*64 uint4 per
// tile) + constants d_fn[F] (4 doubles each); d_stats[3] (zeroed): max da, max |a^|_1 as double
// bits, and 1 if a function cannot be quantised
hipError_t hs_launch_quant_planes(const double* d_a, const double* d_b, int F, int d, int K, int S, double W,
                                  double eps_scale, void* d_aq_all, void* d_aq_tab, void* d_fn,
                                  unsigned long long* d_stats, hipStream_t s);
// points -> d_xq [n][S*4] uint4 + d_xmeta [n][3]
hipError_t hs_launch_quant_points(const double* d_pts, uint64_t n, int k, int S, void* d_xq, double* d_xmeta,
                                  hipStream_t s);
// fast pass: bucket ints of F functions (d_aq / d_fn already offset to the first of them) for n
// points given as codes (d_codes != null) or as quantised points; uncertain values are appended to
// d_flags (*d_flag_count zeroed by the caller) ...
hipError_t hs_launch_proj(const uint8_t* d_codes, const void* d_xq, const double* d_xmeta, uint64_t n, int k,
                          int S, const void* d_aq, const void* d_fn, int F, const hs_proj_table* d_tab,
                          double W, int32_t* d_out, int out_stride, uint2* d_flags, uint32_t flag_cap,
                          uint32_t* d_flag_count, int n_cu, hipStream_t s);
// ... and recomputed here in the reference's operation order (everything, if the list overflowed)
hipError_t hs_launch_proj_fix(const uint8_t* d_codes, const double* d_pts, uint64_t n, int k, const double* d_aT,
                              int ldf, const double* d_b, int F, double W, const double* d_coords,
                              int32_t* d_out, int out_stride, const uint2* d_flags, uint32_t flag_cap,
                              const uint32_t* d_flag_count, hipStream_t s);

// ---- multi-probe (hs_multiprobe.hip) ----------------------------------------------------------------
// the exact projections of n points: d_ints[i][f] = floor(v), d_frac[i][f] = v - floor(v), v = (dot + b) / W in the
// reference's order; d_aT = the transposed planes [8k][F]
hipError_t hs_launch_mp_hash(const double* d_pts, uint64_t n, int k, const double* d_aT, int F, const double* d_b,
                             double W, int32_t* d_ints, double* d_frac, hipStream_t s);
// every (point, table)'s 1 + T probes (include/hsearch.h hs_probe_buckets): probe t of (q, l) goes to slot
// o = q sq + l sl + t st, its K ints at d_out[o K ..], its flag at d_valid[o]
hipError_t hs_launch_mp_probe_sets(const int32_t* d_ints, const double* d_frac, uint64_t n, int K, int L, int T,
                                   int32_t* d_out, uint8_t* d_valid, uint64_t sq, uint32_t sl, uint32_t st,
                                   hipStream_t s);
// d_out[r][:] = d_in[r / P][:], row elements per row
hipError_t hs_launch_mp_repeat_f64(const double* d_in, uint64_t n_out_rows, uint32_t row, uint32_t P, double* d_out,
                                   hipStream_t s);
hipError_t hs_launch_mp_repeat_u8(const uint8_t* d_in, uint64_t n_out_rows, uint32_t row, uint32_t P, uint8_t* d_out,
                                  hipStream_t s);
// d_q[i] = q_base + d_q[i] / P
hipError_t hs_launch_mp_map_q(uint32_t* d_q, uint64_t n, uint32_t P, uint32_t q_base, hipStream_t s);
// d_cand[q][l] = sum over t < P of d_vcand[q P + t][l]
hipError_t hs_launch_mp_cand(const uint64_t* d_vcand, uint64_t nq, uint32_t L, uint32_t P, uint64_t* d_cand,
                             hipStream_t s);

// ---- kernel launchers (hs_kernels.hip) -----------------------------------------------------------
hipError_t hs_launch_embed(const uint8_t* d_codes, uint64_t n, int k, const double* d_coords,
                           double* d_out, hipStream_t s);
// buckets out[i*out_stride + f], f in [0,F): exact reference arithmetic.  d_aT = the plane matrix
// TRANSPOSED, [8k][ldf] doubles (dimension-major), already offset to the first of the F functions.
hipError_t hs_launch_hash_codes(const uint8_t* d_codes, uint64_t n, int k, const double* d_aT, int ldf,
                                const double* d_b, int F, double W, const double* d_coords,
                                int32_t* d_out, int out_stride, hipStream_t s);
hipError_t hs_launch_hash_points(const double* d_pts, uint64_t n, int k, const double* d_aT, int ldf,
                                 const double* d_b, int F, double W, int32_t* d_out, int out_stride,
                                 hipStream_t s);
// d_out[c][r] = d_in[r][c]
hipError_t hs_launch_transpose_f64(const double* d_in, int rows, int cols, double* d_out, hipStream_t s);
// keys[i] = fingerprint(ints[i*stride .. +K)); ids[i] = i (if ids != null)
hipError_t hs_launch_keys(const int32_t* d_ints, uint64_t n, int stride, int K, uint32_t seed,
                          uint64_t* d_keys, uint32_t* d_ids, hipStream_t s);
// flag |= 1 if two sorted neighbours share a fingerprint but not a key string; flag |= 2 if the
// queue of non-identical neighbour tuples (d_slow: count + slow_cap positions) overflowed, in which
// case the caller repeats the call with exhaustive = true (every neighbour pair compared as strings)
hipError_t hs_launch_check_runs(const uint64_t* d_keys_sorted, const uint32_t* d_ids_sorted,
                                const int32_t* d_ints, uint64_t n, int K, uint32_t* d_flag,
                                uint32_t* d_slow, uint32_t slow_cap, bool exhaustive, int sorted_from_bit,
                                hipStream_t s);
hipError_t hs_launch_dir_tuples(const uint32_t* d_dir_start, const uint32_t* d_ids_sorted,
                                const int32_t* d_ints, uint32_t nb, int K, int32_t* d_dir_tuple,
                                hipStream_t s);
hipError_t hs_launch_pack(const uint8_t* d_codes, uint64_t n, int k, int alphabet, uint4* d_packed,
                          uint32_t* d_bad, hipStream_t s);
hipError_t hs_launch_gather_packed(const uint4* d_packed_all, const uint32_t* d_ids_sorted,
                                   uint64_t n, int PW, uint4* d_out, hipStream_t s);
hipError_t hs_launch_set_u32(uint32_t* d_p, uint32_t v, hipStream_t s);
// zeros over n <= HS_ZERO_RANGES ranges of 32-bit words, one launch
#define HS_ZERO_RANGES 8
struct hs_zero_ranges {
  uint32_t* p[HS_ZERO_RANGES];
  uint64_t words[HS_ZERO_RANGES];
  uint32_t n;
};
hipError_t hs_launch_zero_ranges(const hs_zero_ranges& r, hipStream_t s);
// d_out[i] = d_in[i] if it is a row of the table (< alphabet), else 0 and *d_bad |= 1
hipError_t hs_launch_recognise_kmers(const double* d_centers, uint64_t nq, int k, const double* d_coords, int alphabet,
                                     uint8_t* d_out_codes, uint32_t* d_n_unrecognised, hipStream_t s);
hipError_t hs_launch_check_codes(const uint8_t* d_in, uint64_t n_bytes, int alphabet, uint8_t* d_out,
                                 uint32_t* d_bad, hipStream_t s);
// windows of length k of every sequence of a residue buffer -> codes [n_windows][k] (+ the buffer
// position of every window); d_win_off[s] = number of the first window of sequence s
hipError_t hs_launch_windows(const uint8_t* d_residues, uint32_t n_residues, const uint32_t* d_seq_start,
                             const uint32_t* d_win_off, uint32_t n_seq, int k, uint8_t* d_codes,
                             uint32_t* d_win_pos, hipStream_t s);
// KLSH codes of n_seq sequences of reduced-alphabet classes (one wave per sequence)
hipError_t hs_launch_klsh(const uint8_t* d_classes, const uint64_t* d_seq_start, uint64_t n_seq,
                          const double* d_w, const double* d_b, const double* d_t, uint32_t bits,
                          uint64_t* d_codes, uint64_t* d_uncertain, hipStream_t s);
// d_out[d_perm[i]] = i
hipError_t hs_launch_invert_perm(const uint32_t* d_perm, uint32_t n, uint32_t* d_out, hipStream_t s);
hipError_t hs_launch_gather_rows(const uint8_t* d_all, const uint32_t* d_subset, uint64_t n_sub, int k,
                                 uint8_t* d_out, hipStream_t s);
// hs_index_load: checks of a table read from a file (see hs_validate_*_kernel); writes the inverse
// permutation into d_pos_of, ORs failure bits into *d_flag, atomicMax of the bucket sizes into
// *d_max_bucket
hipError_t hs_launch_validate_table(const uint32_t* d_ids, uint32_t n, uint32_t* d_pos_of,
                                    const uint32_t* d_dir_start, const uint64_t* d_dir_key,
                                    const int32_t* d_dir_tuple, uint32_t nb, int K, uint32_t seed,
                                    uint32_t* d_flag, uint32_t* d_max_bucket, hipStream_t s);
// the tuple hashes of the buckets with more than `threshold` members, unordered: d_out[atomicAdd(d_count, 1)]
// while the count stays below cap (the count keeps running: the caller sees an overflow)
hipError_t hs_launch_giant_buckets(const int32_t* d_dir_tuple, int K, const uint32_t* d_dir_start, uint32_t nb,
                                   uint32_t threshold, uint64_t* d_out, uint32_t cap, uint32_t* d_count, hipStream_t s);
// Bucket partition, ahead of the probe: d_flag[ql] = 1 where probe ql = (query, table) belongs to tabs.part (by
// its bucket ints alone: no fingerprint, no directory); the outputs of the probe kernel are cleared for the
// others (d_qbucket[ql] = nb_total: found nothing).  d_flag[nq * L] = 0.
hipError_t hs_launch_part_owned(const hs_tables_dev& tabs, const int32_t* d_qints, uint32_t nq, int K, int L,
                                uint32_t nb_total, uint32_t* d_flag, uint32_t* d_qstart, uint32_t* d_qcount,
                                uint32_t* d_nslices, uint64_t* d_cand_out, uint32_t* d_qbucket, hipStream_t s);
// d_list[d_pos[i]] = i where d_flag[i] (d_pos = exclusive scan of d_flag)
hipError_t hs_launch_flagged_list(const uint32_t* d_flag, const uint32_t* d_pos, uint32_t n, uint32_t* d_list,
                                  hipStream_t s);
#define HS_REC_MAX_K 24
// rec[b] = {key[b], start[b], start[b + 1] - start[b]; int16 tuple[b][0..K)}; *d_flag |= 1 where an int does not fit
hipError_t hs_launch_dir_records(const uint64_t* d_dir_key, const uint32_t* d_dir_start, const int32_t* d_dir_tuple,
                                 uint32_t nb, int K, uint4* d_rec, uint32_t* d_flag, hipStream_t s);
// jump[t] = first directory entry with (key >> shift) >= t, t = 0 .. n_slots (jump[n_slots] = nb)
hipError_t hs_launch_dir_jump(const uint64_t* d_dir_key, uint32_t nb, uint32_t shift, uint32_t n_slots,
                              uint32_t* d_jump, hipStream_t s);
hipError_t hs_launch_max_u32(const uint32_t* d_in, uint32_t n, uint32_t* d_out, hipStream_t s);

hipError_t hs_launch_probe(const hs_tables_dev& tabs, const int32_t* d_qints, uint32_t nq, int K,
                           int L, uint32_t seed, uint32_t* d_qstart, uint32_t* d_qcount,
                           uint32_t* d_nslices, uint64_t* d_cand_out, unsigned long long* d_cand_total,
                           uint32_t* d_slow /* [nq*L + 1] */, const uint32_t* d_dir_base,
                           uint32_t nb_total, uint32_t* d_bucket_count, uint32_t* d_qbucket,
                           uint32_t* d_qrank, hipStream_t s);
// The caller has zeroed d_slow[0] and, where given, d_bucket_count[0 .. nb_total + 2) (the batch's reset);
// d_nslices == null: no slice counts (every segment goes to the join).
// With d_qbucket != null the probe also numbers every probe's bucket for the join's grouping: global
// bucket number d_qbucket[ql] = d_dir_base[table] + directory index (nb_total = the pseudo-bucket
// of probes that found none).  With d_bucket_count != null hs_rank_kernel follows: d_qrank[ql] = the probe's
// rank inside its bucket -- any bijection of the bucket's probes onto [0, count) -- and d_bucket_count[bucket]
// = count, from one global atomic per bucket and workgroup of 2048 queries of a table, not one per probe.
// hs_launch_seg_group turns that into sorted_ql / seg_key / seg_cnt / n_seg (a counting sort: the
// segments come out in bucket-number order, the pseudo-bucket last).
// The same outputs when buckets far outnumber probes (the counting sort's passes over every bucket
// slot would dominate: C3 shape at W = 160, 1.3e8 slots for 4e6 probes): the probes are radix-sorted
// on their bucket number (d_qbucket from the probe kernels, which then take no ranks), segment
// heads found by comparing neighbours.  d_work: 4 (nql + 1) words; d_iota / d_keys_sorted: nql words.
hipError_t hs_launch_seg_group_sparse(const hs_tables_dev& tabs, const uint32_t* d_dir_base, int L, int shift,
                                      uint32_t nb_total, void* d_temp, size_t temp_bytes,
                                      const uint32_t* d_qbucket, uint32_t* d_keys_sorted, uint32_t* d_iota,
                                      uint32_t* d_work, uint32_t nql, uint32_t* d_sorted_ql,
                                      uint64_t* d_seg_key, uint32_t* d_seg_cnt, uint32_t* d_n_seg,
                                      uint32_t* d_seg_of /* [nql]: segment of every sorted probe position */,
                                      hipStream_t s, const uint32_t* d_probes_in = nullptr);
// bucket partition: the probes that found a bucket (d_qbucket[ql] != nb_total), in probe order, as (bucket,
// probe) pairs d_keys / d_probes; d_pos[nql] = their number.  d_flag, d_pos: nql + 1 words.  d_list != null: only
// the nql probes d_list[0 .. nql) (ascending) are looked at.
hipError_t hs_launch_found_probes(const uint32_t* d_qbucket, uint32_t nql, uint32_t nb_total, void* d_temp,
                                  size_t temp_bytes, uint32_t* d_flag, uint32_t* d_pos, uint32_t* d_keys,
                                  uint32_t* d_probes, hipStream_t s, const uint32_t* d_list = nullptr);
hipError_t hs_launch_seg_group(const hs_tables_dev& tabs, const uint32_t* d_dir_base, int L, int shift,
                               uint32_t nb_total, const uint32_t* d_bucket_count,
                               uint32_t* d_bucket_work /* 2 x (nb_total + 2), 8-byte aligned */, void* d_temp,
                               size_t temp_bytes, const uint32_t* d_qbucket, const uint32_t* d_qrank,
                               uint32_t nql, uint32_t* d_sorted_ql, uint64_t* d_seg_key,
                               uint32_t* d_seg_cnt, uint32_t* d_n_seg, uint32_t* d_seg_of, hipStream_t s);
// self-join: query q = indexed k-mer first_id + q probes the bucket it sits in (no hash, no directory
// search); outputs as hs_launch_probe
hipError_t hs_launch_self_probe(const hs_tables_dev& tabs, uint32_t first_id, uint32_t nq, int L,
                                uint32_t* d_qstart, uint32_t* d_qcount, uint32_t* d_nslices,
                                uint64_t* d_cand_out, unsigned long long* d_cand_total,
                                const uint32_t* d_dir_base, uint32_t nb_total, uint32_t* d_bucket_count,
                                uint32_t* d_qbucket, uint32_t* d_qrank, hipStream_t s);
hipError_t hs_launch_qtables(const double* d_centers, uint32_t nq, int k, const double* d_coords,
                             int alphabet, float* d_tq, hipStream_t s);
hipError_t hs_launch_verify(const hs_tables_dev& tabs, const uint32_t* d_qstart,
                            const uint32_t* d_qcount, const uint32_t* d_slice_off, uint32_t nql,
                            const float* d_tq, int k, int L, float r2_hi, uint32_t* d_prov_count,
                            uint32_t prov_cap, uint2* d_prov, int n_blocks, hipStream_t s,
                            const double* d_radii = nullptr /* [nq] or null: the bound from every query's own radius */);
// d_qcodes != null: the queries are indexed k-mers given as codes [nq][k] (self-join), d_centers unused
hipError_t hs_launch_finalize(const hs_tables_dev& tabs, const uint8_t* d_codes,
                              const double* d_centers, const uint8_t* d_qcodes, const double* d_coords,
                              const uint32_t* d_qstart, const uint32_t* d_qcount,
                              const uint2* d_prov, const uint32_t* d_prov_count, uint32_t prov_cap,
                              const uint32_t* d_sorted_ql, int k, int L, double r2, double r_sqrt,
                              uint32_t q_base, uint32_t self_first, uint32_t* d_hit_count,
                              uint32_t hit_cap, uint64_t* d_hit_key, uint64_t* d_hit_val,
                              uint32_t* d_qcnt /* [nq] hits per query, or null */, int alphabet,
                              const uint4* d_qpacked /* the queries as packed k-mers (with d_qcodes), or null */,
                              uint32_t* d_hit_rank /* with d_qcnt: the hit's number among its query's hits */,
                              hipStream_t s, const double* d_radii = nullptr /* [nq] or null: r2 = radii[q]^2 */);
#ifdef __HIPCC__
// First-seen rule (label[], motif_both_points.cpp:233): a hit's id was already reported if an EARLIER
// table's probed bucket holds it, i.e. if its sorted position in that table falls inside the bucket's
// range.  These kernels are bound by the ADDRESSES their scattered loads present (a wave instruction with
// 64 different cache lines occupies the address unit for 64 cycles), so: four tables per step; their four
// (start, count) words as two 16-byte loads (qstart / qcount carry four words of padding for the last
// query); one position load per table, each under the lanes that need that table only.
__device__ __forceinline__ bool seen_in_earlier_table(const hs_tables_dev& tabs, const uint32_t* __restrict__ qstart,
                                                      const uint32_t* __restrict__ qcount, uint32_t q, int l, int L,
                                                      uint32_t id, bool hit) {
  bool dup = false;
  struct __attribute__((packed, aligned(4))) U4 { uint32_t v[4]; };
  // steps of 1, 3, 4, 4, ... tables: a pair that shares a bucket in one table mostly shares table 0's too, and
  // a hit found there needs no further look (every look is a cache line of pos_of from HBM)
  int w = 1;
  for (int l0 = 0; l0 < L; l0 += w, w = l0 == 1 ? 3 : 4) {
    if (!__ballot(hit && l > l0 && !dup)) break;  // (wave-uniform)
    if (hit && l > l0 && !dup) {
      const U4 c4 = *reinterpret_cast<const U4*>(qcount + (size_t)q * L + l0);
      const U4 s4 = *reinterpret_cast<const U4*>(qstart + (size_t)q * L + l0);
      uint32_t p4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < w && l0 + u < l) p4[u] = tabs.t[l0 + u].pos_of[id];
#pragma unroll
      for (int u = 0; u < 4; ++u) dup = dup || (u < w && l0 + u < l && p4[u] - s4.v[u] < c4.v[u]);
    }
  }
  return dup;
}
#endif

// hs_finalize's first-seen test reads four words at a time from d_qstart / d_qcount: this many words of padding
#define HS_QRANGE_PAD 4
// the batch's hits in the reference's order without a sort: bucket by query (d_qoff = exclusive
// scan of the per-query counts), order every query's few hits, unpack to the outputs (at most
// out_room of them); *d_big is set when a query has too many hits for that (caller: radix sort)
hipError_t hs_launch_hit_order(const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_hit_count,
                               uint32_t hit_cap, uint32_t q_base, uint32_t nq, const uint32_t* d_qoff,
                               const uint32_t* d_rank, void* d_kv /* hit_cap x 16 bytes: (key, value) by query */, uint32_t* d_big,
                               uint32_t* d_qlist /* 8 + 3 nq words, the first eight zero */,
                               uint32_t* d_q, uint32_t* d_id, uint32_t* d_table, double* d_dist,
                               uint64_t out_room, int n_cu, hipStream_t s);
// self_first: the queries are the indexed k-mers self_first, self_first + 1, ... themselves (the
// self-join): the pair of a k-mer with itself is not a hit; HS_NO_SELF otherwise
#define HS_NO_SELF 0xffffffffu
// merge of the table-partitioned layout (hs_merge_first_table_dev): keys (q, id, table) + the distance bits;
// run heads of the sorted keys; the heads re-keyed (q, table, id) at their scanned positions
hipError_t hs_launch_merge_key1(const uint32_t* d_q, const uint32_t* d_id, const uint32_t* d_table, const double* d_dist,
                                uint32_t n, uint64_t* d_key, uint64_t* d_val, hipStream_t s);
hipError_t hs_launch_merge_flag(const uint64_t* d_key, uint32_t n, uint32_t* d_flag /* [n + 1] */, hipStream_t s);
hipError_t hs_launch_merge_compact(const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_pos /* [n + 1] */,
                                   uint32_t n, uint64_t* d_key2, uint64_t* d_val2, hipStream_t s);
hipError_t hs_launch_unpack_hits(const uint64_t* d_key, const uint64_t* d_val, uint32_t n,
                                 uint32_t* d_q, uint32_t* d_id, uint32_t* d_table, double* d_dist,
                                 hipStream_t s);
// nearest centre per DB id (hs_annotate.hip): a batch's hits -- (d_key, d_val) as the exact pass leaves them, or,
// with d_key == null, the four arrays of a merged list -- reduced into best_dist / best_tq [n_slots]; ids whose
// slot was HS_ANNOT_EMPTY are appended to d_touched (*d_n_touched counts them).  The gather writes row i from the
// slot of d_sorted_id[i] (d_out_id == null: no rows) and empties the slot.
#define HS_ANNOT_EMPTY 0xffffffffffffffffull
hipError_t hs_launch_annot_reduce(const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_q,
                                  const uint32_t* d_id, const uint32_t* d_table, const double* d_dist,
                                  uint32_t n_hits, uint64_t* d_best_dist, uint32_t* d_best_tq, uint32_t n_slots,
                                  uint32_t* d_touched, uint32_t* d_n_touched, hipStream_t s);
hipError_t hs_launch_annot_gather(const uint32_t* d_sorted_id, uint32_t cnt, uint64_t* d_best_dist,
                                  const uint32_t* d_best_tq, uint32_t n_slots, uint32_t* d_out_id, uint32_t* d_out_q,
                                  uint32_t* d_out_table, double* d_out_dist, hipStream_t s);
// top-k hits per query (hs_knn.hip; the rule, the passes and the scratch are written at its head): the hits of one
// batch -- (d_key, d_val), or with d_key == null the four arrays of a merged list -- whose queries are [first, first +
// count) of the call, selected per query into rows row0 + first ... of the output arrays (d_nn_table may be null).
// d_cnt, d_off [count + 1], d_cur [count], d_seg_d, d_seg_w [n_hits], d_temp of hs_knn_temp(count) bytes; *d_total
// (64 bits) grows by the batch's hits.  self_first != HS_NO_SELF: the pair of a k-mer with itself is no hit.
size_t hs_knn_temp(uint32_t count);
hipError_t hs_launch_knn_batch(const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_q, const uint32_t* d_id,
                               const uint32_t* d_table, const double* d_dist, uint32_t n_hits, uint32_t self_first,
                               uint32_t first, uint32_t count, uint32_t* d_cnt, uint32_t* d_off, uint32_t* d_cur,
                               void* d_temp, size_t temp_bytes, uint64_t* d_seg_d, uint64_t* d_seg_w, uint64_t* d_total,
                               uint32_t topk, uint64_t row0, uint32_t* d_nn_id, uint32_t* d_nn_table, double* d_nn_dist,
                               uint32_t* d_nn_count, hipStream_t s);
// rows of padding with zero counts: a call that ran no batch
hipError_t hs_launch_knn_fill(uint64_t rows, uint32_t topk, uint32_t* d_nn_id, uint32_t* d_nn_table, double* d_nn_dist,
                              uint32_t* d_nn_count, hipStream_t s);
// hits per (query group, sequence, diagonal) (hs_seqmatch.hip; the rule, the passes and the scratch are written at its
// head).  check: d_out [3] (zeroed) = {flags (non-zero: invalid), max q_off, max ids of a sequence}.  key: the 64-bit
// key and the index of each hit of a batch -- (d_key, d_val), or with d_key == null the arrays of a merged list.
// head: d_head [n + 1] over sorted keys.  reduce: the sorted elements (d_skey, d_sidx, the scan d_excl of d_head) whose
// source is a batch's hits or, with d_src_rows != null, the rows of a list of capacity src_cap, into rows dst_row0 ...
// dst_row0 + n_rows of the list d_dst_rows of capacity dst_cap (one allocation of 40 bytes per row of capacity);
// d_part of hs_sm_part_bytes(n) bytes.  decode: a list's first n rows into the output arrays; *d_flag |= 1 where a
// count passes 32 bits.
bool hs_sm_widths(uint64_t n_groups, uint64_t n_seq, uint64_t max_len, uint64_t max_qoff, int* wg, int* ws, int* wd);
hipError_t hs_launch_sm_check(const uint32_t* d_q_group, const uint32_t* d_q_off, uint64_t nq, uint64_t n_groups,
                              const uint64_t* d_id_start, uint64_t n_seq, uint64_t n, uint64_t* d_out, hipStream_t s);
hipError_t hs_launch_sm_key(const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_q, const uint32_t* d_id,
                            const double* d_dist, uint32_t n_hits, const uint32_t* d_q_group, const uint32_t* d_q_off,
                            const uint64_t* d_id_start, uint64_t n_seq, int ws, int wd, uint64_t max_qoff,
                            uint64_t* d_out_key, uint32_t* d_out_idx, hipStream_t s);
hipError_t hs_launch_sm_iota(uint32_t n, uint32_t* d_idx, hipStream_t s);
hipError_t hs_launch_sm_head(const uint64_t* d_skey, uint32_t n, uint32_t* d_head, hipStream_t s);
size_t hs_sm_part_bytes(uint32_t n);
hipError_t hs_launch_sm_reduce(const uint64_t* d_skey, const uint32_t* d_sidx, const uint32_t* d_excl,
                               const uint32_t* d_head, uint32_t n, const uint64_t* d_key, const uint64_t* d_val,
                               const uint32_t* d_q, const uint32_t* d_id, const double* d_dist,
                               const uint64_t* d_id_start, int ws, int wd, const void* d_src_rows, uint64_t src_cap,
                               void* d_dst_rows, uint64_t dst_cap, uint64_t dst_row0, uint32_t n_rows, void* d_part,
                               hipStream_t s);
hipError_t hs_launch_sm_decode(const void* d_rows, uint64_t cap, uint32_t n, int ws, int wd, uint64_t max_qoff,
                               uint32_t* d_group, uint32_t* d_seq, int32_t* d_diag, uint32_t* d_count,
                               double* d_best_dist, uint32_t* d_best_q, uint32_t* d_best_id, uint32_t* d_lo,
                               uint32_t* d_hi, uint32_t* d_flag, hipStream_t s);
// connected components of the self-join's graph (hs_components.hip): d_parent [n] is a union-find forest with
// parent[x] <= x, d_counts two 64-bit words {ordered pairs united, roots}.  begin: the identity and zero counts;
// union: a batch's pairs (self_first + (key >> 37), (uint32_t)key) as the exact pass leaves them in d_key, the
// pair of an id with itself skipped; flatten: d_label[i] = the root of i = the smallest id of i's component.
hipError_t hs_launch_cc_begin(uint32_t* d_parent, uint32_t n, uint64_t* d_counts, hipStream_t s);
hipError_t hs_launch_cc_union(const uint64_t* d_key, uint32_t n_hits, uint32_t self_first, uint32_t* d_parent,
                              uint32_t n, uint64_t* d_counts, hipStream_t s);
hipError_t hs_launch_cc_flatten(uint32_t* d_parent, uint32_t n, uint32_t* d_label, uint64_t* d_counts, hipStream_t s);
// density clusters of the self-join's graph (hs_dbscan.hip): d_deg, d_parent, d_anchor [n], d_counts five 64-bit
// words {ordered pairs, clusters, core, border, noise}.  begin: zero degrees, the identity, no anchors, zero counts;
// degree (pass 1): deg[a] += 1 per pair (a, b) of a batch as the exact pass leaves them in d_key -- NOT idempotent,
// every ordered pair must come exactly once; unite (pass 2, behind the kernel boundary of the last degree): cores
// (deg + 1 >= min_pts) united, anchor[a] = the smallest core neighbour of a non-core a; finish: the labels and counts.
hipError_t hs_launch_db_begin(uint32_t* d_deg, uint32_t* d_parent, uint32_t* d_anchor, uint32_t n, uint64_t* d_counts,
                              hipStream_t s);
hipError_t hs_launch_db_degree(const uint64_t* d_key, uint32_t n_hits, uint32_t self_first, uint32_t* d_deg, uint32_t n,
                               uint64_t* d_counts, hipStream_t s);
hipError_t hs_launch_db_unite(const uint64_t* d_key, uint32_t n_hits, uint32_t self_first, const uint32_t* d_deg,
                              uint32_t min_pts, uint32_t* d_parent, uint32_t* d_anchor, uint32_t n, hipStream_t s);
hipError_t hs_launch_db_finish(uint32_t* d_parent, const uint32_t* d_deg, const uint32_t* d_anchor, uint32_t min_pts,
                               uint32_t n, uint32_t* d_label, uint64_t* d_counts, hipStream_t s);
// minimum spanning forest of the self-join's graph (hs_msf.hip; the state, the round and the invariant are written at
// its head).  d_counts: eight 64-bit words, of which five are used {ordered pairs of the pass, pairs that cross two
// components, entries appended to the kept list, tree edges, roots}.  begin: comp and parent the identity, the slots
// empty, zero counts.  min_d_hits / min_pair_hits: steps 1 and 2 over a batch's pairs as the exact pass leaves them in
// (d_key, d_val); with d_kept != null step 1 also appends the pairs with a < b to d_kept[kept_cap] (16 bytes each:
// lo << 32 | hi, distance bits) while there is room -- counts[2] keeps running.  min_d_kept / min_pair_kept: the same
// steps over that list.  select: step 3, then comp[i] = find(i) and the slots emptied.  finish: d_label (may be null)
// = comp, the roots counted.  unpack: the sorted (pair, bits) into the three output arrays.
#define HS_MSF_MAX_ROUNDS 34u
hipError_t hs_launch_msf_begin(uint32_t* d_comp, uint32_t* d_parent, uint64_t* d_best_d, uint64_t* d_best_pair,
                               uint32_t n, uint64_t* d_counts, hipStream_t s);
hipError_t hs_launch_msf_min_d_hits(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits, uint32_t self_first,
                                    const uint32_t* d_comp, uint64_t* d_best_d, uint32_t n, uint64_t* d_counts,
                                    void* d_kept, uint64_t kept_cap, hipStream_t s);
hipError_t hs_launch_msf_min_pair_hits(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits,
                                       uint32_t self_first, const uint32_t* d_comp, const uint64_t* d_best_d,
                                       uint64_t* d_best_pair, uint32_t n, hipStream_t s);
hipError_t hs_launch_msf_min_d_kept(const void* d_kept, uint64_t n_kept, const uint32_t* d_comp, uint64_t* d_best_d,
                                    uint32_t n, uint64_t* d_counts, hipStream_t s);
hipError_t hs_launch_msf_min_pair_kept(const void* d_kept, uint64_t n_kept, const uint32_t* d_comp,
                                       const uint64_t* d_best_d, uint64_t* d_best_pair, uint32_t n, hipStream_t s);
hipError_t hs_launch_msf_select(uint32_t* d_comp, uint32_t* d_parent, uint64_t* d_best_d, uint64_t* d_best_pair,
                                uint32_t n, uint64_t* d_out_pair, uint64_t* d_out_d, uint64_t* d_counts,
                                hipStream_t s);
hipError_t hs_launch_msf_finish(const uint32_t* d_comp, uint32_t n, uint32_t* d_label, uint64_t* d_counts,
                                hipStream_t s);
hipError_t hs_launch_msf_unpack(const uint64_t* d_pair, const uint64_t* d_d, uint32_t m, uint32_t* d_lo, uint32_t* d_hi,
                                double* d_dist, hipStream_t s);
// the density tree of the self-join's graph (hs_density.hip; the rule, the state and the rounds of the core pass are
// written at its head).  d_counts: hs_msf's eight 64-bit words, with [5] = k-mers with a finite core distance and
// [6] = k-mers of the batch still open after a round.  begin: the state of a call (core = +0 for min_pts = 1, open
// otherwise).  pairs: a batch's ordered pairs counted and, with d_kept != null, those with a < b appended as
// hs_launch_msf_min_d_hits appends them.  round: one threshold round (next, count, settle) over a batch's hits for the
// k-mers [first, first + count) -- a range outside 0 .. n is hipErrorInvalidValue, nothing launched.  core_finish: unsettled k-mers get +inf,
// the finite ones are counted.  min_d_* / min_pair_*: steps 1 and 2 of hs_msf's round under the weight
// max(d, core[a], core[b]); a pair with an infinite end is skipped.  finish: d_label (may be null) = comp where the
// core distance is finite and HS_NOISE elsewhere; with d_counts != null the roots among the former are counted.
hipError_t hs_launch_dt_begin(uint64_t* d_core, uint64_t* d_thr, uint64_t* d_next, uint32_t* d_cnt, uint32_t n,
                              uint32_t min_pts, hipStream_t s);
hipError_t hs_launch_dt_pairs(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits, uint32_t self_first,
                              uint32_t n, uint64_t* d_counts, void* d_kept, uint64_t kept_cap, hipStream_t s);
hipError_t hs_launch_dt_round(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits, uint32_t self_first,
                              uint32_t n, uint32_t first, uint32_t count, uint32_t min_pts, uint64_t* d_core,
                              uint64_t* d_thr, uint64_t* d_next, uint32_t* d_cnt, uint64_t* d_counts, hipStream_t s);
hipError_t hs_launch_dt_core_finish(uint64_t* d_core, uint32_t n, uint64_t* d_counts, hipStream_t s);
hipError_t hs_launch_dt_min_d_hits(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits, uint32_t self_first,
                                   const uint64_t* d_core, const uint32_t* d_comp, uint64_t* d_best_d, uint32_t n,
                                   uint64_t* d_counts, hipStream_t s);
hipError_t hs_launch_dt_min_pair_hits(const uint64_t* d_key, const uint64_t* d_val, uint32_t n_hits,
                                      uint32_t self_first, const uint64_t* d_core, const uint32_t* d_comp,
                                      const uint64_t* d_best_d, uint64_t* d_best_pair, uint32_t n, hipStream_t s);
hipError_t hs_launch_dt_min_d_kept(const void* d_kept, uint64_t n_kept, const uint64_t* d_core, const uint32_t* d_comp,
                                   uint64_t* d_best_d, uint32_t n, uint64_t* d_counts, hipStream_t s);
hipError_t hs_launch_dt_min_pair_kept(const void* d_kept, uint64_t n_kept, const uint64_t* d_core,
                                      const uint32_t* d_comp, const uint64_t* d_best_d, uint64_t* d_best_pair,
                                      uint32_t n, hipStream_t s);
hipError_t hs_launch_dt_finish(const uint32_t* d_comp, const uint64_t* d_core, uint32_t n, uint32_t* d_label,
                               uint64_t* d_counts, hipStream_t s);
// cluster profiles and radii from a label array (hs_summary.hip; the arrays are the state listed at its head).
// group: sizes, validation (*d_err |= 1: a label that is neither HS_NOISE nor < n) and the two scans -- the caller
// reads d_err[0], d_row_of[n] (rows) and d_off_of[n] (kept members) back before it goes on; members: the rows' labels
// and offsets and the ids grouped by row; head: out_label / out_size of the rows.
//
// What the item kernels of hs_summary.hip and hs_cluster_pssm.hip share.  Work items are ch consecutive member SLOTS;
// the pieces of rows inside an item (segments) are dealt to the workgroup's HS_SM_WAVES waves in rounds, and an item
// that lies inside one row is shared by the waves instead.  hs_sm_segment: the segment wave `wave` takes in round
// `round` of the item [p0, p1) whose first row is rf and which holds nseg rows.
#define HS_SM_WAVES 4u
struct hs_sm_seg {
  bool active, whole;  // whole: the segment is its whole row (plain stores); else it is added with atomics
  uint32_t row, lo, hi;
};
__device__ __forceinline__ hs_sm_seg hs_sm_segment(const uint32_t* __restrict__ row_off, uint32_t rf, uint32_t nseg,
                                                   uint32_t round, uint32_t wave, uint32_t p0, uint32_t p1) {
  hs_sm_seg s;
  const uint32_t t = nseg == 1 ? 0u : round * HS_SM_WAVES + wave;
  s.active = t < nseg;
  s.row = rf + (s.active ? t : 0u);
  const uint32_t ro = row_off[s.row], rn = row_off[s.row + 1];
  s.lo = ro > p0 ? ro : p0;
  s.hi = rn < p1 ? rn : p1;
  s.whole = ro >= p0 && rn <= p1;
  return s;
}
// lanes per member of the histogram kernels: the power of two >= k, at most 64, as a shift
inline uint32_t hs_sm_lpm_shift(int k) {
  uint32_t s = 0;
  while (s < 6 && (1 << s) < k) ++s;
  return s;
}
hipError_t hs_launch_sm_group(const uint32_t* d_label, uint32_t n, uint32_t min_size, uint32_t* d_size, uint32_t* d_tmp,
                              uint32_t* d_row_of, uint32_t* d_off_of, void* d_temp, size_t temp_bytes, uint32_t* d_err,
                              hipStream_t s);
hipError_t hs_launch_sm_members(const uint32_t* d_label, uint32_t n, uint32_t min_size, const uint32_t* d_size,
                                const uint32_t* d_row_of, uint32_t* d_off_of, uint32_t* d_row_label,
                                uint32_t* d_row_off, uint32_t* d_member, hipStream_t s);
hipError_t hs_launch_sm_head(const uint32_t* d_row_label, const uint32_t* d_row_off, uint32_t n_rows,
                             uint32_t* d_out_label, uint32_t* d_out_size, hipStream_t s);
// the batch of rows [r0, r1): d_counts [(r1 - r0)][k][alphabet] (row r0 first), then its centroids into
// d_centroid [n_rows][8k] (indexed by the row itself).  ch: member slots per work item.
hipError_t hs_launch_sm_profile(const uint8_t* d_codes, int k, int alphabet, const uint32_t* d_label,
                                const uint32_t* d_row_of, const uint32_t* d_row_off, const uint32_t* d_member,
                                uint32_t r0, uint32_t r1, uint32_t ch, uint32_t n_kept, uint32_t* d_counts,
                                int n_cu, hipStream_t s);
hipError_t hs_launch_sm_centroid(const uint32_t* d_counts, const double* d_coords, int k, int alphabet,
                                 const uint32_t* d_row_off, uint32_t r0, uint32_t r1, double* d_centroid,
                                 hipStream_t s);
// d_max_d2, d_radius [n_rows] f64, d_medoid [n_rows] u32 (the outputs; d_radius holds the rows' minima on the way)
hipError_t hs_launch_sm_radii(const uint8_t* d_codes, int k, int alphabet, const double* d_coords,
                              const uint32_t* d_label, const uint32_t* d_row_of, const uint32_t* d_row_off,
                              const uint32_t* d_member, uint32_t n_rows, uint32_t n_kept, uint32_t ch,
                              const double* d_centers, uint64_t* d_d2, double* d_max_d2, double* d_radius,
                              uint32_t* d_medoid, int n_cu, hipStream_t s);
// weighted cluster profiles and covering thresholds (hs_cluster_pssm.hip; the passes are written at its head), on the
// state hs_launch_sm_group / _members left.  weights: the batch of rows [r0, r1) whose raw counts are final and whose
// tables d_u [(r1 - r0)][k][alphabet] hs_launch_pssm_weights_table has built -> d_wcounts [(r1 - r0)][k][alphabet]
// (row r0 first).  cover: d_S [n_rows][k][alphabet] -> d_min_score, d_argmin [n_rows]; d_key [n_kept] u64 is scratch
// (the members' score keys), d_min_score holds the rows' minimal keys on the way.
hipError_t hs_launch_cp_weights(const uint8_t* d_codes, int k, int alphabet, const uint32_t* d_label,
                                const uint32_t* d_row_of, const uint32_t* d_row_off, const uint32_t* d_member,
                                uint32_t r0, uint32_t r1, uint32_t ch, uint32_t n_kept, const uint64_t* d_u,
                                uint64_t* d_wcounts, int n_cu, hipStream_t s);
hipError_t hs_launch_cp_cover(const uint8_t* d_codes, int k, int alphabet, const double* d_S, const uint32_t* d_label,
                              const uint32_t* d_row_of, const uint32_t* d_row_off, const uint32_t* d_member,
                              uint32_t n_rows, uint32_t n_kept, uint32_t ch, uint64_t* d_key, double* d_min_score,
                              uint32_t* d_argmin, int n_cu, hipStream_t s);
// brute force
hipError_t hs_launch_bruteforce(const uint4* d_packed_all, uint32_t n, const float* d_tq,
                                uint32_t nq, int k, float r2_hi, uint32_t* d_prov_count,
                                uint32_t prov_cap, uint2* d_prov, const float* d_q_thr,
                                float* d_slice_min, int n_blocks, hipStream_t s, const double* d_radii = nullptr);
// bucket join (hs_join.hip)
hipError_t hs_launch_jtables(const double* d_coords, int alphabet, void* d_tab16, float* d_rownorm,
                             uint32_t* d_unsafe, hipStream_t s);
// d_radii (here and in the two int8 forms below): null, or every query's own radius [nq] in place of r2
hipError_t hs_launch_qprep(const double* d_centers, uint32_t nq, int k, double r2, void* d_c16,
                           uint32_t* d_unsafe, hipStream_t s, const double* d_radii = nullptr);
// items[j] for joined segments (>= min_q probing queries and >= min_m members), 0 otherwise, and
// nslices[ql] = 0 for the probes of joined segments; stats[0] += MFMA pairs issued, [1] += real pairs.
// Also the class flags of the item numbering order, n_max + 1 entries, the last 0: low half = joined with
// >= big_min_q probing queries, high half = joined with <= max_q_resident of them (0: no such class).
hipError_t hs_launch_seg_route(const uint64_t* d_seg_key, const uint32_t* d_seg_cnt,
                               const uint32_t* d_seg_qoff, const uint32_t* d_n_seg,
                               const uint32_t* d_sorted_ql, const uint32_t* d_qcount, uint32_t n_max,
                               uint32_t min_q, uint32_t min_m, uint32_t jm, int L, int shift,
                               uint32_t max_q_resident /* segments up to this many queries are issued in
                               16-query column tiles (hs_join8r_kernel); 0: none */,
                               uint32_t big_min_q, uint32_t* d_items, uint64_t* d_class,
                               unsigned long long* d_stats, uint32_t* d_nslices, const uint32_t* d_seg_of,
                               hipStream_t s,
                               uint32_t jm_stream = 0 /* members per item of the segments OUTSIDE the query-resident
                               class (hs_join6w_kernel: 192); 0: jm.  The same value to hs_launch_item_desc */);
hipError_t hs_launch_item_desc(const hs_tables_dev& tabs, const uint64_t* d_seg_key,
                               const uint32_t* d_seg_cnt,
                               const uint32_t* d_seg_qoff, const uint32_t* d_item_off, uint32_t n_max,
                               const uint32_t* d_sorted_ql, const uint32_t* d_qcount, uint32_t n_items,
                               uint32_t jm, int shift, const uint32_t* d_order, int PW,
                               const uint32_t* d_n_items /* null, or the device-side count: n_items is
                               then the capacity */,
                               const uint64_t* d_class_pos /* scan of the class flags, n_max + 1 entries */,
                               uint32_t* d_split /* [2]: first item of the query-resident class, items */,
                               uint32_t* d_split_copy /* null, or [2]: the same two words once more */,
                               uint4* d_desc, hipStream_t s, uint32_t jm_stream = 0);
// item numbering order of the segments: many-query segments first (stable two-class partition):
// class flags [n + 1] (last = 0; hs_launch_seg_route) -> hs_exclusive_scan_u64 -> d_class_pos [n + 1] ->
// d_order[n], d_items_ordered[n + 1] (last = 0)
// ... and LAST the segments with at most max_q_resident probing queries (d_res flags, null / 0: no such
// class): their items are the tail [split[0], split[1]) of the item list (hs_launch_item_desc), taken by the
// query-resident join kernel (hs_join8r_kernel)
hipError_t hs_launch_seg_order(const uint64_t* d_class_pos, const uint32_t* d_items, uint32_t n, uint32_t* d_order,
                               uint32_t* d_items_ordered, hipStream_t s);
// queries of a segment the query-resident join keeps in registers (two 32-query tiles: with three the
// kernel spills at two waves per SIMD)
#define HS_JR_MAXQ 64u
// ... and alphabets of up to this many residues (its pair table has eight copies of 32 x alphabet entries in LDS)
#define HS_JR_MAX_ALPHABET 24
// members per work item: 512 (one workgroup tile) for the staged kernels, 128 (one wave) for the
// wave-independent int8 join
#define HS_JM_BLOCK 512u
#define HS_JM_WAVE 128u
// queries per work item of the wave-independent join (a wave re-uses its members' operands over
// all of them; the staged kernel's items stop at 2048)
#ifndef HS_JQG_WAVE
#define HS_JQG_WAVE 8192u
#endif
hipError_t hs_launch_gather_c16(const void* d_c16, const uint32_t* d_sorted_ql, uint32_t nql, int L,
                                void* d_out, hipStream_t s);
hipError_t hs_launch_join(const uint4* d_desc, uint32_t n_items, const uint4* d_packed_base,
                          const uint32_t* d_sorted_ql, const void* d_c16s, const void* d_tab16,
                          const float* d_rownorm, int k, uint32_t* d_prov_count, uint32_t prov_cap,
                          uint2* d_prov, int n_blocks, hipStream_t s);
// int8 form of the join filter (hs_join8.hip)
// `wide` below: rows of short k-mers (k <= 20) carry all 8 coordinates on one scale (6 k-steps, table
// d_tabW, scale[4..6]); the launchers that take d_tab8 expect d_tabW in its place then
hipError_t hs_launch_jtables8(const double* d_coords, int alphabet, void* d_tab8, float* d_scale,
                              uint32_t* d_unsafe, void* d_tabR, void* d_tabW, hipStream_t s);
// d_c8b (may be null): the second row per query (columns 4..7 + the refinement's scalars), hs_refine8_kernel's
// input -- null for queries from codes, whose survivors hs_refine_codes_kernel refines without query rows
// the same rows for queries that are k-mers given as codes (self-join): x^ from the tables, no doubles
hipError_t hs_launch_qprep8_codes(const uint8_t* d_qcodes, uint32_t nq, int k, int wide, double r2,
                                  const double* d_coords, const void* d_tab8, const void* d_tabR,
                                  const void* d_tabW, const float* d_scale, void* d_c8, void* d_c8b,
                                  hipStream_t s, const double* d_radii = nullptr);
hipError_t hs_launch_qprep8(const double* d_centers, uint32_t nq, int k, int wide, double r2,
                            const float* d_scale, void* d_c8, uint32_t* d_unsafe, void* d_c8b,
                            hipStream_t s, const double* d_radii = nullptr);
// survivors of the 4-column bound -> those that also pass the 8-column bound (compacted, direct form)
hipError_t hs_launch_refine8(const hs_tables_dev& tabs, const uint2* d_prov, const uint32_t* d_prov_count,
                             uint32_t prov_cap, const uint32_t* d_sorted_ql, const void* d_c8,
                             const void* d_c8b, const void* d_tabR, const float* d_scale, int k, int L,
                             const uint32_t* d_qstart, const uint32_t* d_qcount,
                             uint2* d_out, uint32_t* d_out_count, hipStream_t s);
// the same step for queries that are k-mers (k <= 50): from the members' and the queries' packed words
// (d_qpacked, hs_launch_pack's) and an alphabet x alphabet table of squared distances -- no query rows
hipError_t hs_launch_refine_codes(const hs_tables_dev& tabs, const uint2* d_prov, const uint32_t* d_prov_count,
                                  uint32_t prov_cap, const uint32_t* d_sorted_ql, const uint4* d_qpacked,
                                  const double* d_coords, int alphabet, int k, int L, double r2,
                                  const double* d_radii, const uint32_t* d_qstart, const uint32_t* d_qcount,
                                  uint2* d_out, uint32_t* d_out_count, hipStream_t s);
hipError_t hs_launch_gather_c8t(const void* d_c8, const uint32_t* d_sorted_ql, const uint32_t* d_seg_qoff,
                                const uint32_t* d_seg_of, uint32_t nql, int L, int k, int wide, void* d_out,
                                hipStream_t s);
// bytes of a quantised int8 row (32 per k-step: 128 for k <= 25, 192 for k <= 41 and for wide rows,
// 256 for k <= 50) and the members of one work item of the wave-independent int8 join (128 / 64)
int hs_join8_row_bytes(int k, int wide);
uint32_t hs_join8_members_per_item(int k, int wide);
uint32_t hs_join8_chunk_items(uint32_t n_items, int n_blocks, double pairs_per_item, uint32_t chunk);
// hs_join6.hip: the FP6 (e2m3) form of the join for queries that are k-mers, k = 21..25, 4-column rows.
// d_tab6: hs_join6_table_bytes() bytes (hs_j6_dev); query rows of hs_join6_row_bytes() bytes, gathered into
// segment order by hs_launch_gather_c6t (the tile layout: hs_j6_tile_offset, hs_join6_tables.h); member records
// (16 bytes per bucket entry) parallel to the bucket-ordered packed copy.  G = items per counter access
// (hs_join8_chunk_items).
size_t hs_join6_table_bytes();
size_t hs_join6_ok_offset();  // of the int32 that says the tables are usable
int hs_join6_row_bytes();
uint32_t hs_join6_wide_item();
hipError_t hs_launch_gather_c6t(const void* d_c6, const uint32_t* d_sorted_ql, const uint32_t* d_seg_qoff,
                                const uint32_t* d_seg_of, uint32_t nql, int L, void* d_out, hipStream_t s);
hipError_t hs_launch_jtables6(const double* d_coords, int alphabet, void* d_tab6, hipStream_t s);
hipError_t hs_launch_gather_rec6(const uint4* d_packed_all, const uint32_t* d_ids_sorted, uint32_t n, int k,
                                 const void* d_tab6, uint4* d_out_rec, hipStream_t s);
hipError_t hs_launch_qprep6_codes(const uint8_t* d_qcodes, uint32_t nq, int k, double r2, const void* d_tab6,
                                  void* d_c6, hipStream_t s, const double* d_radii = nullptr);
hipError_t hs_launch_join6x(const uint4* d_desc, uint32_t n_items, const uint4* d_packed_base,
                            const uint4* d_rec_base, const void* d_c6t, const void* d_tab6, uint32_t* d_prov_count,
                            uint32_t prov_cap, uint2* d_prov, uint32_t* d_item_counter, int n_blocks,
                            const uint32_t* d_n_items, uint32_t G, uint32_t xcd_run, hipStream_t s,
                            int wide_items = 0 /* 1: hs_join6w_kernel, on items of hs_join6_wide_item() members */);
hipError_t hs_launch_join8w(const uint4* d_desc, uint32_t n_items, const uint4* d_packed_base,
                            const uint4* d_rec_base, const void* d_c8t, const void* d_tab8, int k, int wide,
                            uint32_t* d_prov_count, uint32_t prov_cap, uint2* d_prov,
                            uint32_t* d_item_counter, int n_blocks, const uint32_t* d_n_items,
                            double pairs_per_item, uint32_t xcd_run, hipStream_t s, uint32_t chunk = 0);
// the item list's tail [d_split[0], d_split[1]) (segments with <= HS_JR_MAXQ probing queries; k <= 25,
// 4-column rows) through the query-resident form; d_cn_rep = 128 copies of the gamma slots' constant
// factors (HS_J8_CONST bytes); the packed / record arrays must be readable 128 entries past their end
hipError_t hs_launch_join8r(const uint4* d_desc, uint32_t desc_cap, const uint32_t* d_split,
                            const uint4* d_packed_base, const uint32_t* d_rho_base /* the records in four bytes */,
                            const void* d_c8t,
                            const void* d_tab8, int alphabet /* <= HS_JR_MAX_ALPHABET */, uint32_t* d_prov_count, uint32_t prov_cap,
                            uint2* d_prov, uint32_t* d_item_counter, int n_blocks, double pairs_per_item,
                            hipStream_t s);
// bucket-ordered packed copy of one table (k <= 25) + the per-entry 16-byte A-row tails of the
// int8 join (d_out_rec[i] belongs to d_out_packed[i])
hipError_t hs_launch_gather_rec8(const uint4* d_packed_all, const uint32_t* d_ids_sorted, uint32_t n,
                                 int k, int wide, const void* d_tab8, const void* d_tabW, const float* d_scale,
                                 uint4* d_out_packed, uint4* d_out_rec,
                                 uint32_t* d_out_rho /* null, or the record in four bytes (hs_join8r_kernel) */,
                                 hipStream_t s);
hipError_t hs_launch_kth_min(const float* d_slice_min, uint32_t nq, uint32_t per_q, uint32_t topk,
                             float* d_thr, hipStream_t s);
hipError_t hs_launch_topk_exact(const uint8_t* d_codes, const double* d_centers,
                                const double* d_coords, const uint2* d_prov,
                                const uint32_t* d_prov_count, uint32_t prov_cap, int k,
                                uint64_t* d_key, uint64_t* d_val, hipStream_t s);
hipError_t hs_launch_bf_finalize(const uint8_t* d_codes, const double* d_centers,
                                 const double* d_coords, const uint2* d_prov,
                                 const uint32_t* d_prov_count, uint32_t prov_cap, int k, double R,
                                 uint32_t q_base, uint32_t* d_hit_count, uint32_t hit_cap,
                                 uint64_t* d_hit_key, uint64_t* d_hit_val, hipStream_t s,
                                 const double* d_radii = nullptr /* [nq] or null: R = radii[q] */);
// per-query radii of a call (hs_query_radii_dev): d_out[0] = the bits of max |radii[q]| as a double (0 for n = 0),
// d_out[1] = 1 if one of them is a NaN; d_out zeroed by the caller
hipError_t hs_launch_radii_max(const double* d_radii, uint64_t n, unsigned long long* d_out, hipStream_t s);

// ---- hs_index_append (hs_append.hip: the rule, the steps and the scratch are written at its head) ----------------
// match: per block bucket its place in the old directory -- d_pos = the bucket (d_is_new = 0; *d_flag |= 1 where the
// tuples differ as HashKey strings) or the insertion rank (d_is_new = 1, ++d_inc[rank]; d_inc [nb + 1] zeroed).
hipError_t hs_launch_append_match(const uint64_t* d_bkey, const int32_t* d_btuple, uint32_t nbB, int K,
                                  const uint64_t* d_dir_key, const int32_t* d_dir_tuple, const uint32_t* d_dir_jump,
                                  uint32_t jump_shift, uint32_t nb, uint32_t* d_pos, uint32_t* d_is_new,
                                  uint32_t* d_inc, uint32_t* d_flag, hipStream_t s);
// dir: the merged keys, tuples and COUNTS (d_new_scan / d_inc_scan: exclusive scans of d_is_new / d_inc), the maps old
// bucket -> merged and block bucket -> merged, and per block bucket the old members of its merged bucket
hipError_t hs_launch_append_dir(const uint64_t* d_dir_key, const uint32_t* d_dir_start, const int32_t* d_dir_tuple,
                                uint32_t nb, const uint64_t* d_bkey, const uint32_t* d_bstart, const int32_t* d_btuple,
                                uint32_t nbB, int K, const uint32_t* d_pos, const uint32_t* d_is_new,
                                const uint32_t* d_new_scan, const uint32_t* d_inc, const uint32_t* d_inc_scan,
                                uint32_t* d_map_old, uint32_t* d_map_blk, uint32_t* d_old_cnt, uint64_t* d_out_key,
                                int32_t* d_out_tuple, uint32_t* d_out_count, hipStream_t s);
// bases: destination = base[bucket] + source position, for the old table's entries and for the block's
hipError_t hs_launch_append_bases(const uint32_t* d_out_start, const uint32_t* d_dir_start, const uint32_t* d_map_old,
                                  uint32_t nb, const uint32_t* d_bstart, const uint32_t* d_map_blk,
                                  const uint32_t* d_old_cnt, uint32_t nbB, uint32_t* d_base_old, uint32_t* d_base_blk,
                                  hipStream_t s);
// move: entry p of the source arrays (n_seg non-empty segments d_seg_start [n_seg + 1]) to d_base[segment of p] + p of
// the destination arrays of n_dst entries; ids grow by id_add; d_dst_rec / d_dst_rho may be null
hipError_t hs_launch_append_move(uint32_t n_src, const uint32_t* d_seg_start, uint32_t n_seg, const uint32_t* d_base,
                                 uint32_t n_dst, int PW, const uint32_t* d_src_ids, uint32_t id_add,
                                 const uint4* d_src_packed, const uint4* d_src_rec, const uint32_t* d_src_rho,
                                 uint32_t* d_dst_ids, uint4* d_dst_packed, uint4* d_dst_rec, uint32_t* d_dst_rho,
                                 hipStream_t s);

// ---- hs_index_remove (hs_remove.hip: the rule, the steps and the scratch are written at its head) ----------------
// Keep masks: nw + 1 64-bit words for n positions (nw = ceil(n / 64); the last word is 0), counts [nw + 1]; the
// caller's exclusive scan of the counts over nw + 1 elements gives d_scan, whose last element is the survivors.
// mark: the dead bitmap d_dead [nw] (zeroed by the caller) from ids (*d_flag |= 1 for an id >= n) or from ranges
// (device arrays; the caller has checked that each ends inside n)
hipError_t hs_launch_remove_mark_ids(const uint32_t* d_ids, uint64_t m, uint32_t n, uint64_t* d_dead, uint32_t* d_flag,
                                     hipStream_t s);
hipError_t hs_launch_remove_mark_ranges(const uint64_t* d_first, const uint64_t* d_count, uint64_t n_ranges, uint32_t n,
                                        uint64_t* d_dead, hipStream_t s);
hipError_t hs_launch_remove_masks_ids(const uint64_t* d_dead, uint32_t n, uint64_t* d_mask, uint32_t* d_cnt,
                                      hipStream_t s);
hipError_t hs_launch_remove_new_id(const uint64_t* d_mask, const uint32_t* d_scan, uint32_t n, uint32_t* d_new_id,
                                   hipStream_t s);
hipError_t hs_launch_remove_masks_tab(const uint32_t* d_ids, const uint64_t* d_dead, uint32_t n, uint64_t* d_mask,
                                      uint32_t* d_cnt, hipStream_t s);
// dir_flags: d_alive / d_retuple [nb + 1] (the last 0).  dir_write: keys, counts and copied tuples of the nb_new alive
// buckets; for a retupled one the OLD id of its new first member and its new number, at d_retuple_scan[b] of
// d_need_id / d_need_bucket.  tuples_put: d_ints [n_need][K] to the listed buckets.
hipError_t hs_launch_remove_dir_flags(const uint32_t* d_dir_start, uint32_t nb, const uint64_t* d_mask,
                                      const uint32_t* d_scan, uint32_t* d_alive, uint32_t* d_retuple, hipStream_t s);
hipError_t hs_launch_remove_dir_write(const uint64_t* d_dir_key, const uint32_t* d_dir_start, const int32_t* d_dir_tuple,
                                      const uint32_t* d_ids, uint32_t nb, uint32_t n, int K, const uint64_t* d_mask,
                                      const uint32_t* d_scan, const uint32_t* d_alive, const uint32_t* d_alive_scan,
                                      const uint32_t* d_retuple, const uint32_t* d_retuple_scan, uint32_t nb_new,
                                      uint64_t* d_out_key, int32_t* d_out_tuple, uint32_t* d_out_count,
                                      uint32_t* d_need_id, uint32_t* d_need_bucket, hipStream_t s);
hipError_t hs_launch_remove_tuples_put(const int32_t* d_ints, const uint32_t* d_need_bucket, uint32_t n_need, int K,
                                       uint32_t nb_new, int32_t* d_out_tuple, hipStream_t s);
// move: surviving entry p of a table's arrays to rank(p) of the shrunken ones (n_dst entries), its id renumbered
// through d_new_id; d_dst_rec / d_dst_rho may be null
hipError_t hs_launch_remove_move(uint32_t n, uint32_t n_dst, const uint64_t* d_mask, const uint32_t* d_scan,
                                 const uint32_t* d_new_id, int PW, const uint32_t* d_src_ids, const uint4* d_src_packed,
                                 const uint4* d_src_rec, const uint32_t* d_src_rho, uint32_t* d_dst_ids,
                                 uint4* d_dst_packed, uint4* d_dst_rec, uint32_t* d_dst_rho, hipStream_t s);
// the id-order arrays: row i of codes [n][k] and of packed_all [n][PW] (d_packed_out may be null) to row d_new_id[i]
hipError_t hs_launch_remove_compact_ids(const uint8_t* d_codes, const uint4* d_packed_all, uint64_t n, int k, int PW,
                                        const uint32_t* d_new_id, uint32_t n_dst, uint8_t* d_codes_out,
                                        uint4* d_packed_out, hipStream_t s);

// ---- hs_pssm_scan (hs_pssm.hip: the filter, its layouts and the exact pass are written at its head) ---------------
size_t hs_pssm_prof_bytes(uint32_t k);       // per profile slot of a batch: the parameters and offsets hs_pssm_prep_kernel keeps
size_t hs_pssm_tile_bytes(uint32_t steps);   // per tile of 16 profiles: the B operands of all steps
// flag |= 1: an entry NaN, infinite or beyond 2^100; |= 2: a threshold NaN or infinite
hipError_t hs_launch_pssm_check(const double* d_S, uint64_t n_entries, const double* d_t, uint64_t nm, uint32_t* d_flag,
                                hipStream_t s);
// the batch's mb profiles (d_S, d_t: the batch's first) -> parameters and tau of ceil16(mb) slots, the B tiles, and
// *d_n_dead += the profiles no k-mer can hit
hipError_t hs_launch_pssm_prep(const double* d_S, const double* d_t, uint32_t mb, uint32_t k, uint32_t alphabet,
                               void* d_prof, float* d_tau, void* d_btiles, uint32_t* d_n_dead, hipStream_t s);
// survivors {profile of the batch, id} into d_prov through hs_reserve_survivors on d_prov_count
hipError_t hs_launch_pssm_filter(const uint4* d_packed_all, uint32_t n, int k, int alphabet, const void* d_btiles,
                                 const float* d_tau, uint32_t mb, uint32_t* d_prov_count, uint32_t prov_cap,
                                 uint2* d_prov, hipStream_t s);
// d_counters: the batch's counter block ([0] survivors, [1] hits); all_pairs: every pair of the batch, no list
hipError_t hs_launch_pssm_exact(const uint8_t* d_codes, const double* d_S, const double* d_t, int k, int alphabet,
                                uint32_t m_base, uint32_t mb, uint32_t n, const uint2* d_prov, uint32_t* d_counters,
                                uint32_t prov_cap, bool all_pairs, uint32_t hit_cap, uint64_t* d_hit_key,
                                uint64_t* d_hit_val, int n_cu, hipStream_t s);
hipError_t hs_launch_pssm_emit(const uint64_t* d_key, const uint64_t* d_val, uint32_t nh, bool write, uint32_t* d_out_m,
                               uint32_t* d_out_id, double* d_out_score, uint64_t* d_cnt, hipStream_t s);

// ---- hs_pssm_compare (hs_pssm_compare.hip: the kernels are written at its head; shapes: hs_pssm_compare.h) ----------
// np profiles d_P -> rows [ceil32(np)][row] (lead zero bytes, k columns of stride bytes, zeros) and their parameters
// [ceil32(np)] {s, l1, amax}
hipError_t hs_launch_pcmp_tables(const double* d_P, uint32_t np, uint32_t k, uint32_t alphabet, uint32_t stride,
                                 uint32_t lead, uint32_t row, void* d_rows, void* d_par, hipStream_t s);
size_t hs_pcmp_filter_lds(uint32_t k, uint32_t alphabet, uint32_t v);
// the batch's mb X rows against a chunk's nyc Y rows: survivors {x of the batch, y of the call} into d_prov through
// hs_reserve_survivors on d_prov_count.  x_base, y_base: the call's numbers of their first profiles; self: pairs with
// x >= y are left out
hipError_t hs_launch_pcmp_filter(const void* d_xq, const void* d_xpar, const double* d_t, uint32_t x_base, uint32_t mb,
                                 const void* d_yq, const void* d_ypar, uint32_t y_base, uint32_t nyc, uint32_t k,
                                 uint32_t alphabet, uint32_t v, bool self, uint32_t* d_prov_count, uint32_t prov_cap,
                                 uint2* d_prov, hipStream_t s);
// d_X, d_t: the batch's first; d_Y: the call's ny profiles.  d_counters: the batch's counter block ([0] survivors, [1]
// hits); all_pairs: every pair of the batch, no list
hipError_t hs_launch_pcmp_exact(const double* d_X, const double* d_Y, const double* d_t, uint32_t k, uint32_t alphabet,
                                uint32_t v, uint32_t x_base, uint32_t mb, uint32_t ny, bool self, const uint2* d_prov,
                                uint32_t* d_counters, uint32_t prov_cap, bool all_pairs, uint32_t hit_cap,
                                uint64_t* d_hit_key, uint64_t* d_hit_val, int n_cu, hipStream_t s);
hipError_t hs_launch_pcmp_emit(const uint64_t* d_key, const uint64_t* d_val, uint32_t nh, bool write, uint32_t* d_out_x,
                               uint32_t* d_out_y, int32_t* d_out_d, double* d_out_score, uint64_t* d_cnt,
                               hipStream_t s);

// ---- hs_pssm_topk (hs_pssm_topk.hip: the three steps of a batch are written at its head) ---------------------------
size_t hs_pssm_topk_temp(uint32_t count);    // the scan's workspace for a batch of `count` profiles
// t_used [mb] = max(floor, the topk-th best exact score among the n_s sample k-mers floor(j * n / n_s)); d_S, d_floor
// (may be null: no floor) and d_t_used are the batch's
// d_part_lists: hs_pssm_sample_part_bytes(mb, n_s) bytes (0 with one workgroup per profile: may be null then)
size_t hs_pssm_sample_part_bytes(uint32_t mb, uint32_t n_s);
hipError_t hs_launch_pssm_sample(const uint8_t* d_codes, const double* d_S, const double* d_floor, int k, int alphabet,
                                 uint32_t n, uint32_t n_s, uint32_t topk, uint32_t mb, void* d_part_lists,
                                 double* d_t_used, hipStream_t s);
// the batch's nh unordered hits (m << 32 | id, score bits) of profiles [first, first + count) -> rows first .. of the
// call's arrays, whole rows with their padding, and top_count; d_cnt / d_off / d_cur [count + 1], d_seg_* [nh];
// d_floor (may be null) and d_t_used are the batch's; *d_raised += the profiles with t_used above their floor
hipError_t hs_launch_pssm_topk_select(const uint64_t* d_key, const uint64_t* d_val, uint32_t nh, uint32_t first,
                                      uint32_t count, uint32_t* d_cnt, uint32_t* d_off, uint32_t* d_cur, void* d_temp,
                                      size_t temp_bytes, uint64_t* d_seg_d, uint64_t* d_seg_w, uint32_t topk,
                                      const double* d_floor, const double* d_t_used, uint32_t* d_top_id,
                                      double* d_top_score, uint32_t* d_top_count, uint64_t* d_raised, hipStream_t s);
// rows of padding, zero counts, t_used (may be null) = the floor: a call that ran no batch
hipError_t hs_launch_pssm_topk_fill(uint64_t rows, uint32_t topk, const double* d_floor, uint32_t* d_top_id,
                                    double* d_top_score, uint32_t* d_top_count, double* d_t_used, hipStream_t s);

// ---- hs_pssm_rank (hs_pssm_rank.hip: a round's three steps and the segmented radix select are written at its head) --
size_t hs_pssm_rank_state_bytes(uint32_t count);  // the select's state for `count` segments
size_t hs_pssm_rank_temp(uint32_t count);         // the scan's workspace for a batch of `count` profiles
uint32_t hs_pssm_rank_sample_batch(uint32_t n_s); // profiles per sub-batch of the sample pass (keys within 2^27 bytes)
// *d_flag |= 4 for a rank outside 1 .. n; *d_max_rank = max(*d_max_rank, the ranks)
hipError_t hs_launch_pssm_rank_check(const uint64_t* d_rank, uint64_t nm, uint64_t n, uint32_t* d_flag,
                                     uint64_t* d_max_rank, hipStream_t s);
// d_resolved [nm] = 0, *d_unresolved = 0
hipError_t hs_launch_pssm_rank_init(uint64_t nm, uint32_t* d_resolved, uint32_t* d_unresolved, hipStream_t s);
// the sample pass and its select for profiles m0 .. m0 + mb - 1 (every array is the CALL's): d_t_scan [m] = the plan's
// r_s-th largest sample score, -DBL_MAX beyond the sample, +DBL_MAX for a resolved profile; d_t_scan_out (may be null)
// takes the unresolved profiles' values.  d_keys [mb * n_s] (< 2^32), d_off [mb + 1], d_state of
// hs_pssm_rank_state_bytes(mb)
hipError_t hs_launch_pssm_rank_sample(const uint8_t* d_codes, const double* d_S, const uint64_t* d_rank,
                                      const uint32_t* d_resolved, int k, int alphabet, uint32_t n, uint32_t n_s,
                                      uint32_t round, uint32_t m0, uint32_t mb, uint64_t* d_keys, uint32_t* d_off,
                                      void* d_state, double* d_t_scan, double* d_t_scan_out, hipStream_t s);
// the batch's nh unordered hits (m << 32 | id, score bits) of profiles [first, first + count): the unresolved profiles
// with at least rank hits get t_rank, cnt_ge, cnt_gt, rounds (may be null) = round and are resolved; *d_unresolved +=
// the others.  d_cnt / d_off / d_cur [count + 1], d_seg [max(1, nh)], d_state of hs_pssm_rank_state_bytes(count)
hipError_t hs_launch_pssm_rank_select(const uint64_t* d_key, const uint64_t* d_val, uint32_t nh, uint32_t first,
                                      uint32_t count, uint32_t* d_cnt, uint32_t* d_off, uint32_t* d_cur, void* d_temp,
                                      size_t temp_bytes, uint64_t* d_seg, void* d_state, const uint64_t* d_rank,
                                      uint32_t* d_resolved, uint32_t round, double* d_t_rank, uint64_t* d_cnt_ge,
                                      uint64_t* d_cnt_gt, uint32_t* d_rounds, uint32_t* d_unresolved, hipStream_t s);

// ---- hs_pssm_pvalue (hs_pssm_null.hip: a batch's three steps are written at its head; the rule: hs_pssm_null.h) -------
size_t hs_pssm_null_prof_bytes(uint32_t mb);  // the parameters of a batch's profiles
// *d_flag |= 16: bg outside the rule; 32: a p outside (0, 1]; 64: a hit's profile >= nm; 128: a NaN hit score.  d_bg,
// d_p, d_hit_m (with d_hit_score) may be null: not checked
hipError_t hs_launch_pssm_null_check(const double* d_bg, uint32_t alphabet, const double* d_p, uint64_t nm,
                                     const uint32_t* d_hit_m, const double* d_hit_score, uint64_t n, uint32_t* d_flag,
                                     hipStream_t s);
// the batch's mb profiles (d_S, d_t_lo -- may be null: 0 -- the batch's first) -> d_prof, the bin shifts d_q_dn / d_q_up
// [mb][k][alphabet] (d_q_up untouched with sides == 1) and d_cdf [sides][mb][B]
hipError_t hs_launch_pssm_null_tables(const double* d_S, const double* d_bg, const double* d_t_lo, uint32_t mb,
                                      uint32_t k, uint32_t alphabet, uint32_t B, int sides, void* d_prof,
                                      uint16_t* d_q_dn, uint16_t* d_q_up, double* d_cdf, hipStream_t s);
// the call's n hits: those of profiles m0 .. m0 + mb - 1 get p_hi (and p_lo with sides == 2 and d_p_lo given)
hipError_t hs_launch_pssm_null_lookup(const void* d_prof, const double* d_cdf, uint32_t m0, uint32_t mb, uint32_t k,
                                      uint32_t alphabet, uint32_t B, int sides, const uint32_t* d_hit_m,
                                      const double* d_hit_score, uint64_t n, double* d_p_hi, double* d_p_lo,
                                      hipStream_t s);
// every array the batch's: t_p, the bracket at t_p, flag
hipError_t hs_launch_pssm_null_threshold(const void* d_prof, const double* d_cdf, uint32_t mb, uint32_t k,
                                         uint32_t alphabet, uint32_t B, int sides, const double* d_t_lo,
                                         const double* d_p, double* d_t_p, double* d_p_hi, double* d_p_lo,
                                         uint32_t* d_flag, hipStream_t s);

// ---- hs_pssm_seq_scan (hs_pssm_seq.hip: the passes over a batch's sorted hits are written at its head) -------------
// head: the n hits sorted by m << 32 | id -> d_seq [n] (the sequence of every hit) and d_head [n + 1] (row starts)
hipError_t hs_launch_pssm_seq_head(const uint64_t* d_key, uint32_t n, const uint64_t* d_id_start, uint64_t n_seq,
                                   uint32_t* d_seq, uint32_t* d_head, hipStream_t s);
// the search alone: d_seq [n]
hipError_t hs_launch_pssm_seq_of(const uint64_t* d_key, uint32_t n, const uint64_t* d_id_start, uint64_t n_seq,
                                 uint32_t* d_seq, hipStream_t s);
size_t hs_pssm_seq_part_bytes(uint32_t n);
// rows: d_excl = the exclusive scan of d_head over n + 1 elements, n_rows its total.  Scratch: d_row_start [n_rows + 1],
// d_row_key / d_row_id [n_rows], d_part of hs_pssm_seq_part_bytes(n) bytes.  write: the rows go to the seven output
// arrays (the batch's: already at the call's running offset); else only the counts.  *d_cnt [m] += the hits of every
// row of m, *d_seq_cnt [m] += its rows (either may be null).
hipError_t hs_launch_pssm_seq_rows(const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_seq,
                                   const uint32_t* d_head, const uint32_t* d_excl, uint32_t n, uint32_t n_rows,
                                   const uint64_t* d_id_start, bool write, uint32_t* d_row_start, uint64_t* d_row_key,
                                   uint32_t* d_row_id, void* d_part, uint32_t* d_out_m, uint32_t* d_out_seq,
                                   uint32_t* d_out_count, double* d_out_best_score, uint32_t* d_out_best_id,
                                   uint32_t* d_out_lo, uint32_t* d_out_hi, uint64_t* d_cnt, uint64_t* d_seq_cnt,
                                   hipStream_t s);

// ---- hs_pssm_family_scan (hs_pssm_family.hip: the passes over a batch's sorted hits are written at its head) --------
struct HsFamilyOut;  // hs_pssm_family.h: the ten row arrays
// *d_flag |= the HS_FAM_BAD_* bits of d_m_group [nm], d_m_off [nm], d_t_group [n_groups] (each may be null)
hipError_t hs_launch_pssm_family_check(const uint32_t* d_m_group, const uint32_t* d_m_off, const double* d_t_group,
                                       uint64_t nm, uint64_t n_groups, uint32_t* d_flag, hipStream_t s);
// the n hits sorted by m << 32 | id and their sequences -> d_row_key [n], d_idx [n] = 0 .. n - 1; d_cnt [m] += the
// hits of every profile (may be null)
hipError_t hs_launch_pssm_family_key(const uint64_t* d_key, const uint32_t* d_seq, uint32_t n, const uint32_t* d_m_group,
                                     const uint32_t* d_m_off, const uint64_t* d_id_start, int ws, int wd,
                                     uint64_t max_off, uint64_t* d_row_key, uint32_t* d_idx, uint64_t* d_cnt,
                                     hipStream_t s);
// d_skey / d_sidx: the pairs sorted on the row key; d_head [n + 1] their run heads, d_excl its exclusive scan, n_rows
// its total.  Scratch: d_row_start [n_rows + 1], d_rows of 48 n_rows bytes (HsFamilyOut::in), d_keep [n_rows + 1]: the
// filters' flags
hipError_t hs_launch_pssm_family_rows(const uint64_t* d_skey, const uint32_t* d_sidx, const uint32_t* d_head,
                                      const uint32_t* d_excl, uint32_t n, uint32_t n_rows, const uint64_t* d_key,
                                      const uint64_t* d_val, const uint64_t* d_id_start, int ws, int wd,
                                      uint64_t max_off, uint32_t min_count, const double* d_t_group,
                                      uint32_t* d_row_start, void* d_rows, uint32_t* d_keep, hipStream_t s);
// d_pos = the exclusive scan of d_keep.  write: the kept rows go to out (the batch's: already at the call's running
// offset); d_grp_rows [g] += the kept rows of every group (may be null)
hipError_t hs_launch_pssm_family_write(const void* d_rows, const uint32_t* d_keep, const uint32_t* d_pos,
                                       uint32_t n_rows, bool write, const HsFamilyOut& out, uint64_t* d_grp_rows,
                                       hipStream_t s);

// ---- hs_pssm_family_chain (hs_pssm_chain.hip: the passes over a batch's sorted hits are written at its head) --------
struct HsChainOut;  // hs_pssm_chain.h: the ten row arrays
size_t hs_pssm_chain_state_bytes(uint32_t n);  // d_state of a batch of n hits
// d_skey / d_sidx: the (g << ws | s, hit index) pairs sorted on the key; d_head [n + 1] their run heads, d_excl its
// exclusive scan, n_segs its total.  Scratch: d_seg_start [n_segs + 1], d_state, d_rows of 44 n_segs bytes
// (HsChainOut::in), d_keep [n_segs + 1]: whether a segment reports a row
hipError_t hs_launch_pssm_chain(const uint64_t* d_skey, const uint32_t* d_sidx, const uint32_t* d_head,
                                const uint32_t* d_excl, uint32_t n, uint32_t n_segs, const uint64_t* d_key,
                                const uint64_t* d_val, const uint64_t* d_id_start, const uint32_t* d_m_off, int ws,
                                uint32_t max_shift, double gap_open, double gap_ext, uint32_t min_count,
                                const double* d_t_group, uint32_t* d_seg_start, void* d_state, void* d_rows,
                                uint32_t* d_keep, hipStream_t s);
// d_pos = the exclusive scan of d_keep.  write: the kept rows go to out (the batch's: already at the call's running
// offset); d_grp_rows [g] += the kept rows of every group (may be null)
hipError_t hs_launch_pssm_chain_write(const void* d_rows, const uint32_t* d_keep, const uint32_t* d_pos, uint32_t n_segs,
                                      bool write, const HsChainOut& out, uint64_t* d_grp_rows, hipStream_t s);

// ---- hs_pssm_hit_counts (hs_pssm_counts.hip: the passes over a batch's sites are written at its head) --------------
// the batch's n hits m << 32 | id -> d_m [n], d_id [n]
hipError_t hs_launch_pssm_counts_split(const uint64_t* d_key, uint32_t n, uint32_t* d_m, uint32_t* d_id, hipStream_t s);
// d_site_m [ns] ascending, every m in [m0, m0 + mb) -> d_start [mb + 1] (the profiles' runs) and d_n_item [mb + 1]
// (their chunks of ch sites; the last is 0)
hipError_t hs_launch_pssm_counts_items(const uint32_t* d_site_m, uint32_t ns, uint32_t m0, uint32_t mb, uint32_t ch,
                                       uint32_t* d_start, uint32_t* d_n_item, hipStream_t s);
// d_off = the exclusive scan of d_n_item over mb + 1 elements, n_items its total; d_counts [nm][k][alphabet] is the
// call's, zeroed before the first batch
hipError_t hs_launch_pssm_counts(const uint8_t* d_codes, int k, int alphabet, const uint32_t* d_site_id,
                                 const uint32_t* d_start, const uint32_t* d_off, uint32_t m0, uint32_t mb, uint32_t ch,
                                 uint32_t n_items, uint32_t* d_counts, hipStream_t s);
// d_used [nm], d_cnt [nm] (either may be null) = the sites of every profile, from the finished counts
hipError_t hs_launch_pssm_counts_used(const uint32_t* d_counts, uint32_t nm, int k, int alphabet, uint64_t* d_used,
                                      uint64_t* d_cnt, hipStream_t s);

// ---- hs_pssm_weighted_counts (hs_pssm_weights.hip: the second sink stage of a batch is written at its head) --------
size_t hs_pssm_weights_table_bytes(uint32_t mb, int k, int alphabet);  // d_u of a batch
// the batch's finished d_counts [mb][k][alphabet] -> d_u [mb][k][alphabet], d_distinct [mb] (may be null)
hipError_t hs_launch_pssm_weights_table(const uint32_t* d_counts, uint32_t mb, int k, int alphabet, uint64_t* d_u,
                                        uint32_t* d_distinct, hipStream_t s);
// the sites, runs and items of hs_launch_pssm_counts; d_wcounts [nm][k][alphabet] is the call's, zeroed before the
// first batch
hipError_t hs_launch_pssm_weights(const uint8_t* d_codes, int k, int alphabet, const uint32_t* d_site_id,
                                  const uint32_t* d_start, const uint32_t* d_off, uint32_t m0, uint32_t mb, uint32_t ch,
                                  uint32_t n_items, const uint64_t* d_u, uint64_t* d_wcounts, hipStream_t s);
// d_wsum [nm] (may be null) from the finished d_wcounts
hipError_t hs_launch_pssm_weights_sum(const uint64_t* d_wcounts, uint32_t nm, int k, int alphabet, uint64_t* d_wsum,
                                      hipStream_t s);

#endif
