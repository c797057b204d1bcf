// hs_handle.h -- the handle behind include/hsearch.h, private to the host layer of the C ABI: the types struct hs_handle
// is made of, the error macros and internal statuses of a call, and the survivor-capacity loop every batch runs under
// (filter_passes: a template, so that the query path and the profile path each get their pass inlined).  Included by
// hs_capi.hip (the handle's life, the queries and what reduces their hits), hs_capi_index.hip (the index calls) and
// hs_capi_pssm.hip (the profile calls).  The types have external linkage on purpose: all of them must see ONE struct
// hs_handle.  Its layout depends on -DHS_TEST_HOOKS (Knobs), so every file that includes this is compiled once with
// and once without it.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "../../include/hs_tables.h"
#include "hs_internal.h"

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// host staging kept across calls (pageable: page-locking 40 MB took longer than a whole
// Clustering() of 10^6 k-mers; what is saved is the fresh allocation + page faults per call)
struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    free(p);
    cap = 0;
    p = malloc(bytes);
    if (!p) return hipErrorOutOfMemory;
    memset(p, 0, bytes);  // touch the pages here: a device -> host copy into untouched pages crawls
    cap = bytes;
    return hipSuccess;
  }
  void release() {
    free(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

enum { EV_COUNT = 12 };
enum { EV_FORK = 0, EV_JOIN = 1, EVX_COUNT = 2 };

// Switches of a handle (hs_set_option, include/hsearch.h; read_knobs for the few that come from the
// environment).  None of them changes a result: each forces one of several equivalent paths (the tests run
// both and compare), sizes a batch, or prints a diagnostic.  Fault injection (HS_TEST_SPLIT_ABOVE) exists only
// in the test build of the library (-DHS_TEST_HOOKS: libhsearch_amd_hooks.so), never in libhsearch_amd.so.
struct Knobs {
  bool build_serial = false;       // HS_OPT_BUILD_SERIAL: no hash / sort overlap in the build (measurement)
  int join_xcd_run = -1;           // HS_OPT_JOIN_XCD_RUN: chunks per XCD-local run of join items (0 off, -1 auto)
  bool no_probe_records = false;   // HS_OPT_PROBE_RECORDS = 0: the probe reads the directory arrays, not the records
  uint32_t join_chunk = 0;         // HS_OPT_JOIN_CHUNK: items per counter access of hs_join8x_kernel (0: by itself)
  bool build_debug = false;        // HS_BUILD_DEBUG: say when a table is sorted a second time; hs_index_append: its stages' host time
  bool cluster_timing = false;     // HS_CLUSTER_TIMING: phase times of hs_self_join_range on stderr
  bool debug_refine = false;       // HS_DEBUG_REFINE: survivor counts per batch on stderr
  bool force_wide = false;         // HS_OPT_WIDE_ROWS = 1: 8-column rows whatever the radius (k <= 25)
  bool no_wide_by_radius = false;  // HS_OPT_WIDE_ROWS >= 2: never choose 8-column rows by radius
  bool no_refine8 = false;         // HS_OPT_REFINE8 = 0: no 8-column refinement of the join's survivors
  bool no_join_f6 = false;         // HS_OPT_JOIN_F6 = 0: k-mer queries never through the FP6 join (hs_join6.hip)
  int join_f6_form = -1;           // HS_OPT_JOIN_F6_FORM: 0 hs_join6x_kernel, 1 hs_join6w_kernel, -1 automatic
  bool no_pssm_filter = false;     // HS_OPT_PSSM_FILTER = 0: hs_pssm_scan sends every pair to the exact pass (hs_pssm.hip)
  bool no_pssm_cmp_filter = false; // HS_OPT_PSSM_CMP_FILTER = 0: hs_pssm_compare sends every pair to the exact pass
  bool no_self_codes = false;      // HS_OPT_SELF_CODES = 0: self-join from embedded centres, not from codes
  bool sort_hits = false;          // HS_OPT_SORT_HITS: order hits by the radix sort, not per query
  bool sync_items = false;         // HS_OPT_SYNC_ITEMS: read the join's item count back before launching it
  bool no_join_r = false;          // HS_OPT_JOIN_RESIDENT = 1: every segment through the query-streaming join kernel
  bool no_recognise = false;       // HS_OPT_RECOGNISE_KMERS = 0: centres that are k-mers are not looked for (run_query)
  bool force_join_r = false;       // HS_OPT_JOIN_RESIDENT = 2: the query-resident kernel for its class whatever its share
  bool build_sort = false;         // HS_OPT_BUILD_GROUPING = 1: group a table's k-mers by sorting (fingerprint, id) pairs
                                   // (rocPRIM; rounds 1-2) instead of hs_group.hip's table + rank sort
  int seg_mode = 0;                // HS_OPT_SEG_MODE: 1 sparse / 2 dense; 0 = by the bucket : probe ratio
  int sort_from_bit = 16;          // HS_OPT_SORT_FROM_BIT: lowest fingerprint bit the build's sort looks at
  uint32_t query_batch = 0;        // HS_OPT_QUERY_BATCH: queries per batch (0: by L and the free HBM)
  uint32_t pssm_topk_sample = 262144;  // HS_OPT_PSSM_TOPK_SAMPLE: k-mers the sample pass of hs_pssm_topk scores per profile
  uint32_t pssm_rank_sample = 262144;  // HS_OPT_PSSM_RANK_SAMPLE: k-mers the sample pass of hs_pssm_rank scores per profile
  uint32_t pssm_null_bins = 4096;  // HS_OPT_PSSM_NULL_BINS: bins of hs_pssm_pvalue's score grid (64 .. 8192)
  uint32_t pssm_count_chunk = 0;   // HS_OPT_PSSM_COUNT_CHUNK: sites per work item of hs_pssm_counts.hip (0: by the batch)
  uint32_t summary_chunk = 0;      // HS_OPT_SUMMARY_CHUNK: member slots per work item of hs_summary.hip (0: 512)
  uint32_t summary_rows = 0;       // HS_OPT_SUMMARY_ROWS: rows per batch of hs_cluster_profile (0: by the scratch budget)
  int64_t msf_edge_budget = -1;    // HS_OPT_MSF_EDGE_BUDGET: bytes of HBM hs_msf may keep pairs in (0 never, -1 a share of the free)
#ifdef HS_TEST_HOOKS
  uint32_t test_split_above = 0;   // HS_TEST_SPLIT_ABOVE: batches above this size report a survivor overflow
  bool test_group_fallback = false;  // HS_TEST_GROUP_FALLBACK: the build's fingerprint table reports itself full
  bool test_append_collision = false;  // HS_TEST_APPEND_COLLISION: hs_index_append's match step reports a collision
  bool test_remove_reseed = false;     // HS_TEST_REMOVE_RESEED: hs_index_remove treats the index's seed as non-zero
  bool test_rec6_no_room = false;      // HS_TEST_REC6_NO_ROOM: the FP6 member records report that they found no room
#endif
};

// What becomes of a batch's hits once the batch has come through whole (run_query, reduce_batch).  LIST: ordered and
// handed out in the call's output arrays.  Every other sink reduces them where finalize_hits leaves them -- no
// ordering, no output arrays (cap = 0), no capacity verdict:
//   ANNOTATE   hs_annotate: the nearest centre per DB id (annot_reduce)
//   CC_UNION   hs_components: a self-join's pairs united in the handle's union-find forest
//   DB_DEGREE  hs_degrees / hs_dbscan pass 1 (hs_dbscan.hip): a self-join's pairs counted into the degree array
//   DB_UNITE   hs_dbscan pass 2: the degrees known, the pairs united and anchored at min_pts
//   MSF_MIN_D, MSF_MIN_PAIR   hs_msf (hs_msf.hip): steps 1 and 2 of a Boruvka round over a self-join's pairs
//   MSF_COLLECT               hs_msf's first pass: step 1, and the pairs appended to the list kept in HBM
//   DT_CORE, DT_CORE_COLLECT  hs_core_distance / hs_density_tree (hs_density.hip): the core pass -- the threshold
//                             rounds over the batch's hits at min_pts; COLLECT: and the pairs appended to the kept list
//   DT_MIN_D, DT_MIN_PAIR     hs_density_tree: steps 1 and 2 of a Boruvka round under the mutual-reachability weight
//   TOPK       hs_query_topk / hs_self_knn (hs_knn.hip): per query of the batch the topk smallest hits under (dist, id),
//              written as rows row0 + (the query's number in the call) of the four device arrays (topk_reduce)
//   SEQ_MATCH  hs_seq_match (hs_seqmatch.hip): the batch's hits reduced per (query group, sequence, diagonal) and the
//              rows appended to the handle's list (seq_reduce); the list is reduced once more at the end of the call
struct SeqMatchCall {
  const uint32_t* q_group = nullptr;  // device; null: a query is its own group
  const uint32_t* q_off = nullptr;    // device; null: no diagonals
  const uint64_t* id_start = nullptr; // device, [n_seq + 1]
  uint64_t n_groups = 0, n_seq = 0, max_qoff = 0;
  int wg = 0, ws = 0, wd = 0;         // the key's field widths (include/hsearch.h)
};

struct HitSink {
  enum Kind { LIST, ANNOTATE, CC_UNION, DB_DEGREE, DB_UNITE, MSF_MIN_D, MSF_MIN_PAIR, MSF_COLLECT, DT_CORE,
              DT_CORE_COLLECT, DT_MIN_D, DT_MIN_PAIR, TOPK, SEQ_MATCH } kind = LIST;
  uint32_t min_pts = 1;
  uint32_t topk = 0;
  uint64_t row0 = 0;
  uint32_t* nn_id = nullptr;
  uint32_t* nn_table = nullptr;  // (may stay null)
  double* nn_dist = nullptr;
  uint32_t* nn_count = nullptr;
  const SeqMatchCall* sm = nullptr;
};

// One query call's queries and what it asks (run_query, query_batch, probe_tabs)
struct QueryCall {
  const double* centers = nullptr;
  const uint8_t* codes = nullptr;  // queries given as residue codes [nq][k] (hs_query_codes); centers unused
  double R = 0.0;                  // with radii: the largest |radii[q]| of the call, what plan_batch decides from
  bool brute = false;
  uint32_t self_first = HS_NO_SELF;  // self-join: DB id of query 0
  bool sqrt_test = false;            // hit test sqrt(d2) <= R (hclust2.cpp:119-120) instead of d2 <= R*R
  // multi-probe (mp_query): every row is one probe of a query, its bucket ints given ([nq][L][K], device) in
  // place of the hash, and pre_valid[q L + l] == 0 an empty probe
  const int32_t* pre_ints = nullptr;
  const uint8_t* pre_valid = nullptr;
  // hs_query_radii: every query's own radius ([nq], device); null: R for all.  Searches and brute force only.
  const double* radii = nullptr;
  HitSink sink;
};

// What a handle learns from its batches to steer the next ones (plan_batch, the join launch); written by
// learn_from_batch alone, forgotten with the index (drop_index)
struct BatchHistory {
  // work items of the last joined batch x 1.25: with it the next batch sizes its descriptor array
  // without asking the device (the kernels clamp to the real count; an overflow repeats the batch)
  uint32_t item_cap_hint = 0;
  double pairs_per_item = 0.0;  // average of the previous batch's join work items (0: none yet)
  // share of the last joined batch's work items that lay in segments with few probing queries (the
  // query-resident kernel's class); < 0: unknown.  That kernel pays when the class is the bulk of the items
  // (configs[2]'s shape: 90 %); where it is a minority (configs[1]: the extra launch costs more than the
  // class's items cost in the streaming kernel) the next batch runs everything through the streaming kernel
  double resident_share = -1.0;
  uint32_t resident_age = 0;  // joined batches since it was measured (measured again every 64)
  uint32_t resident_nq = 0;   // ... on a batch of this many queries (a batch half / twice that size measures anew)
  // the last batch that ordered its hits itself had to fall back to the sort, at this radius (NaN after a
  // batch with per-query radii: such a batch neither leaves a radius to match nor matches one)
  bool order_failed = false;
  double order_failed_R = 0.0;
};

struct hs_handle {
  hs_params p;
  int d = 0, LK = 0, PW = 0, alphabet = HS_ALPHABET;
  int n_cu = 256;
  hipStream_t stream = nullptr;
  hipEvent_t ev[EV_COUNT];
  bool ev_ok = false;
  // side stream: the streaming filter (and its per-query tables) runs beside the bucket join
  hipStream_t stream2 = nullptr;
  hipEvent_t evx[EVX_COUNT];
  bool evx_ok = false;
  DevBuf a, b, coords;
  DevBuf aT;  // the planes transposed, [d][L*K]: what the hash kernels read
  // index
  bool built = false;
  uint64_t n = 0;
  uint32_t key_seed = 0;
  DevBuf codes, packed_all;
  DevBuf t_dirkey[HS_MAX_L], t_dirstart[HS_MAX_L], t_dirtuple[HS_MAX_L], t_ids[HS_MAX_L];
  DevBuf t_dirjump;  // the jump tables of all directories, one allocation (a table's at its own offset)
  DevBuf t_dirrec;   // the directory records of all tables (hs_table_dev::dir_rec), 64 bytes per bucket
  DevBuf part_work;  // bucket partition: flags, positions, compacted (bucket, probe) pairs of a batch
  DevBuf t_giant;    // the fingerprints of every table's giant buckets (hs_table_dev::giant_key), ascending
  uint32_t bucket_part = 0, bucket_parts = 1;  // hs_set_bucket_partition
  // bucket-ordered packed copies of all tables in ONE allocation ([L][n][PW]), and the int8 join's
  // per-entry records ([L][n], k <= 50 only) at the same entry numbers
  DevBuf t_packed, t_rec8;
  // the records once more in four bytes per entry ([L][n]; k <= 25 with 4-column rows: what the
  // query-resident join kernel reads instead of t_rec8 -- it is bound by the bytes it moves per member)
  DevBuf t_rho;
  DevBuf hit_kv;     // query_batch: the hits bucketed by query, (key, value) side by side
  DevBuf hit_rank;   // query_batch: a hit's number among its query's hits (ordering without a sort)
  DevBuf qpacked;    // query_batch: queries given as k-mers, packed like the members (exact pass)
  DevBuf rec_codes;  // run_query: the residue codes of centres that turned out to be k-mers (+ the counter)
  // member records of the wide rows for k = 21..25 (built when a call's radius first asks for them)
  DevBuf t_rec8w;
  bool rec8w_ready = false;
  // the FP6 join (hs_join6.hip): its tables, and the member records (16 bytes per entry and table), built on the
  // first batch that can use them; rec6_state: 0 not built, 1 ready, -1 no room for them (int8 join for this index)
  DevBuf jtab6, t_rec6;
  int rec6_state = 0;
  bool join6_tables_ok = false;
  double pair4_mean = 0.0, pair4_var = 0.0;  // 4-column squared distance of two random residues
  DevBuf t_pos;  // [L][n] sorted position of every DB id in every table (first-seen dedupe)
  DevBuf dir_base;       // [L + 1] first global bucket number of every table; [L] = nb_total
  uint32_t nb_total = 0;  // buckets of all tables
  DevBuf bucket_work;    // per-batch: counts + their 64-bit double scan over the nb_total + 2 bucket slots
  hs_tables_dev tabs;
  hs_index_info info;
  // query workspace (grown on demand, reused across calls)
  DevBuf qints, qstart, qcount, nslices, slice_off, tq, prov, hit_key, hit_val, hit_key2, hit_val2,
      counters, temp, io_centers, io_q, io_id, io_table, io_dist, io_cand, io_codes, io_misc;
  // multi-probe (hs_set_multiprobe): extra probes per table; a chunk's exact projections and fractions, its
  // probes' bucket ints and flags, its queries once per probe, the probe rows' hits and candidate counts
  uint32_t mp_T = 0;
  uint64_t mp_room = 0;
  DevBuf mp_pts, mp_codes, mp_ints, mp_frac, mp_vints, mp_valid, mp_rows, mp_q, mp_id, mp_table, mp_dist, mp_cand;
  DevBuf mp_radii;   // ... and, for a call with per-query radii, the probe rows' radii
  // hs_annotate (hs_annotate.hip): smallest distance and its (table, q) per DB id, the ids touched by the call and
  // their count, the touched ids sorted.  ann_clean: slots [0, ann_clean) of ann_dist are known to be empty;
  // ann_open: a call is (or ended early while) reducing -- the next one empties all slots first
  DevBuf ann_dist, ann_tq, ann_touched, ann_sorted, ann_cnt;
  uint64_t ann_clean = 0;
  bool ann_open = false;
  // hs_components (hs_components.hip): the union-find forest over the indexed k-mers (parent[x] <= x), the
  // call's two 64-bit counts {ordered pairs, roots}, and the labels of a host-pointer call on their way out
  DevBuf cc_parent, cc_cnt, cc_label;
  // hs_degrees / hs_dbscan (hs_dbscan.hip): the degree and the smallest core neighbour per indexed k-mer (the forest
  // is cc_parent: every call starts it from the identity), and the call's five 64-bit counts
  DevBuf db_deg, db_anchor, db_cnt;
  // hs_msf (hs_msf.hip: the state listed at its head; the forest is cc_parent): the components of the round, the two
  // slots per component, the tree edges and their sorted copy, the call's counts; the list of pairs kept in HBM, the
  // entries the call may keep (HS_OPT_MSF_EDGE_BUDGET) and whether the list could not grow to hold a batch
  DevBuf msf_comp, msf_best_d, msf_best_pair, msf_out_pair, msf_out_d, msf_s_pair, msf_s_d, msf_cnt, msf_kept;
  uint64_t msf_kept_budget = 0;
  bool msf_kept_failed = false;
  // hs_core_distance / hs_density_tree (hs_density.hip: the state listed at its head; the rest is hs_msf's): the core
  // distance bits, the threshold and the round's minimum per indexed k-mer, the neighbours counted
  DevBuf dt_core, dt_thr, dt_next, dt_cnt;
  // hs_query_topk / hs_self_knn (hs_knn.hip: the scratch listed at its head, all sized by a batch): hits per query,
  // their scan, the scatter's cursors, the call's 64-bit hit count; the counts of a host-pointer call on their way out
  DevBuf knn_cnt, knn_off, knn_cur, knn_total, knn_io_count;
  // hs_pssm_topk (hs_pssm_topk.hip; the selection's scratch is hs_knn.hip's): a batch's thresholds when the caller
  // wants none; the sample pass's lists when a profile's sample is split over several workgroups
  DevBuf pt_tused, pt_parts;
  // hs_pssm_rank (hs_pssm_rank.hip; the hit selection's counts, offsets and cursors are hs_knn.hip's): a sub-batch's
  // sample keys, their segment offsets, the select's state; the call's resolved flags, scan thresholds, and the word
  // that counts a round's unresolved profiles; a host-pointer call's ranks in and outputs on their way out
  DevBuf pr_keys, pr_off, pr_state, pr_resolved, pr_tscan, pr_unres, pr_rank, pr_out;
  // hs_pssm_pvalue / hs_pssm_pvalue_threshold (hs_pssm_null.hip): a batch's parameters, bin shifts (both sides) and cdf
  // tables; the background and the check's words; a host-pointer call's arrays in and out
  DevBuf pn_prof, pn_q, pn_cdf, pn_bg, pn_chk, pn_in, pn_out;
  // hs_pssm_hit_counts (hs_pssm_counts.hip): a batch's sites as (m, id) words and their copies sorted on m, the
  // profiles' run starts, chunk counts and their scan, the rows of the one-site-per-protein mode; a host-pointer
  // call's counts, cnt and used on their way out
  DevBuf pc_m, pc_id, pc_m2, pc_id2, pc_start, pc_nitem, pc_off, pc_rows, pc_out;
  // hs_pssm_weighted_counts (hs_pssm_weights.hip): a batch's u tables; the raw counts of a call that does not ask for
  // them; a host-pointer call's wcounts, wsum and distinct on their way out
  DevBuf pw_u, pw_counts, pw_out;
  // hs_pssm_compare (hs_pssm_compare.hip): the int8 rows of an X batch and of a Y chunk, their parameters
  // {s, l1, amax} per profile; a host-pointer call's Y on its way up
  DevBuf pcm_xq, pcm_yq, pcm_xpar, pcm_ypar, pcm_y;
  // hs_seq_match (hs_seqmatch.hip: the scratch listed at its head): a batch's keys and hit indices, their sorted
  // copies, the run heads and their scan, the waves' cut runs; the call's rows so far (sq_rows of them in a list of
  // sq_acc.cap / 40) and their final reduction; the argument check's words; a host-pointer call's arrays in and out
  DevBuf sq_key, sq_idx, sq_skey, sq_sidx, sq_head, sq_excl, sq_part, sq_acc, sq_fin, sq_chk, sq_in, sq_out;
  uint64_t sq_rows = 0;
  uint32_t sq_batches = 0;
  // hs_pssm_family_scan (hs_pssm_family.hip; the keys, heads and scans of a batch's hits are the sq_ buffers above): the
  // hit indices sorted on the row key, the rows' run starts, the rows before the filters, the filters' flags and their
  // scan; a host-pointer call's m_group, m_off and t_group on their way up
  DevBuf pf_sidx, pf_start, pf_rows, pf_keep, pf_pos, pf_in;
  // hs_pssm_family_chain (hs_pssm_chain.hip; keys, sorts, starts, flags and inputs are the sq_ and pf_ buffers above):
  // the chain state of a batch's hits by sorted position, the segments' rows before the filters
  DevBuf pch_state, pch_rows;
  // hs_cluster_profile / hs_cluster_radii (hs_summary.hip: the state listed at its head), the counts of a row batch
  // when the caller wants none, and the arrays of a host-pointer call on their way in and out.  hs_cluster_weighted_profile
  // / hs_cluster_pssm_cover (hs_cluster_pssm.hip) run on the same state: a row batch's u tables go to pw_u, the members'
  // score keys to sm_d2, the profiles' value check to word 1 of sm_err; a host-pointer call's wcounts, wsum and distinct
  // leave through pw_out, its profiles come in through io_centers, min_score / argmin leave through sm_io_f64 / sm_io_a
  DevBuf sm_size, sm_tmp, sm_row_of, sm_off_of, sm_row_label, sm_row_off, sm_member, sm_d2, sm_err, sm_counts;
  // host-pointer calls: the labels in; out, hs_cluster_profile: sm_io_a = out_label, sm_io_b = out_size, sm_io_counts,
  // sm_io_f64 = centroid; hs_cluster_radii (centres in through io_centers, as the searches' are): sm_io_f64 = max_d2,
  // sm_io_f64b = radius, sm_io_a = medoid
  DevBuf sm_io_label, sm_io_a, sm_io_b, sm_io_counts, sm_io_f64, sm_io_f64b;
  DevBuf io_radii;   // hs_query_radii: the radii on the device; hs_query_radii_dev: {max |radius|, NaN flag}
  DevBuf qcodes_buf, qembed;  // hs_query_codes: a batch's checked copy of the query codes; their embedding
                              // when no from-codes path applies
  HostBuf sj_host;  // hs_self_join_range: hits of one chunk on their way to the edge lists
  // bucket-join workspace
  // hs_index_build_subset: the caller's whole code array, kept on the device across calls
  DevBuf all_codes, subset_ids;
  const uint8_t* all_codes_key = nullptr;
  uint64_t all_codes_n = 0;
  DevBuf bs_ints2[2], bs_keys2[2], bs_iota2[2], bs_keys_sorted, bs_rle_unique, bs_rle_counts, bs_small,
      bs_sort_temp, bs_slow_q;  // index-build scratch (build_tables)
  DevBuf bs_fptab, bs_blk, bs_dk, bs_hist, bs_rank;  // ... of the table + rank-sort grouping (hs_group.hip)
  // hs_index_shard_*: the build with the hashing spread over ranks (this rank's block of the k-mers)
  bool shard_open = false;
  uint32_t shard_lo = 0, shard_cnt = 0, shard_seed = 0, shard_nb = 0;
  int shard_table = -1;
  DevBuf seg_of;    // query_batch: the segment of every sorted probe position
  DevBuf seg_res;   // cut_items: the scan of the segments' class flags (many queries | query-resident kernel)
  DevBuf c16s, item_desc, probe_slow, jtab8, qhits;  // qhits: per-query hit counts, offsets, fill
  DevBuf c8b, prov2;  // survivor refinement: second int8 row per query, the refined survivor list
  bool join8_tables_ok = false;  // int8 can carry the coordinate table
  double join8_scale = 0.0, join8_scale_w = 0.0;  // quantisation scales: 4-column rows, wide rows
  bool wide8_ok = false;         // the 8-column table is usable (wide rows on demand for k = 21..25)
  uint32_t* pin_cnt = nullptr;   // HS_CNT_WORDS pinned words: where a pass's counter block lands, in one copy (small
                                 // device -> host copies into PAGEABLE memory cost ~ 50 us of host staging per batch)
  BatchHistory hist;
  Knobs knobs;
  bool wide8 = false;            // short k-mers: int8 rows over all 8 coordinate columns (hs_join8.hip)
  // segment routing thresholds (HS_JOIN_MIN_Q / _M): segments with fewer probing queries or members
  // go to the per-pair filters instead of the join.  1 / 1 = everything through the join: its
  // persistent waves leave no room for a kernel beside it, and the per-pair filter run before it
  // cost 0.3 ms at C2 (a chain of dependent loads per probe) against 0.06 ms of extra join time
  uint32_t join_min_q = 1, join_min_m = 1;
  int join_blocks_per_cu = 2;                // resident workgroups of hs_join_kernel per CU
  DevBuf jtab, c16, seg_keys, seg_keys_sorted, seg_vals, sorted_ql, seg_key, seg_cnt, seg_qoff,
      seg_items, item_off, seg_n;
  // projection on the matrix cores (hs_proj.hip): quantised planes in both tilings, per-function
  // constants, the quantised coordinate table, flag lists (0/1: the two tables in flight during a
  // build, 2: queries and the hash entry points) and their counters {reserved, real} x 3
  int proj_S = 0;               // k-steps the MFMA pass is compiled for (0: k too long)
  bool proj_usable = false;     // S > 0 and the buffers below are filled for the current planes
  bool proj_auto = false;       // ... and the error bound is narrow enough for the auto mode
  int hash_mode = 0;            // 0 auto, 1 exact fp64 kernel, 2 MFMA pass wherever usable
  double proj_eps_scale = 1.0;
  double proj_est = 0.0;        // typical half-width of the bound, in bucket units
  DevBuf proj_aq_all, proj_aq_tab, proj_fn, proj_tab, proj_stats, proj_flags[3], proj_cnt, proj_xq, proj_xmeta;
  bool join_tables_ok = false;  // fp16 can carry the coordinate table
  int verify_mode = 0;          // 0 auto, 1 streaming kernel, 2 bucket join
  std::string err;
  hs_profile prof;
};

// Defined once, in hs_capi.hip.  fail: the handle's error text and the status to return; ev_ms: milliseconds between
// two of the handle's events; ensure_device: the calling thread on the handle's GPU; ensure_pin_cnt: the pinned words
// a pass's counter block lands in.
hs_status fail(hs_handle* h, hs_status st, const std::string& msg);
float ev_ms(hs_handle* h, int i0, int i1);
hs_status ensure_device(hs_handle* h);
hs_status ensure_pin_cnt(hs_handle* h);
// ... and what the index calls (hs_capi_index.hip) share with the rest.  drop_index: the index is about to change or go;
// hash_dispatch: bucket ints of one table's functions (or all) for n points on a stream, set = which flag list and
// counter pair; hash_account: the pass's statistics into the profile, after a synchronisation of that stream.
void drop_index(hs_handle* h);
hs_status hash_dispatch(hs_handle* h, const uint8_t* d_codes, const double* d_pts, uint64_t n, int table, int32_t* out,
                        int out_stride, int set, hipStream_t s);
hs_status hash_account(hs_handle* h, uint64_t n, int F, int set);

#define HS_HIP(h, expr)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(h, e_ == hipErrorOutOfMemory ? HS_ERR_NOMEM : HS_ERR_HIP,                  \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                        \
  } while (0)
#define HS_CHECK(expr)                \
  do {                                \
    hs_status st_ = (expr);           \
    if (st_ != HS_OK) return st_;     \
  } while (0)

// Counters block (h->counters): [0] prov_count u32, [1] hit_count u32, [2..3] cand_total u64, ...,
// [20] hits not ordered on the device, [21] HS_CNT_SURVIVOR_OVERFLOW, [32] the join's item counter.
// Internal status: the batch's filters passed more pairs than the 32-bit survivor counter holds.
static const hs_status HS_SPLIT_BATCH = (hs_status)1000;
// Internal status: a batch that left its item count on the device found it over the capacity hint, or a
// query row the join cannot carry; the batch runs again with the count read back first.
static const hs_status HS_SYNC_ITEMS = (hs_status)1001;

inline int bit_width_u32(uint32_t v) {
  int b = 0;
  while (v) {
    ++b;
    v >>= 1;
  }
  return b;
}

// the topk every selecting call takes (hs_query_topk, hs_self_knn, hs_pssm_topk)
inline bool topk_ok(uint32_t topk) { return topk >= 1 && topk <= HS_TOPK_MAX; }

// The survivor-capacity loop of a batch: pass(prov_cap, hit_cap, again) issues the filters and the exact
// decision, recording ev[3] / ev[4] / ev[5] around them (ev[11] .. ev[10] around the join when join_timed), and
// the counters' read-back; it runs again with a longer survivor list while the filters pass more than the
// list holds.  item_cap > 0: the batch left its item count on the device with room for that many items.
// On success: the timings, the survivors and the hit count (*n_hits) accounted.
template <class Pass>
hs_status filter_passes(hs_handle* h, uint32_t nq, uint32_t item_cap, bool join_timed, uint32_t* n_hits,
                        Pass pass) {
  uint32_t* const d_cnt = h->counters.as<uint32_t>();
  uint32_t prov_cap = (uint32_t)std::max<size_t>(h->prov.cap / 8, std::max<size_t>(1u << 20, 16ull * nq));
  HS_CHECK(ensure_pin_cnt(h));
  const uint32_t* const host_cnt = h->pin_cnt;
  memset(h->pin_cnt, 0, HS_CNT_WORDS * 4);
  double ms_verify = 0, ms_final = 0, ms_join = 0;
  uint32_t launches = 0;
  for (;;) {
    HS_HIP(h, h->prov.reserve((size_t)prov_cap * 8));
    const uint32_t hit_cap = (uint32_t)std::max<size_t>(h->hit_key.cap / 8, prov_cap);
    HS_HIP(h, h->hit_key.reserve((size_t)hit_cap * 8));
    HS_HIP(h, h->hit_val.reserve((size_t)hit_cap * 8));
    // (first pass: both callers have just cleared all the counters)
    if (launches) HS_HIP(h, hipMemsetAsync(d_cnt, 0, 8, h->stream));
    HS_CHECK(pass(prov_cap, hit_cap, launches != 0));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    // > ~4e9 survivors: run_query halves the batch (HS_TEST_SPLIT_ABOVE=n: as if every batch of more
    // than n queries had overflowed -- the tests' handle on the splitting logic)
    if (host_cnt[HS_CNT_SURVIVOR_OVERFLOW]) return HS_SPLIT_BATCH;
#ifdef HS_TEST_HOOKS
    if (h->knobs.test_split_above && nq > h->knobs.test_split_above) return HS_SPLIT_BATCH;
#endif
    if (host_cnt[HS_CNT_BAD_QUERY_CODE])
      return fail(h, HS_ERR_INVALID, "residue code outside the alphabet in the queries");
    if (item_cap && (host_cnt[8] /* join legality */ || host_cnt[HS_CNT_SPLIT + 1] > item_cap)) return HS_SYNC_ITEMS;
    ms_verify += ev_ms(h, 3, 4);
    if (join_timed) ms_join += ev_ms(h, 11, 10);
    ms_final += ev_ms(h, 4, 5);
    ++launches;
    if (h->knobs.debug_refine)
      fprintf(stderr, "survivors %u -> refined %u -> hits %u\n", host_cnt[0], host_cnt[4], host_cnt[1]);
    if (host_cnt[0] <= prov_cap) break;  // hit_count <= prov_count <= prov_cap <= hit_cap
    // the survivor list was too short: once more with room for what the filters reported (64-bit
    // arithmetic: the count may sit just under the overflow flag's 0xF0000000).  The six lists of the
    // exact pass are sized from it -- 48 bytes per entry -- so beyond 2^30 entries, or when the device
    // has no room for them, the batch is cut in halves like a counter overflow instead.
    const uint64_t need = (uint64_t)host_cnt[0] + host_cnt[0] / 8 + 1024;
    if (need > (1ull << 30) && nq > 1) return HS_SPLIT_BATCH;
    if (need > 0xffffffffull) return fail(h, HS_ERR_CAPACITY, "the filter survivors of one query exceed the survivor list");
    const uint64_t have = prov_cap;
    prov_cap = (uint32_t)need;
    if (nq > 1) {  // can the lists grow?  (a failed reserve keeps the old buffer's size at 0: re-reserved below)
      const size_t bytes = (size_t)prov_cap * 8;
      if (h->prov.reserve(bytes) != hipSuccess || h->hit_key.reserve(bytes) != hipSuccess ||
          h->hit_val.reserve(bytes) != hipSuccess) {
        (void)hipGetLastError();
        prov_cap = (uint32_t)have;
        return HS_SPLIT_BATCH;
      }
    }
  }
  h->prof.ms_hash += ev_ms(h, 0, 1);
  h->prof.ms_probe += ev_ms(h, 1, 2);
  h->prof.ms_verify += ms_verify;
  h->prof.ms_finalize += ms_final;
  h->prof.ms_join += ms_join;
  h->prof.verify_launches += launches;
  h->prof.provisional += host_cnt[0];
  *n_hits = host_cnt[1];
  return HS_OK;
}
