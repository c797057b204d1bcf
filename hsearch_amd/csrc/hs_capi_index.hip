// hs_capi_index.hip -- the index calls of include/hsearch.h: build (from codes, from a subset, from windows, or with
// the hashing spread over ranks), append, remove, save / load.  The handle and what these calls share with the
// queries (drop_index, hash_dispatch, hash_account): hs_handle.h.
//
// HBM layout of an index (N k-mers of k residues, L tables, PW = ceil(k/25) 16-byte words):
//   codes       [N][k]      u8   original order (exact fp64 re-evaluation of survivors)
//   packed_all  [N][PW]     u128 5-bit residues, original order (brute force scans this)
//   per table l:
//     ids       [N]         u32  DB ids grouped by bucket, ascending inside a bucket
//     packed    [N][PW]     u128 the same k-mers in bucket order -> a bucket is ONE contiguous,
//                                coalesced stream for the verify kernel (no gather at query time)
//     dir_key   [nb]        u64  sorted fingerprints of the distinct HashKey strings
//     dir_start [nb+1]      u32  bucket boundaries
//     dir_tuple [nb][K]     i32  bucket ints of each bucket (exact string check at probe time)
//
// What the calls share, each once:
//   rows_of, reserve_table_rows, row_slice   which bucket-ordered rows an index carries, their sizes, table l's part
//   gather_rows, gather_table_rows           a table's rows filled from its ids
//   publish_table, NewTables, adopt_tables   a table as the kernels get it; a new set of tables taking the old one's place
//   pack_checked                             packing with the residue check, refused in the caller's words
//   begin_index, end_index, finish_index     how a new index starts and how every index ends
//   reserve_directory, directory_from_runs   a table's directory, and its keys and boundaries from sorted runs
//   release_if_large                         scratch kept for the next build only while it is small
//   build_tables = hash_table, group_by_rank | group_by_sort, finish_table per table, under one BuildCtx
#include <string.h>

#include <algorithm>
#include <chrono>
#include <initializer_list>
#include <string>
#include <vector>

#include "hs_handle.h"
#include "hs_table_append.h"
#include "hs_table_remove.h"

namespace {

// ---- the layout of the tables ------------------------------------------------------------------------------------
// Which rows a table carries beside its ids, packed k-mers and positions: the int8 member records of the bucket join
// (hs_join8.hip) and, with their 4-column form, the rho words.
struct TableRows {
  bool rec8, rho;
};
TableRows rows_of(const hs_handle* h) {
  const int k = (int)h->p.k;
  const bool rec8 = h->join8_tables_ok && k <= 50;
  return {rec8, rec8 && k <= 25 && !h->wide8};
}

// The bucket-ordered rows of the L tables of n k-mers each, table l's from entry l * n on.
// (+ 128 entries: hs_join8r_kernel reads a bucket's ragged last member tile without clamping)
hs_status reserve_table_rows(hs_handle* h, DevBuf& packed, DevBuf& rec8, DevBuf& rho, DevBuf& pos, uint64_t n) {
  const int L = (int)h->p.L, PW = h->PW;
  const TableRows rows = rows_of(h);
  HS_HIP(h, packed.reserve(((size_t)L * n + HS_JM_WAVE) * PW * 16));
  if (rows.rec8) HS_HIP(h, rec8.reserve(((size_t)L * n + HS_JM_WAVE) * 16));
  if (rows.rho) HS_HIP(h, rho.reserve(((size_t)L * n + HS_JM_WAVE + 4) * 4));
  HS_HIP(h, pos.reserve(std::max<size_t>(16, (size_t)L * n * 4)));
  return HS_OK;
}

// table l's part of those arrays; null where the index does not carry the row
struct RowSlice {
  uint4 *packed, *rec8;
  uint32_t *rho, *pos;
};
RowSlice row_slice(const hs_handle* h, const DevBuf& packed, const DevBuf& rec8, const DevBuf& rho, const DevBuf& pos,
                   int l, uint64_t n) {
  const TableRows rows = rows_of(h);
  const size_t at = (size_t)l * n;
  return {packed.as<uint4>() + at * h->PW, rows.rec8 ? rec8.as<uint4>() + at : nullptr,
          rows.rho ? rho.as<uint32_t>() + at : nullptr, pos.as<uint32_t>() + at};
}
RowSlice table_slice(const hs_handle* h, int l, uint64_t n) {
  return row_slice(h, h->t_packed, h->t_rec8, h->t_rho, h->t_pos, l, n);
}

// n packed k-mers of src through ids into bucket order: with their member records (rec8 given; the 4-column table of
// jtab8 or the 8-column one of the wide rows, and the scales) and rho words (rho given), or alone
hs_status gather_rows(hs_handle* h, const uint4* src, const uint32_t* ids, uint64_t n, uint4* packed, uint4* rec8,
                      uint32_t* rho) {
  if (rec8)
    HS_HIP(h, hs_launch_gather_rec8(src, ids, (uint32_t)n, (int)h->p.k, h->wide8, h->jtab8.p,
                                    h->jtab8.as<char>() + 1536, h->jtab8.as<float>() + 128, packed, rec8, rho, h->stream));
  else
    HS_HIP(h, hs_launch_gather_packed(src, ids, n, h->PW, packed, h->stream));
  return HS_OK;
}

// table l's rows from its ids (n of them) and the index's packed k-mers; with_pos: and the positions from the ids
hs_status gather_table_rows(hs_handle* h, int l, uint64_t n, bool with_pos) {
  const RowSlice s = table_slice(h, l, n);
  const uint32_t* ids = h->t_ids[l].as<uint32_t>();
  HS_CHECK(gather_rows(h, h->packed_all.as<uint4>(), ids, n, s.packed, s.rec8, s.rho));
  if (with_pos) HS_HIP(h, hs_launch_invert_perm(ids, (uint32_t)n, s.pos, h->stream));
  return HS_OK;
}

// table l of n k-mers in nb buckets as the kernels get it (info.max_bucket[l] is the caller's: each learns it its own way)
void publish_table(hs_handle* h, int l, uint64_t n, uint64_t nb) {
  const RowSlice s = table_slice(h, l, n);
  hs_table_dev& tb = h->tabs.t[l];
  tb.dir_key = h->t_dirkey[l].as<uint64_t>();
  tb.dir_start = h->t_dirstart[l].as<uint32_t>();
  tb.dir_tuple = h->t_dirtuple[l].as<int32_t>();
  tb.packed = s.packed;
  tb.ids = h->t_ids[l].as<uint32_t>();
  tb.pos_of = s.pos;
  tb.nb = (uint32_t)nb;
  h->info.n_buckets[l] = nb;
}

// device buffers of one call, given back when it ends
struct BufGuard {
  std::vector<DevBuf*> b;
  ~BufGuard() { for (DevBuf* x : b) x->release(); }
};

// The tables an append or a removal writes beside the handle's: freed with the call unless adopt_tables has made
// them the handle's, and then the handle's old ones are.
struct NewTables {
  const int L;  // the handle's number of tables: as many of the per-table buffers are used
  DevBuf packed, rec8, rho, pos, ids[HS_MAX_L], key[HS_MAX_L], start[HS_MAX_L], tuple[HS_MAX_L];
  explicit NewTables(const hs_handle* h) : L((int)h->p.L) {}
  RowSlice slice(const hs_handle* h, int l, uint64_t n2) const { return row_slice(h, packed, rec8, rho, pos, l, n2); }
  ~NewTables() {
    for (DevBuf* x : {&packed, &rec8, &rho, &pos}) x->release();
    for (int l = 0; l < L; ++l)
      for (DevBuf* x : {&ids[l], &key[l], &start[l], &tuple[l]}) x->release();
  }
};
void adopt_tables(hs_handle* h, uint64_t n2, NewTables& t, const uint64_t* new_nb, const uint64_t* new_max) {
  std::swap(h->t_packed, t.packed);
  std::swap(h->t_rec8, t.rec8);
  std::swap(h->t_rho, t.rho);
  std::swap(h->t_pos, t.pos);
  for (int l = 0; l < (int)h->p.L; ++l) {
    std::swap(h->t_ids[l], t.ids[l]);
    std::swap(h->t_dirkey[l], t.key[l]);
    std::swap(h->t_dirstart[l], t.start[l]);
    std::swap(h->t_dirtuple[l], t.tuple[l]);
    publish_table(h, l, n2, new_nb[l]);
    h->info.max_bucket[l] = new_max[l];
  }
}

// n k-mers of d_codes packed into d_packed, the residue codes checked on the way: one outside the alphabet is refused
// with the caller's status and words.  beside: host work done between the kernel's launch and the wait for its verdict.
// It exists for index_build_resident alone, which makes the build's allocations there (reserve_build_buffers): made
// after the wait, with the GPU idle, they were 6.5 of a first build's 30 ms.
hs_status pack_checked(hs_handle* h, const uint8_t* d_codes, uint64_t n, uint4* d_packed, hs_status refused,
                       const char* message, hs_status (*beside)(hs_handle*) = nullptr) {
  HS_HIP(h, hipMemsetAsync(h->counters.p, 0, 256, h->stream));
  HS_HIP(h, hs_launch_pack(d_codes, n, (int)h->p.k, h->alphabet, d_packed, h->counters.as<uint32_t>(), h->stream));
  if (beside) HS_CHECK(beside(h));
  uint32_t bad = 0;
  HS_HIP(h, hipMemcpyAsync(&bad, h->counters.p, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (bad) return fail(h, refused, message);
  return HS_OK;
}

// A new index of n k-mers starts: the old one is gone, the profile and the info are clear, the codes have their
// room, and the build's clock (ev[8] .. ev[9], end_index) runs.
hs_status begin_index(hs_handle* h, uint64_t n) {
  drop_index(h);
  h->n = n;
  memset(&h->prof, 0, sizeof(h->prof));
  memset(&h->info, 0, sizeof(h->info));
  HS_HIP(h, h->codes.reserve(std::max<size_t>(16, (size_t)n * h->p.k)));
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  return HS_OK;
}

// a directory of nb buckets: fingerprints, boundaries, bucket ints
hs_status reserve_directory(hs_handle* h, DevBuf& key, DevBuf& start, DevBuf& tuple, uint64_t nb) {
  HS_HIP(h, key.reserve(std::max<size_t>(16, (size_t)nb * 8)));
  HS_HIP(h, start.reserve(((size_t)nb + 1) * 4));
  HS_HIP(h, tuple.reserve(std::max<size_t>(16, (size_t)nb * h->p.K * 4)));
  return HS_OK;
}
hs_status reserve_directory(hs_handle* h, int l, uint64_t nb) {
  return reserve_directory(h, h->t_dirkey[l], h->t_dirstart[l], h->t_dirtuple[l], nb);
}

// Table l's fingerprints and boundaries from the run-length encoding of its n sorted fingerprints (bs_rle_unique,
// bs_rle_counts: nb runs); the largest bucket goes to bs_small[2].  The bucket ints are the caller's.
hs_status directory_from_runs(hs_handle* h, int l, uint32_t nb, uint64_t n) {
  HS_CHECK(reserve_directory(h, l, nb));
  uint32_t* counts = h->bs_rle_counts.as<uint32_t>();
  uint32_t* start = h->t_dirstart[l].as<uint32_t>();
  if (nb) {
    HS_HIP(h, hipMemcpyAsync(h->t_dirkey[l].p, h->bs_rle_unique.p, (size_t)nb * 8, hipMemcpyDeviceToDevice, h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(h->bs_sort_temp.p, h->bs_sort_temp.cap, counts, start, nb, h->stream));
    HS_HIP(h, hs_launch_max_u32(counts, nb, h->bs_small.as<uint32_t>() + 2, h->stream));
  }
  HS_HIP(h, hs_launch_set_u32(start + nb, (uint32_t)n, h->stream));
  return HS_OK;
}

// Build scratch stays for the next build while it is small beside the device's memory (1/16 of it: 2.2 GB at the
// C2 sizes stay -- freeing them took 2.5 ms of a 23 ms build --, 22 GB at the C3 shape go).
void release_if_large(std::initializer_list<DevBuf*> b) {
  size_t held = 0, free_b = 0, total_b = 0;
  for (DevBuf* x : b) held += x->cap;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = (size_t)16 << 30;
  if (held > total_b / 16)
    for (DevBuf* x : b) x->release();
}

// ---- build ---------------------------------------------------------------------------------------------------------
// The allocations of a build, all sized by n alone.  index_build_resident makes them while the packing kernel (and
// the copy of the codes before it) still runs: an allocation costs ~ 0.3 ms whatever its size, and a first build
// makes two dozen of them -- with the GPU idle, they were 6.5 of its 30 ms at the C2 sizes.  build_tables calls
// this again as its first step (no-ops then; the allocations themselves for an empty index, which packs nothing).
hs_status reserve_build_buffers(hs_handle* h) {
  const uint64_t n = h->n;
  const int K = (int)h->p.K, L = (int)h->p.L;
  for (int i = 0; i < 2; ++i) {
    HS_HIP(h, h->bs_ints2[i].reserve(std::max<size_t>(16, (size_t)n * K * 4)));
    HS_HIP(h, h->bs_keys2[i].reserve(std::max<size_t>(16, (size_t)n * 8)));
    HS_HIP(h, h->bs_iota2[i].reserve(std::max<size_t>(16, (size_t)n * 4)));
  }
  HS_HIP(h, h->bs_keys_sorted.reserve(std::max<size_t>(16, (size_t)n * 8)));
  HS_HIP(h, h->bs_rle_unique.reserve(std::max<size_t>(16, (size_t)n * 8)));
  HS_HIP(h, h->bs_rle_counts.reserve(std::max<size_t>(16, (size_t)n * 4)));
  HS_HIP(h, h->bs_small.reserve(64));  // [0]=runs [1]=collision flag [2]=max count
  HS_HIP(h, h->bs_sort_temp.reserve(std::max(std::max(hs_sort_pairs_u64_u32_temp(n), hs_rle_u64_temp(n)),
                                             hs_scan_u32_temp(n + 1)) + 256));
  HS_CHECK(reserve_table_rows(h, h->t_packed, h->t_rec8, h->t_rho, h->t_pos, n));
  for (int l = 0; l < L; ++l) HS_HIP(h, h->t_ids[l].reserve(std::max<size_t>(16, (size_t)n * 4)));
  if (!h->knobs.build_sort && n && n < (1ull << 31)) {  // what group_by_rank works in
    const uint32_t C = hs_group_table_slots(n), n_blk = (C + 1023) / 1024, n_tiles = hs_rs_blocks(n);
    HS_HIP(h, h->bs_fptab.reserve((size_t)C * 8));    // the slots: 64-bit fingerprints
    HS_HIP(h, h->bs_blk.reserve(2 * ((size_t)n_blk + 2) * 4));
    HS_HIP(h, h->bs_rank.reserve((size_t)n * 4));
    HS_HIP(h, h->bs_hist.reserve(2 * (size_t)((size_t)256 * n_tiles + 64) * 4));
  }
  return HS_OK;
}

// One build_tables call.  The scratch is shared by all tables and lives in the handle (bs_*: Clustering() rebuilds a
// 10^6-k-mer index per table, and twelve hipMalloc / hipFree pairs per build cost more than the build's kernels).
// Hashing (fp64 vector ALU) and grouping (radix sort: memory) of consecutive tables overlap: table l + 1 is hashed on
// the side stream into the other half of the double-buffered ints / keys / iota while table l is grouped on the main
// stream.
struct BuildCtx {
  hs_handle* h;
  uint32_t seed;
  // The hash runs on the handle's side stream (lowest priority: the sort's many small kernels get
  // the CUs they ask for, the hash fills the rest).  Measured at 10 M x 8 tables, repeated builds:
  // 44 ms without the overlap, 40 ms with it (the sort slows from 20 to 27 ms beside the hash); a
  // normal-priority stream gave 44 ms; a CU-masked stream (hipExtStreamCreateWithCUMask) reserving
  // a quarter of the CUs for the sort hung in the second build of a process and was dropped.
  hipStream_t hash_stream;
  // grouping by key: hs_group.hip (table of distinct fingerprints + a radix sort on 32-bit ranks) unless
  // HS_BUILD_SORT asks for the full-width sort of rounds 1-2 (which also remains the fallback of a table
  // the other path cannot take: a fingerprint equal to its empty marker, or nearly all keys distinct)
  bool group_by_rank;
  bool serial;  // measurement: no overlap
  hipEvent_t ev_hashed[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};
  hipEvent_t ev_t[4] = {nullptr, nullptr, nullptr, nullptr};  // hash start/end per buffer
  double ms_hash = 0, ms_sort = 0, ms_gather = 0;
  ~BuildCtx() {
    // nothing may still be running on either stream when the scratch goes away
    if (hash_stream) (void)hipStreamSynchronize(hash_stream);
    (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t e : {ev_hashed[0], ev_hashed[1], ev_free[0], ev_free[1], ev_t[0], ev_t[1], ev_t[2], ev_t[3]})
      if (e) (void)hipEventDestroy(e);
    release_if_large({&h->bs_ints2[0], &h->bs_ints2[1], &h->bs_keys2[0], &h->bs_keys2[1], &h->bs_iota2[0],
                      &h->bs_iota2[1], &h->bs_keys_sorted, &h->bs_rle_unique, &h->bs_rle_counts, &h->bs_small,
                      &h->bs_sort_temp, &h->bs_slow_q, &h->bs_fptab, &h->bs_blk, &h->bs_dk, &h->bs_hist, &h->bs_rank});
  }
};

// hash + fingerprints of table t into buffer t & 1, on the side stream
hs_status hash_table(BuildCtx& c, int t) {
  hs_handle* h = c.h;
  const uint64_t n = h->n;
  const int K = (int)h->p.K, u = t & 1;
  if (t >= 2) HS_HIP(h, hipStreamWaitEvent(c.hash_stream, c.ev_free[u], 0));  // table t - 2 is done with it
  HS_HIP(h, hipEventRecord(c.ev_t[2 * u], c.hash_stream));
  HS_CHECK(hash_dispatch(h, h->codes.as<uint8_t>(), nullptr, n, t, h->bs_ints2[u].as<int32_t>(), K, u, c.hash_stream));
  if (!c.group_by_rank)  // (hs_group.hip fingerprints the bucket ints itself, in its one pass over them)
    HS_HIP(h, hs_launch_keys(h->bs_ints2[u].as<int32_t>(), n, K, K, c.seed, h->bs_keys2[u].as<uint64_t>(),
                             h->bs_iota2[u].as<uint32_t>(), c.hash_stream));
  HS_HIP(h, hipEventRecord(c.ev_t[2 * u + 1], c.hash_stream));
  HS_HIP(h, hipEventRecord(c.ev_hashed[u], c.hash_stream));
  return HS_OK;
}

// Table l (n >= 1) grouped through the table of its distinct fingerprints and a radix sort on their 32-bit ranks:
// ids, directory and largest bucket (bs_small[2]) on the stream, *nb and *grouped = true on return.  The membership
// proof's verdict (bs_small[1] bit 0) is still on its way: finish_table reads it.  A table this path cannot take stays
// ungrouped, with its fingerprints and ids 0 .. n - 1 made ready for group_by_sort.
hs_status group_by_rank(BuildCtx& c, int l, uint32_t* nb_out, bool* grouped) {
  hs_handle* h = c.h;
  const uint64_t n = h->n;
  const int K = (int)h->p.K;
  const int32_t* ints = h->bs_ints2[l & 1].as<int32_t>();
  uint32_t* d_small = h->bs_small.as<uint32_t>();
  DevBuf& sort_temp = h->bs_sort_temp;
  const uint32_t C = hs_group_table_slots(n), n_blk = (C + 1023) / 1024, n_tiles = hs_rs_blocks(n);
  uint32_t* blk_cnt = h->bs_blk.as<uint32_t>();
  uint32_t* blk_off = blk_cnt + n_blk + 2;
  uint32_t* rank = h->bs_rank.as<uint32_t>();
  HS_HIP(h, hs_launch_group_insert(ints, n, K, c.seed, h->bs_fptab.as<uint64_t>(), C, rank, d_small + 1, h->stream));
  HS_HIP(h, hs_launch_fp_count(h->bs_fptab.as<uint64_t>(), C, blk_cnt, h->stream));
  HS_HIP(h, hipMemsetAsync(blk_cnt + n_blk, 0, 4, h->stream));
  HS_HIP(h, hs_exclusive_scan_u32(sort_temp.p, sort_temp.cap, blk_cnt, blk_off, (size_t)n_blk + 1, h->stream));
  uint32_t host2[2] = {0, 0};
  HS_HIP(h, hipMemcpyAsync(&host2[0], blk_off + n_blk, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(&host2[1], d_small + 1, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));   // the table's one round trip: its number of buckets
#ifdef HS_TEST_HOOKS
  if (h->knobs.test_group_fallback && (l & 1)) host2[1] |= 16u;  // (every other table, so that both forms mix)
#endif
  if (host2[1] & 48u) {
    if (h->knobs.build_debug)
      fprintf(stderr, "table %d: grouping by rank not possible (flag 0x%x), sorting\n", l, host2[1]);
    HS_HIP(h, hipMemsetAsync(d_small, 0, 64, h->stream));
    // the sorting path needs the fingerprints and the ids 0 .. n - 1 as its values
    HS_HIP(h, hs_launch_keys(ints, n, K, K, c.seed, h->bs_keys2[l & 1].as<uint64_t>(), h->bs_iota2[l & 1].as<uint32_t>(),
                             h->stream));
    return HS_OK;
  }
  const uint32_t nb = host2[0];
  *nb_out = nb;
  *grouped = true;
  HS_CHECK(reserve_directory(h, l, nb));
  HS_HIP(h, h->bs_dk.reserve((size_t)nb * 16 + 64));   // distinct keys (8) + their slots (4) + slots sorted (4)
  uint64_t* dk = h->bs_dk.as<uint64_t>();
  uint32_t* ds = reinterpret_cast<uint32_t*>(dk + nb);
  uint32_t* ds_sorted = ds + nb;
  uint32_t* ids = h->t_ids[l].as<uint32_t>();
  uint32_t* dir_start = h->t_dirstart[l].as<uint32_t>();
  int32_t* dir_tuple = h->t_dirtuple[l].as<int32_t>();
  HS_HIP(h, hs_launch_fp_compact(h->bs_fptab.as<uint64_t>(), C, blk_off, dk, ds, h->stream));
  HS_HIP(h, hs_sort_pairs_u64_u32(sort_temp.p, sort_temp.cap, dk, h->t_dirkey[l].as<uint64_t>(), ds, ds_sorted, nb, 0, 64,
                                  h->stream));
  // (the table's slots are free now: they take the rank of every slot's key)
  uint32_t* rank_of_slot = h->bs_fptab.as<uint32_t>();
  HS_HIP(h, hs_launch_rank_slots(ds_sorted, nb, rank_of_slot, h->stream));
  HS_HIP(h, hs_launch_rank_kmers(rank, n, rank_of_slot, h->stream));
  // stable LSD radix sort of (rank, id) on the bits the ranks have; the last pass writes the table's ids
  const int bits = std::max(1, bit_width_u32(nb ? nb - 1 : 0));
  const int n_pass = (bits + 7) / 8;
  uint32_t* kbuf[2] = {h->bs_keys_sorted.as<uint32_t>(), h->bs_keys_sorted.as<uint32_t>() + n};
  uint32_t* ibuf[2] = {ids, h->bs_rle_counts.as<uint32_t>()};   // pass p writes ibuf[(n_pass - 1 - p) & 1]
  uint32_t* hist = h->bs_hist.as<uint32_t>();
  uint32_t* hist_scanned = hist + ((size_t)256 * n_tiles + 64);
  const uint32_t* kin = rank;
  const uint32_t* iin = nullptr;
  for (int p = 0; p < n_pass; ++p) {
    uint32_t* kout = kbuf[p & 1];
    uint32_t* iout = ibuf[(n_pass - 1 - p) & 1];
    HS_HIP(h, hs_launch_rs_hist(kin, (uint32_t)n, 8 * p, hist, h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(sort_temp.p, sort_temp.cap, hist, hist_scanned, (size_t)256 * n_tiles, h->stream));
    HS_HIP(h, hs_launch_rs_scatter(kin, iin, (uint32_t)n, 8 * p, hist_scanned, kout, iout, h->stream));
    kin = kout;
    iin = iout;
  }
  HS_HIP(h, hs_launch_dir_start(kin, (uint32_t)n, nb, dir_start, d_small + 2, h->stream));
  HS_HIP(h, hs_launch_dir_tuples(dir_start, ids, ints, nb, K, dir_tuple, h->stream));
  // the exact-membership proof of every k-mer against its bucket's tuple (flag 1, read with the largest bucket)
  HS_HIP(h, hs_launch_group_check(ints, n, K, rank, dir_tuple, d_small + 1, h->stream));
  return HS_OK;
}

// Table l grouped by a sort of its fingerprints (keys and ids 0 .. n - 1 ready in buffer l & 1): ids, directory and
// largest bucket (bs_small[2]) on the stream, *nb on return -- or *collided: one fingerprint, two HashKey strings,
// and nothing more is done for the table.
hs_status group_by_sort(BuildCtx& c, int l, uint32_t* nb_out, bool* collided) {
  hs_handle* h = c.h;
  const uint64_t n = h->n;
  const int K = (int)h->p.K;
  const int32_t* ints = h->bs_ints2[l & 1].as<int32_t>();
  uint64_t* keys_sorted = h->bs_keys_sorted.as<uint64_t>();
  uint32_t* ids = h->t_ids[l].as<uint32_t>();
  uint32_t* d_small = h->bs_small.as<uint32_t>();
  DevBuf &sort_temp = h->bs_sort_temp, &slow_q = h->bs_slow_q;
  uint32_t nb = 0, flag = 0;
  // The radix sort looks at the fingerprints' top 48 bits only (6 passes instead of 8): buckets are
  // far fewer than 2^24, so two DISTINCT fingerprints rarely agree there (~ nb^2 / 2^49 per table);
  // hs_check_runs_kernel sees it if they do (flag 4) and the table is sorted again on all 64 bits.
  // Only where rocPRIM's onesweep passes do the sorting (hs_sort_partial_bits_ok: n above the library's
  // merge_sort_limit, 2^20): up to that size its merge sort takes over, whose cost does not depend on
  // the bits and whose comparator for a range ending at bit 64 is built from 1 << 64 (hs_prims.hip) --
  // the memory fault of this sort's first draft.  (HS_SORT_FROM_BIT: 0 = every bit at once; the tests
  // pass 56 to see the second sort happen.)
  const int from_bit0 = hs_sort_partial_bits_ok((size_t)n) ? h->knobs.sort_from_bit : 0;
  for (int from_bit = from_bit0; n; from_bit = 0) {
    HS_HIP(h, hs_sort_pairs_u64_u32(sort_temp.p, sort_temp.cap, h->bs_keys2[l & 1].as<uint64_t>(), keys_sorted,
                                    h->bs_iota2[l & 1].as<uint32_t>(), ids, n, from_bit, 64, h->stream));
    const uint32_t slow_cap = 1u << 16;
    HS_HIP(h, slow_q.reserve(((size_t)slow_cap + 1) * 4));
    HS_HIP(h, hs_launch_check_runs(keys_sorted, ids, ints, n, K, d_small + 1, slow_q.as<uint32_t>(), slow_cap, false,
                                   from_bit, h->stream));
    HS_HIP(h, hs_rle_u64(sort_temp.p, sort_temp.cap, keys_sorted, h->bs_rle_unique.as<uint64_t>(),
                         h->bs_rle_counts.as<uint32_t>(), d_small, n, h->stream));
    uint32_t host_small[3];
    HS_HIP(h, hipMemcpyAsync(host_small, d_small, 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    nb = host_small[0];
    flag = host_small[1];
    if ((flag & 4u) && from_bit) {  // interleaved fingerprints: once more, on every bit
      if (h->knobs.build_debug) fprintf(stderr, "table %d: %u buckets, second sort on all bits\n", l, nb);
      HS_HIP(h, hipMemsetAsync(d_small, 0, 64, h->stream));
      continue;
    }
    if (flag & 2u) {  // very many aliased neighbours (tiny W): compare every pair as strings
      HS_HIP(h, hipMemsetAsync(d_small + 1, 0, 4, h->stream));
      HS_HIP(h, hs_launch_check_runs(keys_sorted, ids, ints, n, K, d_small + 1, slow_q.as<uint32_t>(), slow_cap, true, 0,
                                     h->stream));
      HS_HIP(h, hipMemcpyAsync(&flag, d_small + 1, 4, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipStreamSynchronize(h->stream));
    }
    break;
  }
  *nb_out = nb;
  *collided = (flag & 1u) != 0;
  if (*collided) return HS_OK;
  HS_CHECK(directory_from_runs(h, l, nb, n));
  HS_HIP(h, hs_launch_dir_tuples(h->t_dirstart[l].as<uint32_t>(), ids, ints, nb, K, h->t_dirtuple[l].as<int32_t>(),
                                 h->stream));
  return HS_OK;
}

// Table l is grouped: its hash buffers go back to the side stream, its rows are gathered, and the tail of its
// counters is read -- for a table grouped by rank that is where a collision shows (*collided: one fingerprint, two
// HashKey strings; the caller tries the next seed).  Then the timers, the hash statistics and the table itself.
hs_status finish_table(BuildCtx& c, int l, uint32_t nb, bool grouped, bool* collided) {
  hs_handle* h = c.h;
  const uint64_t n = h->n;
  const int L = (int)h->p.L, u = l & 1;
  HS_HIP(h, hipEventRecord(c.ev_free[u], h->stream));  // ints / keys / iota of this table are free
  HS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  HS_CHECK(gather_table_rows(h, l, n, true));
  HS_HIP(h, hipEventRecord(h->ev[3], h->stream));
  uint32_t tail2[2] = {0, 0};  // {collision flag, largest bucket}
  HS_HIP(h, hipMemcpyAsync(tail2, h->bs_small.as<uint32_t>() + 1, 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  *collided = grouped && (tail2[0] & 1u);
  if (*collided) return HS_OK;
  if (l + 1 < L && c.serial) HS_CHECK(hash_table(c, l + 1));
  {
    float ms = 0.f;  // the hash ran on the side stream, possibly beside the previous table's sort
    if (hipEventElapsedTime(&ms, c.ev_t[2 * u], c.ev_t[2 * u + 1]) == hipSuccess) c.ms_hash += ms;
  }
  c.ms_sort += ev_ms(h, 1, 2);
  c.ms_gather += ev_ms(h, 2, 3);
  HS_CHECK(hash_account(h, n, (int)h->p.K, u));  // table l's hash has completed (its sort waited for it)
  publish_table(h, l, n, nb);
  h->info.max_bucket[l] = tail2[1];
  return HS_OK;
}

// The L tables of the n k-mers in h->codes / h->packed_all under one seed.  *collided: nothing of the index stands;
// the caller tries the next seed.
hs_status build_tables(hs_handle* h, uint32_t seed, bool* collided) {
  const uint64_t n = h->n;
  const int L = (int)h->p.L;
  *collided = false;
  BuildCtx c = {h, seed, h->stream2, !h->knobs.build_sort && n < (1ull << 31), h->knobs.build_serial};
  HS_CHECK(reserve_build_buffers(h));
  for (int i = 0; i < 2; ++i) {
    HS_HIP(h, hipEventCreateWithFlags(&c.ev_hashed[i], hipEventDisableTiming));
    HS_HIP(h, hipEventCreateWithFlags(&c.ev_free[i], hipEventDisableTiming));
  }
  for (int i = 0; i < 4; ++i) HS_HIP(h, hipEventCreate(&c.ev_t[i]));
  // the side stream starts after everything queued so far (codes, packing, planes)
  HS_HIP(h, hipEventRecord(h->evx[EV_FORK], h->stream));
  HS_HIP(h, hipStreamWaitEvent(c.hash_stream, h->evx[EV_FORK], 0));
  HS_CHECK(hash_table(c, 0));
  for (int l = 0; l < L; ++l) {
    HS_HIP(h, hipMemsetAsync(h->bs_small.p, 0, 64, h->stream));
    if (l + 1 < L && !c.serial) HS_CHECK(hash_table(c, l + 1));  // runs beside this table's grouping
    HS_HIP(h, hipStreamWaitEvent(h->stream, c.ev_hashed[l & 1], 0));
    HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
    uint32_t nb = 0;
    bool grouped = false;  // group_by_rank produced this table's ids and directory
    if (c.group_by_rank && n) HS_CHECK(group_by_rank(c, l, &nb, &grouped));
    if (!grouped) HS_CHECK(group_by_sort(c, l, &nb, collided));
    if (*collided) return HS_OK;
    HS_CHECK(finish_table(c, l, nb, grouped, collided));
    if (*collided) return HS_OK;
  }
  h->prof.ms_hash = c.ms_hash;
  h->prof.ms_sort = c.ms_sort;
  h->prof.ms_gather = c.ms_gather;
  return HS_OK;
}

}  // namespace

extern "C" {

// Common end of hs_index_build* and hs_index_load: info, global bucket numbering, byte count.
static hs_status finish_index(hs_handle* h) {
  h->info.n = h->n;
  h->info.key_seed = h->key_seed;
  {  // global bucket numbering over the tables (grouping of probes by bucket at query time)
    uint32_t base[HS_MAX_L + 1];
    uint64_t acc = 0;
    for (uint32_t l = 0; l < h->p.L; ++l) {
      base[l] = (uint32_t)acc;
      acc += h->info.n_buckets[l];
    }
    if (acc >= 0xfffffff0ull) return fail(h, HS_ERR_INVALID, "too many buckets");
    base[h->p.L] = (uint32_t)acc;
    h->nb_total = (uint32_t)acc;
    HS_HIP(h, h->dir_base.reserve((HS_MAX_L + 1) * 4));
    HS_HIP(h, hipMemcpyAsync(h->dir_base.p, base, ((size_t)h->p.L + 1) * 4, hipMemcpyHostToDevice, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));  // (base[] is a local)
  }
  // jump tables of the directories: the top J bits of a fingerprint (2^J >= number of buckets); one
  // allocation for all tables (an allocation costs ~ 0.5 ms, whatever its size)
  size_t jump_words = 0, jump_at[HS_MAX_L];
  for (uint32_t l = 0; l < h->p.L; ++l) {
    const uint32_t J = (uint32_t)std::max(1, bit_width_u32((uint32_t)h->info.n_buckets[l]));
    jump_at[l] = jump_words;
    jump_words += ((size_t)1 << J) + 2;
  }
  HS_HIP(h, h->t_dirjump.reserve(jump_words * 4));
  for (uint32_t l = 0; l < h->p.L; ++l) {
    const uint32_t nb = (uint32_t)h->info.n_buckets[l];
    const uint32_t J = (uint32_t)std::max(1, bit_width_u32(nb));
    const uint32_t n_slots = 1u << J;
    uint32_t* const jump = h->t_dirjump.as<uint32_t>() + jump_at[l];
    HS_HIP(h, hs_launch_dir_jump(h->t_dirkey[l].as<uint64_t>(), nb, 64 - J, n_slots, jump, h->stream));
    h->tabs.t[l].dir_jump = jump;
    h->tabs.t[l].jump_shift = 64 - J;
  }
  // the giant buckets of every table (bucket partition: shared among the parts by query, hs_probe_part)
  {
    constexpr uint32_t GCAP = 1024;  // per table: buckets of > n / 1024 members number < 1024
    HS_HIP(h, h->t_giant.reserve((size_t)HS_MAX_L * GCAP * 8));
    HS_HIP(h, h->counters.reserve(256));
    uint32_t* const d_ng = h->counters.as<uint32_t>() + 32;
    HS_HIP(h, hipMemsetAsync(d_ng, 0, HS_MAX_L * 4, h->stream));
    const uint32_t thr = hs_giant_threshold(h->n);
    for (uint32_t l = 0; l < h->p.L; ++l)
      HS_HIP(h, hs_launch_giant_buckets(h->t_dirtuple[l].as<int32_t>(), (int)h->p.K, h->t_dirstart[l].as<uint32_t>(),
                                        (uint32_t)h->info.n_buckets[l], thr, h->t_giant.as<uint64_t>() + (size_t)l * GCAP,
                                        GCAP, d_ng + l, h->stream));
    uint32_t ng[HS_MAX_L];
    std::vector<uint64_t> keys((size_t)HS_MAX_L * GCAP);
    HS_HIP(h, hipMemcpyAsync(ng, d_ng, HS_MAX_L * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(keys.data(), h->t_giant.p, keys.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    for (uint32_t l = 0; l < h->p.L; ++l) {
      if (ng[l] > GCAP) return fail(h, HS_ERR_STATE, "more giant buckets in a table than its list holds");
      std::sort(keys.begin() + (size_t)l * GCAP, keys.begin() + (size_t)l * GCAP + ng[l]);
      h->tabs.t[l].giant_key = h->t_giant.as<uint64_t>() + (size_t)l * GCAP;
      h->tabs.t[l].n_giant = ng[l];
    }
    HS_HIP(h, hipMemcpyAsync(h->t_giant.p, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));  // (keys is a local)
  }
  // directory records (hs_dir_records_kernel): one 64-byte line per bucket for the probe, where the tuples fit
  for (uint32_t l = 0; l < h->p.L; ++l) h->tabs.t[l].dir_rec = nullptr;
  if (h->p.K <= HS_REC_MAX_K && h->nb_total) {
    HS_HIP(h, h->t_dirrec.reserve((size_t)h->nb_total * 64));
    HS_HIP(h, h->counters.reserve(256));
    uint32_t* const d_wide = h->counters.as<uint32_t>() + 32;  // one flag per table (L <= 32)
    HS_HIP(h, hipMemsetAsync(d_wide, 0, HS_MAX_L * 4, h->stream));
    uint64_t at = 0;
    for (uint32_t l = 0; l < h->p.L; ++l) {
      const uint32_t nb = (uint32_t)h->info.n_buckets[l];
      uint4* const rec = h->t_dirrec.as<uint4>() + 4 * at;
      HS_HIP(h, hs_launch_dir_records(h->t_dirkey[l].as<uint64_t>(), h->t_dirstart[l].as<uint32_t>(),
                                      h->t_dirtuple[l].as<int32_t>(), nb, (int)h->p.K, rec, d_wide + l, h->stream));
      h->tabs.t[l].dir_rec = rec;
      at += nb;
    }
    uint32_t wide[HS_MAX_L];
    HS_HIP(h, hipMemcpyAsync(wide, d_wide, HS_MAX_L * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    for (uint32_t l = 0; l < h->p.L; ++l)
      if (wide[l]) h->tabs.t[l].dir_rec = nullptr;  // a bucket int outside 16 bits: this table keeps the arrays
  }
  HS_HIP(h, hipStreamSynchronize(h->stream));
  uint64_t bytes = h->codes.cap + h->packed_all.cap + h->t_packed.cap + h->t_rec8.cap + h->t_rec8w.cap + h->t_rec6.cap + h->t_rho.cap +
                   h->t_pos.cap + h->t_dirrec.cap;
  for (uint32_t l = 0; l < h->p.L; ++l)
    bytes += h->t_dirkey[l].cap + h->t_dirstart[l].cap + h->t_dirtuple[l].cap + h->t_ids[l].cap;
  bytes += h->t_dirjump.cap;
  h->info.device_bytes = bytes;
  h->built = true;
  return HS_OK;
}

// the tables of a new or changed index stand: the clock begin_index (or the call itself) started stops, then finish_index
static hs_status end_index(hs_handle* h) {
  HS_HIP(h, hipEventRecord(h->ev[9], h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->prof.ms_total = ev_ms(h, 8, 9);
  return finish_index(h);
}

// Index build over the n x k residue codes already in h->codes (device): validation + packing,
// the L tables, the global bucket numbering.
static hs_status index_build_resident(hs_handle* h, uint64_t n) {
  hs_status st = HS_OK;
  HS_HIP(h, h->packed_all.reserve(std::max<size_t>(16, (size_t)n * h->PW * 16)));
  if (n)  // (the build's buffers are reserved beside the copy of the codes and the packing kernel)
    HS_CHECK(pack_checked(h, h->codes.as<uint8_t>(), n, h->packed_all.as<uint4>(), HS_ERR_INVALID,
                          "residue code outside the alphabet in the DB", reserve_build_buffers));
  bool collided = true;
  uint32_t seed = 0;
  for (; seed < 4 && collided; ++seed) {
    st = build_tables(h, seed, &collided);
    if (st) return st;
    if (!collided) break;
  }
  if (collided) return fail(h, HS_ERR_KEY_COLLISION, "key fingerprints collided for 4 seeds");
  h->key_seed = seed;
  return end_index(h);
}

hs_status hs_index_build(hs_handle* h, const uint8_t* codes, uint64_t n) {
  if (!h || (n && !codes)) return HS_ERR_INVALID;
  if (n >= (1ull << 31)) return fail(h, HS_ERR_INVALID, "n must be < 2^31 (ids are 32-bit, as in the reference)");
  hs_status st = ensure_device(h);
  if (st) return st;
  HS_CHECK(begin_index(h, n));
  if (n) HS_HIP(h, hipMemcpyAsync(h->codes.p, codes, (size_t)n * h->p.k, hipMemcpyHostToDevice, h->stream));
  return index_build_resident(h, n);
}

// ---- index build with the hashing spread over ranks ("Index build" row) --------------
// The index is replicated, so every rank holds all n k-mers; what is spread is the evaluation of the
// L x K hash functions (the matrix-core part of the build): rank r does it for its contiguous block of
// the k-mers (hs_shard_bounds' rule) and the ranks exchange 8-byte fingerprints instead.  Per table:
//   hs_index_shard_hash_dev    bucket ints + fingerprints of the rank's block
//   <all-gather of the fingerprints, blocks in rank order = id order>
//   hs_index_shard_group_dev   every rank groups all n fingerprints (sort, directory)
//   hs_index_shard_tuples_dev  the bucket ints of the buckets whose FIRST member the rank hashed
//   <sum over ranks: every bucket's tuple>
//   hs_index_shard_finish_dev  exact-membership proof of the rank's own k-mers against the tuples, the
//                              bucket-ordered copies; *collided = one fingerprint, two HashKey strings
//   <max over ranks of collided: if set, every rank starts over with seed + 1>
// then hs_index_shard_end.  The index is the one hs_index_build builds, bit for bit.
// The sharded build's scratch (sorted fingerprints, run lengths, ids, sort space, the block's bucket ints:
// ~ 40 bytes per k-mer) stays with the handle for the next build while it is small beside the device's
// memory and is given back otherwise: release_if_large (4-5 GB beside a 157 GB index at 10^8 k-mers).
static void release_large_shard_scratch(hs_handle* h) {
  release_if_large({&h->bs_keys_sorted, &h->bs_rle_unique, &h->bs_rle_counts, &h->bs_iota2[0], &h->bs_sort_temp,
                    &h->bs_ints2[0]});
}

hs_status hs_index_shard_begin(hs_handle* h, const uint8_t* codes, uint64_t n, uint32_t rank, uint32_t world,
                               uint64_t* block_lo, uint64_t* block_count) {
  if (!h || (n && !codes) || !world || rank >= world) return HS_ERR_INVALID;
  if (n >= (1ull << 31)) return fail(h, HS_ERR_INVALID, "n must be < 2^31 (ids are 32-bit, as in the reference)");
  hs_status st = ensure_device(h);
  if (st) return st;
  if (h->shard_open) {  // a sharded build that never reached hs_index_shard_end (a collision on every seed)
    HS_HIP(h, hipStreamSynchronize(h->stream));
    release_large_shard_scratch(h);
    h->shard_open = false;
  }
  HS_CHECK(begin_index(h, n));
  const int K = (int)h->p.K;
  if (n) HS_HIP(h, hipMemcpyAsync(h->codes.p, codes, (size_t)n * h->p.k, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, h->packed_all.reserve(std::max<size_t>(16, (size_t)n * h->PW * 16)));
  if (n)
    HS_CHECK(pack_checked(h, h->codes.as<uint8_t>(), n, h->packed_all.as<uint4>(), HS_ERR_INVALID,
                          "residue code outside the alphabet in the DB"));
  const uint64_t base = n / world, rem = n % world;   // = hs_shard_bounds (hsearch_dist.h)
  const uint64_t lo = (uint64_t)rank * base + std::min<uint64_t>(rank, rem), cnt = base + (rank < rem ? 1 : 0);
  h->shard_lo = (uint32_t)lo;
  h->shard_cnt = (uint32_t)cnt;
  h->shard_open = true;
  h->shard_table = -1;
  if (block_lo) *block_lo = lo;
  if (block_count) *block_count = cnt;
  HS_CHECK(reserve_table_rows(h, h->t_packed, h->t_rec8, h->t_rho, h->t_pos, n));
  HS_HIP(h, h->bs_ints2[0].reserve(std::max<size_t>(16, (size_t)cnt * K * 4)));
  HS_HIP(h, h->bs_iota2[0].reserve(std::max<size_t>(16, (size_t)n * 4)));
  HS_HIP(h, h->bs_keys_sorted.reserve(std::max<size_t>(16, (size_t)n * 8)));
  HS_HIP(h, h->bs_rle_unique.reserve(std::max<size_t>(16, (size_t)n * 8)));
  HS_HIP(h, h->bs_rle_counts.reserve(std::max<size_t>(16, (size_t)n * 4)));
  HS_HIP(h, h->bs_small.reserve(64));
  HS_HIP(h, h->bs_sort_temp.reserve(std::max(std::max(hs_sort_pairs_u64_u32_temp(n), hs_rle_u64_temp(n)),
                                             hs_scan_u32_temp(n + 1)) + 256));
  return HS_OK;
}

hs_status hs_index_shard_hash_dev(hs_handle* h, uint32_t l, uint32_t seed, uint64_t* d_fp_block) {
  if (!h || !h->shard_open || l >= h->p.L || (h->shard_cnt && !d_fp_block)) return HS_ERR_INVALID;
  hs_status st = ensure_device(h);
  if (st) return st;
  const int K = (int)h->p.K;
  h->shard_table = (int)l;
  h->shard_seed = seed;
  if (!h->shard_cnt) return HS_OK;
  HS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  HS_CHECK(hash_dispatch(h, h->codes.as<uint8_t>() + (uint64_t)h->shard_lo * h->p.k, nullptr, h->shard_cnt, (int)l,
                         h->bs_ints2[0].as<int32_t>(), K, 0, h->stream));
  HS_HIP(h, hs_launch_keys(h->bs_ints2[0].as<int32_t>(), h->shard_cnt, K, K, seed, d_fp_block, nullptr, h->stream));
  HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->prof.ms_hash += ev_ms(h, 0, 1);
  return hash_account(h, h->shard_cnt, K, 0);
}

hs_status hs_index_shard_group_dev(hs_handle* h, uint32_t l, const uint64_t* d_fp_all, uint32_t* n_buckets) {
  if (!h || !h->shard_open || (int)l != h->shard_table || !n_buckets || (h->n && !d_fp_all)) return HS_ERR_INVALID;
  hs_status st = ensure_device(h);
  if (st) return st;
  const uint64_t n = h->n;
  *n_buckets = 0;
  uint32_t* d_small = h->bs_small.as<uint32_t>();
  HS_HIP(h, h->t_ids[l].reserve(std::max<size_t>(16, (size_t)n * 4)));
  HS_HIP(h, hipMemsetAsync(d_small, 0, 64, h->stream));
  uint32_t nb = 0;
  if (n) {
    HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
    HS_HIP(h, hs_launch_iota_u32(h->bs_iota2[0].as<uint32_t>(), (uint32_t)n, h->stream));
    HS_HIP(h, hs_sort_pairs_u64_u32(h->bs_sort_temp.p, h->bs_sort_temp.cap, d_fp_all, h->bs_keys_sorted.as<uint64_t>(),
                                    h->bs_iota2[0].as<uint32_t>(), h->t_ids[l].as<uint32_t>(), n, 0, 64, h->stream));
    HS_HIP(h, hs_rle_u64(h->bs_sort_temp.p, h->bs_sort_temp.cap, h->bs_keys_sorted.as<uint64_t>(),
                         h->bs_rle_unique.as<uint64_t>(), h->bs_rle_counts.as<uint32_t>(), d_small, n, h->stream));
    HS_HIP(h, hipMemcpyAsync(&nb, d_small, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  HS_CHECK(directory_from_runs(h, (int)l, nb, n));
  HS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  uint32_t max_count = 0;
  HS_HIP(h, hipMemcpyAsync(&max_count, d_small + 2, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (n) h->prof.ms_sort += ev_ms(h, 1, 2);
  h->shard_nb = nb;
  h->info.n_buckets[l] = nb;
  h->info.max_bucket[l] = max_count;
  *n_buckets = nb;
  return HS_OK;
}

hs_status hs_index_shard_tuples_dev(hs_handle* h, uint32_t l, int32_t* d_tuples) {
  if (!h || !h->shard_open || (int)l != h->shard_table || (h->shard_nb && !d_tuples)) return HS_ERR_INVALID;
  hs_status st = ensure_device(h);
  if (st) return st;
  HS_HIP(h, hs_launch_shard_first_tuples(h->t_dirstart[l].as<uint32_t>(), h->t_ids[l].as<uint32_t>(),
                                         h->bs_ints2[0].as<int32_t>(), h->shard_lo, h->shard_cnt, h->shard_nb,
                                         (int)h->p.K, d_tuples, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

hs_status hs_index_shard_finish_dev(hs_handle* h, uint32_t l, const int32_t* d_tuples_all, uint32_t* collided) {
  if (!h || !h->shard_open || (int)l != h->shard_table || !collided || (h->shard_nb && !d_tuples_all))
    return HS_ERR_INVALID;
  hs_status st = ensure_device(h);
  if (st) return st;
  const uint64_t n = h->n;
  const int K = (int)h->p.K;
  const uint32_t nb = h->shard_nb;
  uint32_t* d_small = h->bs_small.as<uint32_t>();
  uint32_t* const pos_of = table_slice(h, (int)l, n).pos;
  *collided = 0;
  if (nb) HS_HIP(h, hipMemcpyAsync(h->t_dirtuple[l].p, d_tuples_all, (size_t)nb * K * 4, hipMemcpyDeviceToDevice, h->stream));
  HS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  if (n) {
    // (the positions first: the membership proof reads them)
    HS_HIP(h, hs_launch_invert_perm(h->t_ids[l].as<uint32_t>(), (uint32_t)n, pos_of, h->stream));
    HS_HIP(h, hipMemsetAsync(d_small + 1, 0, 4, h->stream));
    HS_HIP(h, hs_launch_shard_check(h->bs_ints2[0].as<int32_t>(), h->shard_lo, h->shard_cnt, K, pos_of,
                                    h->t_dirstart[l].as<uint32_t>(), nb, h->t_dirtuple[l].as<int32_t>(), d_small + 1,
                                    h->stream));
    HS_CHECK(gather_table_rows(h, (int)l, n, false));
  }
  HS_HIP(h, hipEventRecord(h->ev[3], h->stream));
  uint32_t flag = 0;
  HS_HIP(h, hipMemcpyAsync(&flag, d_small + 1, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->prof.ms_gather += ev_ms(h, 2, 3);
  *collided = flag & 1u;
  publish_table(h, (int)l, n, nb);  // (info.max_bucket[l]: hs_index_shard_group_dev)
  h->shard_table = -1;
  return HS_OK;
}

hs_status hs_index_shard_end(hs_handle* h, uint32_t key_seed) {
  if (!h || !h->shard_open) return HS_ERR_INVALID;
  hs_status st = ensure_device(h);
  if (st) return st;
  h->shard_open = false;
  HS_HIP(h, hipStreamSynchronize(h->stream));
  release_large_shard_scratch(h);
  h->key_seed = key_seed;
  return end_index(h);
}

hs_status hs_index_build_subset(hs_handle* h, const uint8_t* codes_all, uint64_t n_all,
                                const uint32_t* subset, uint64_t n_subset) {
  if (!h || (n_all && !codes_all) || (!subset && n_subset != n_all)) return HS_ERR_INVALID;
  if (n_all >= (1ull << 31) || n_subset > n_all)
    return fail(h, HS_ERR_INVALID, "n must be < 2^31 and the subset no larger than the array");
  hs_status st = ensure_device(h);
  if (st) return st;
  if (subset)
    for (uint64_t i = 0; i < n_subset; ++i)
      if (subset[i] >= n_all) return fail(h, HS_ERR_INVALID, "subset index outside the code array");
  const int k = (int)h->p.k;
  HS_CHECK(begin_index(h, n_subset));
  if (h->all_codes_key != codes_all || h->all_codes_n != n_all) {
    h->all_codes_key = nullptr;
    HS_HIP(h, h->all_codes.reserve(std::max<size_t>(16, (size_t)n_all * k)));
    if (n_all) HS_HIP(h, hipMemcpyAsync(h->all_codes.p, codes_all, (size_t)n_all * k, hipMemcpyHostToDevice, h->stream));
    h->all_codes_key = codes_all;
    h->all_codes_n = n_all;
  }
  const uint32_t* d_sub = nullptr;
  if (subset && n_subset) {
    HS_HIP(h, h->subset_ids.reserve((size_t)n_subset * 4));
    HS_HIP(h, hipMemcpyAsync(h->subset_ids.p, subset, (size_t)n_subset * 4, hipMemcpyHostToDevice, h->stream));
    d_sub = h->subset_ids.as<uint32_t>();
  }
  HS_HIP(h, hs_launch_gather_rows(h->all_codes.as<uint8_t>(), d_sub, n_subset, k, h->codes.as<uint8_t>(), h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));  // `subset` is the caller's again
  return index_build_resident(h, n_subset);
}

// DB = every length-k window of every sequence of a concatenated residue buffer (kmer_search.cpp:
// 64-83 enumerates them the same way: sequence-major, ascending offset; windows do not cross
// sequence boundaries, sequences shorter than k contribute none).  The buffer crosses PCIe once
// (n_residues bytes instead of n_windows * k) and the windows are expanded on the device.
hs_status hs_index_build_windows(hs_handle* h, const uint8_t* residues, uint64_t n_residues,
                                 const uint64_t* seq_start, uint64_t n_seq, uint64_t* n_windows,
                                 uint32_t* window_pos) {
  if (!h || !n_windows || (n_seq && !seq_start) || (n_residues && !residues)) return HS_ERR_INVALID;
  *n_windows = 0;
  hs_status st = ensure_device(h);
  if (st) return st;
  const uint64_t k = h->p.k;
  if (n_residues >= (1ull << 32)) return fail(h, HS_ERR_INVALID, "n_residues must be < 2^32");
  // first window number of every sequence
  std::vector<uint32_t> starts((size_t)n_seq + 1), win_off((size_t)n_seq + 1);
  uint64_t n = 0;
  for (uint64_t s = 0; s < n_seq; ++s) {
    if (seq_start[s] > seq_start[s + 1] || seq_start[s + 1] > n_residues)
      return fail(h, HS_ERR_INVALID, "seq_start must be ascending and end at n_residues");
    const uint64_t len = seq_start[s + 1] - seq_start[s];
    starts[s] = (uint32_t)seq_start[s];
    win_off[s] = (uint32_t)n;
    n += len >= k ? len - k + 1 : 0;
    if (n >= (1ull << 31)) return fail(h, HS_ERR_INVALID, "more than 2^31 - 1 windows");
  }
  starts[n_seq] = (uint32_t)(n_seq ? seq_start[n_seq] : 0);
  win_off[n_seq] = (uint32_t)n;
  HS_CHECK(begin_index(h, n));
  if (n) {
    DevBuf d_res, d_starts, d_off, d_pos;
    struct Guard {
      DevBuf* b[4];
      ~Guard() { for (DevBuf* x : b) x->release(); }
    } guard = {{&d_res, &d_starts, &d_off, &d_pos}};
    HS_HIP(h, d_res.reserve((size_t)n_residues));
    HS_HIP(h, d_starts.reserve(((size_t)n_seq + 1) * 4));
    HS_HIP(h, d_off.reserve(((size_t)n_seq + 1) * 4));
    HS_HIP(h, d_pos.reserve((size_t)n * 4));
    HS_HIP(h, hipMemcpyAsync(d_res.p, residues, (size_t)n_residues, hipMemcpyHostToDevice, h->stream));
    HS_HIP(h, hipMemcpyAsync(d_starts.p, starts.data(), ((size_t)n_seq + 1) * 4, hipMemcpyHostToDevice, h->stream));
    HS_HIP(h, hipMemcpyAsync(d_off.p, win_off.data(), ((size_t)n_seq + 1) * 4, hipMemcpyHostToDevice, h->stream));
    HS_HIP(h, hs_launch_windows(d_res.as<uint8_t>(), (uint32_t)n_residues, d_starts.as<uint32_t>(),
                                d_off.as<uint32_t>(), (uint32_t)n_seq, (int)k, h->codes.as<uint8_t>(),
                                d_pos.as<uint32_t>(), h->stream));
    if (window_pos)
      HS_HIP(h, hipMemcpyAsync(window_pos, d_pos.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  *n_windows = n;
  return index_build_resident(h, n);
}

// ---- hs_index_append: a built index grown by a block of k-mers (hs_append.hip) ----------------------------------
namespace {
// the scratch of one append, carved out of one allocation: sized by the block (m) and by the largest directory
struct AppendScratch {
  int32_t *ints, *btuple;
  uint64_t *keys, *keys_sorted, *bkey;
  uint32_t *iota, *bids, *bcount, *bstart, *small, *slow_q, *pos, *is_new, *new_scan, *old_cnt, *map_blk, *base_blk,
      *inc, *inc_scan, *map_old, *base_old, *out_count, *brho;
  uint4 *bpacked, *brec;
  void* sort_temp;
  size_t sort_temp_bytes;
};
const uint32_t kAppendSlowCap = 1u << 16;
size_t carve_append_scratch(AppendScratch& a, char* base, uint64_t m, int K, int PW, uint64_t nb_max) {
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + at : nullptr;
    at += (bytes + 255) & ~(size_t)255;
    return p;
  };
  a.ints = (int32_t*)take(m * K * 4);
  a.btuple = (int32_t*)take(m * K * 4);
  a.keys = (uint64_t*)take(m * 8);
  a.keys_sorted = (uint64_t*)take(m * 8);
  a.bkey = (uint64_t*)take(m * 8);
  a.iota = (uint32_t*)take(m * 4);
  a.bids = (uint32_t*)take(m * 4);
  a.bcount = (uint32_t*)take(m * 4);
  a.bstart = (uint32_t*)take((m + 1) * 4);
  a.small = (uint32_t*)take(64);
  a.slow_q = (uint32_t*)take(((size_t)kAppendSlowCap + 1) * 4);
  a.pos = (uint32_t*)take(m * 4);
  a.is_new = (uint32_t*)take((m + 1) * 4);
  a.new_scan = (uint32_t*)take((m + 1) * 4);
  a.old_cnt = (uint32_t*)take(m * 4);
  a.map_blk = (uint32_t*)take(m * 4);
  a.base_blk = (uint32_t*)take(m * 4);
  a.inc = (uint32_t*)take((nb_max + 1) * 4);
  a.inc_scan = (uint32_t*)take((nb_max + 1) * 4);
  a.map_old = (uint32_t*)take((nb_max + 1) * 4);
  a.base_old = (uint32_t*)take((nb_max + 1) * 4);
  a.out_count = (uint32_t*)take((nb_max + m + 1) * 4);
  a.brho = (uint32_t*)take(m * 4);
  a.bpacked = (uint4*)take(m * PW * 16);
  a.brec = (uint4*)take(m * 16);
  a.sort_temp_bytes = std::max(std::max(hs_sort_pairs_u64_u32_temp(m), hs_rle_u64_temp(m)),
                               hs_scan_u32_temp(nb_max + m + 2)) + 256;
  a.sort_temp = take(a.sort_temp_bytes);
  return at;
}
}  // namespace

// unbuilt index, n + m too large: from the arguments alone, before anything is touched
static hs_status append_check(hs_handle* h, uint64_t m) {
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_append: no index to append to (hs_index_build has not been called)");
  if (m >= (1ull << 31) || h->n + m >= (1ull << 31))
    return fail(h, HS_ERR_INVALID, "hs_index_append: n + m must be < 2^31 (ids are 32-bit, as in the reference)");
  return HS_OK;
}

// The L tables of the index merged with the block, whose codes are the last m of h->codes and whose packed k-mers
// are d_blk_packed [m][PW]; h->n is still the old n.  On success the grown arrays are the handle's and the old ones
// are gone (finish_index is the caller's); *collided: nothing of the handle's tables has changed.
static hs_status append_tables(hs_handle* h, const uint4* d_blk_packed, uint64_t m, bool* collided) {
  const uint64_t n = h->n, n2 = n + m;
  const int K = (int)h->p.K, L = (int)h->p.L, k = (int)h->p.k, PW = h->PW;
  const uint32_t seed = h->key_seed;
  *collided = false;
  const uint8_t* d_blk_codes = h->codes.as<uint8_t>() + (size_t)n * k;
  DevBuf arena;
  BufGuard guard;
  guard.b = {&arena};
  NewTables grown(h);
  uint64_t nb_max = 0;
  for (int l = 0; l < L; ++l) nb_max = std::max<uint64_t>(nb_max, h->info.n_buckets[l]);
  AppendScratch a;
  HS_HIP(h, arena.reserve(carve_append_scratch(a, nullptr, m, K, PW, nb_max)));
  carve_append_scratch(a, arena.as<char>(), m, K, PW, nb_max);
  HS_CHECK(reserve_table_rows(h, grown.packed, grown.rec8, grown.rho, grown.pos, n2));
  uint64_t new_nb[HS_MAX_L], new_max[HS_MAX_L], new_buckets = 0;
  double ms_hash = 0, ms_sort = 0, ms_gather = 0;
  for (int l = 0; l < L; ++l) {
    const uint32_t nb = (uint32_t)h->info.n_buckets[l];
    const hs_table_dev& tb = h->tabs.t[l];
    const RowSlice old = table_slice(h, l, n), dst = grown.slice(h, l, n2);
    HS_HIP(h, hipMemsetAsync(a.small, 0, 64, h->stream));
    HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
    // 1. the block's bucket ints and fingerprints under the index's seed, grouped as the build's sorting path groups
    HS_CHECK(hash_dispatch(h, d_blk_codes, nullptr, m, l, a.ints, K, 0, h->stream));
    HS_HIP(h, hs_launch_keys(a.ints, m, K, K, seed, a.keys, a.iota, h->stream));
    HS_HIP(h, hipEventRecord(h->ev[2], h->stream));
    HS_HIP(h, hs_sort_pairs_u64_u32(a.sort_temp, a.sort_temp_bytes, a.keys, a.keys_sorted, a.iota, a.bids, m, 0, 64,
                                    h->stream));
    HS_HIP(h, hs_launch_check_runs(a.keys_sorted, a.bids, a.ints, m, K, a.small + 1, a.slow_q, kAppendSlowCap, false, 0,
                                   h->stream));
    HS_HIP(h, hs_rle_u64(a.sort_temp, a.sort_temp_bytes, a.keys_sorted, a.bkey, a.bcount, a.small, m, h->stream));
    uint32_t host2[2] = {0, 0};  // {block buckets, flags}
    HS_HIP(h, hipMemcpyAsync(host2, a.small, 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    const uint32_t nbB = host2[0];
    uint32_t flag = host2[1];
    if (flag & 2u) {  // very many aliased neighbours: every pair compared as strings (build_tables does the same)
      HS_HIP(h, hipMemsetAsync(a.small + 1, 0, 4, h->stream));
      HS_HIP(h, hs_launch_check_runs(a.keys_sorted, a.bids, a.ints, m, K, a.small + 1, a.slow_q, kAppendSlowCap, true, 0,
                                     h->stream));
      HS_HIP(h, hipMemcpyAsync(&flag, a.small + 1, 4, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (flag & 1u) {
      *collided = true;
      return HS_OK;
    }
    if (nbB > m || !nbB) return fail(h, HS_ERR_HIP, "hs_index_append: the block's run lengths are inconsistent");
    HS_HIP(h, hs_exclusive_scan_u32(a.sort_temp, a.sort_temp_bytes, a.bcount, a.bstart, nbB, h->stream));
    HS_HIP(h, hs_launch_set_u32(a.bstart + nbB, (uint32_t)m, h->stream));
    HS_HIP(h, hs_launch_dir_tuples(a.bstart, a.bids, a.ints, nbB, K, a.btuple, h->stream));
    // 2. match against the old directory
    HS_HIP(h, hipMemsetAsync(a.inc, 0, ((size_t)nb + 1) * 4, h->stream));
    HS_HIP(h, hipMemsetAsync(a.is_new + nbB, 0, 4, h->stream));
    HS_HIP(h, hipMemsetAsync(a.small + 1, 0, 4, h->stream));
    HS_HIP(h, hs_launch_append_match(a.bkey, a.btuple, nbB, K, tb.dir_key, tb.dir_tuple, tb.dir_jump, tb.jump_shift, nb,
                                     a.pos, a.is_new, a.inc, a.small + 1, h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(a.sort_temp, a.sort_temp_bytes, a.is_new, a.new_scan, (size_t)nbB + 1, h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(a.sort_temp, a.sort_temp_bytes, a.inc, a.inc_scan, (size_t)nb + 1, h->stream));
    uint32_t n_new = 0;
    HS_HIP(h, hipMemcpyAsync(&flag, a.small + 1, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(&n_new, a.new_scan + nbB, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
#ifdef HS_TEST_HOOKS
    if (h->knobs.test_append_collision && l == L - 1) flag |= 1u;  // (the last table: the others have merged by then)
#endif
    if (flag & 1u) {  // one fingerprint, two HashKey strings, the block's and the index's
      *collided = true;
      return HS_OK;
    }
    if (n_new > nbB) return fail(h, HS_ERR_HIP, "hs_index_append: the match counts are inconsistent");
    // 3. the merged directory
    const uint32_t nb2 = nb + n_new;
    HS_HIP(h, grown.ids[l].reserve(std::max<size_t>(16, (size_t)n2 * 4)));
    HS_CHECK(reserve_directory(h, grown.key[l], grown.start[l], grown.tuple[l], nb2));
    uint32_t* const dst_ids = grown.ids[l].as<uint32_t>();
    uint32_t* const dst_start = grown.start[l].as<uint32_t>();
    HS_HIP(h, hs_launch_append_dir(tb.dir_key, tb.dir_start, tb.dir_tuple, nb, a.bkey, a.bstart, a.btuple, nbB, K, a.pos,
                                   a.is_new, a.new_scan, a.inc, a.inc_scan, a.map_old, a.map_blk, a.old_cnt,
                                   grown.key[l].as<uint64_t>(), grown.tuple[l].as<int32_t>(), a.out_count, h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(a.sort_temp, a.sort_temp_bytes, a.out_count, dst_start, nb2, h->stream));
    HS_HIP(h, hs_launch_set_u32(dst_start + nb2, (uint32_t)n2, h->stream));
    HS_HIP(h, hipMemsetAsync(a.small + 2, 0, 4, h->stream));
    HS_HIP(h, hs_launch_max_u32(a.out_count, nb2, a.small + 2, h->stream));
    HS_HIP(h, hs_launch_append_bases(dst_start, tb.dir_start, a.map_old, nb, a.bstart, a.map_blk, a.old_cnt, nbB,
                                     a.base_old, a.base_blk, h->stream));
    HS_HIP(h, hipEventRecord(h->ev[3], h->stream));
    // 4. the block's entries in block-bucket order, by the build's own record kernels; then the move
    uint4* const blk_rec = dst.rec8 ? a.brec : nullptr;
    uint32_t* const blk_rho = dst.rho ? a.brho : nullptr;
    HS_CHECK(gather_rows(h, d_blk_packed, a.bids, m, a.bpacked, blk_rec, blk_rho));
    HS_HIP(h, hs_launch_append_move((uint32_t)n, tb.dir_start, nb, a.base_old, (uint32_t)n2, PW, tb.ids, 0u, tb.packed,
                                    old.rec8, old.rho, dst_ids, dst.packed, dst.rec8, dst.rho, h->stream));
    HS_HIP(h, hs_launch_append_move((uint32_t)m, a.bstart, nbB, a.base_blk, (uint32_t)n2, PW, a.bids, (uint32_t)n,
                                    a.bpacked, blk_rec, blk_rho, dst_ids, dst.packed, dst.rec8, dst.rho, h->stream));
    HS_HIP(h, hs_launch_invert_perm(dst_ids, (uint32_t)n2, dst.pos, h->stream));
    HS_HIP(h, hipEventRecord(h->ev[4], h->stream));
    uint32_t max_count = 0;
    HS_HIP(h, hipMemcpyAsync(&max_count, a.small + 2, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    ms_hash += ev_ms(h, 1, 2);
    ms_sort += ev_ms(h, 2, 3);
    ms_gather += ev_ms(h, 3, 4);
    HS_CHECK(hash_account(h, m, K, 0));
    new_nb[l] = nb2;
    new_max[l] = max_count;
    new_buckets += n_new;
  }
  // every table has merged: the grown arrays become the handle's (and the old ones go with `grown`)
  adopt_tables(h, n2, grown, new_nb, new_max);
  h->prof.ms_hash = ms_hash;
  h->prof.ms_sort = ms_sort;
  h->prof.ms_gather = ms_gather;
  h->prof.append_new_buckets = new_buckets;
  return HS_OK;
}

// The block's codes are d_blk [m][k] on the device (m >= 1, append_check passed).  Validation first; from
// drop_index on, every failure leaves the handle without an index.
static hs_status index_append_resident(hs_handle* h, const uint8_t* d_blk, uint64_t m) {
  const uint64_t n = h->n;
  const int k = (int)h->p.k, PW = h->PW;
  // HS_BUILD_DEBUG: host time of the call's stages on stderr (allocation and release are host work no event sees)
  auto t_last = std::chrono::steady_clock::now();
  auto stage = [&](const char* what) {
    if (!h->knobs.build_debug) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "hs_index_append: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
    t_last = t;
  };
  DevBuf blk_packed, ncodes, npacked_all;
  BufGuard guard;
  guard.b = {&blk_packed, &ncodes, &npacked_all};
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, blk_packed.reserve((size_t)m * PW * 16));
  HS_CHECK(pack_checked(h, d_blk, m, blk_packed.as<uint4>(), HS_ERR_INVALID,
                        "hs_index_append: residue code outside the alphabet in the block"));
  stage("block packed and checked");
  // ---- the handle changes from here on
  drop_index(h);
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  // codes and packed k-mers in id order: old ones copied on the device, the block behind them
  HS_HIP(h, ncodes.reserve(std::max<size_t>(16, (size_t)(n + m) * k)));
  HS_HIP(h, npacked_all.reserve(std::max<size_t>(16, (size_t)(n + m) * PW * 16)));
  if (n) {
    HS_HIP(h, hipMemcpyAsync(ncodes.p, h->codes.p, (size_t)n * k, hipMemcpyDeviceToDevice, h->stream));
    HS_HIP(h, hipMemcpyAsync(npacked_all.p, h->packed_all.p, (size_t)n * PW * 16, hipMemcpyDeviceToDevice, h->stream));
  }
  HS_HIP(h, hipMemcpyAsync(ncodes.as<char>() + (size_t)n * k, d_blk, (size_t)m * k, hipMemcpyDeviceToDevice, h->stream));
  HS_HIP(h, hipMemcpyAsync(npacked_all.as<char>() + (size_t)n * PW * 16, blk_packed.p, (size_t)m * PW * 16,
                           hipMemcpyDeviceToDevice, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));  // (d_blk may be the caller's)
  std::swap(h->codes, ncodes);
  std::swap(h->packed_all, npacked_all);
  ncodes.release();
  npacked_all.release();
  stage("codes grown");
  bool collided = false;
  if (n) {
    HS_CHECK(append_tables(h, blk_packed.as<uint4>(), m, &collided));
    stage("tables merged, old ones freed");
    if (!collided) {
      h->n = n + m;
      const hs_status fst = end_index(h);
      stage("finish_index");
      return fst;
    }
  }
  // an empty index, or one fingerprint under two HashKey strings: the build loop over all the codes, resident
  // already, from seed 0 -- where hs_index_build over the concatenation would have ended too
  blk_packed.release();
  h->n = n + m;
  memset(&h->info, 0, sizeof(h->info));
  const uint64_t rebuilds = collided ? 1 : 0;
  hs_status st = index_build_resident(h, n + m);
  h->prof.append_rebuilds = rebuilds;
  return st;
}

hs_status hs_index_append_dev(hs_handle* h, const uint8_t* d_codes, uint64_t m) {
  if (!h || (m && !d_codes)) return HS_ERR_INVALID;
  HS_CHECK(append_check(h, m));
  if (!m) return HS_OK;
  HS_CHECK(ensure_device(h));
  return index_append_resident(h, d_codes, m);
}

hs_status hs_index_append(hs_handle* h, const uint8_t* codes, uint64_t m) {
  if (!h || (m && !codes)) return HS_ERR_INVALID;
  HS_CHECK(append_check(h, m));
  if (!m) return HS_OK;
  HS_CHECK(ensure_device(h));
  DevBuf d_blk;
  BufGuard guard;
  guard.b = {&d_blk};
  HS_HIP(h, d_blk.reserve((size_t)m * h->p.k));
  HS_HIP(h, hipMemcpyAsync(d_blk.p, codes, (size_t)m * h->p.k, hipMemcpyHostToDevice, h->stream));
  return index_append_resident(h, d_blk.as<uint8_t>(), m);
}

hs_status hs_index_append_windows(hs_handle* h, const uint8_t* residues, uint64_t n_residues,
                                  const uint64_t* seq_start, uint64_t n_seq, uint64_t* n_windows,
                                  uint32_t* window_pos) {
  if (!h || !n_windows || (n_seq && !seq_start) || (n_residues && !residues)) return HS_ERR_INVALID;
  *n_windows = 0;
  if (!h->built) return append_check(h, 0);
  const uint64_t k = h->p.k;
  if (n_residues >= (1ull << 32)) return fail(h, HS_ERR_INVALID, "n_residues must be < 2^32");
  std::vector<uint32_t> starts((size_t)n_seq + 1), win_off((size_t)n_seq + 1);
  uint64_t m = 0;
  for (uint64_t s = 0; s < n_seq; ++s) {
    if (seq_start[s] > seq_start[s + 1] || seq_start[s + 1] > n_residues)
      return fail(h, HS_ERR_INVALID, "seq_start must be ascending and end at n_residues");
    const uint64_t len = seq_start[s + 1] - seq_start[s];
    starts[s] = (uint32_t)seq_start[s];
    win_off[s] = (uint32_t)m;
    m += len >= k ? len - k + 1 : 0;
    if (m >= (1ull << 31)) return fail(h, HS_ERR_INVALID, "more than 2^31 - 1 windows");
  }
  starts[n_seq] = (uint32_t)(n_seq ? seq_start[n_seq] : 0);
  win_off[n_seq] = (uint32_t)m;
  HS_CHECK(append_check(h, m));
  if (!m) return HS_OK;
  HS_CHECK(ensure_device(h));
  DevBuf d_res, d_starts, d_off, d_pos, d_blk;
  BufGuard guard;
  guard.b = {&d_res, &d_starts, &d_off, &d_pos, &d_blk};
  HS_HIP(h, d_res.reserve((size_t)n_residues));
  HS_HIP(h, d_starts.reserve(((size_t)n_seq + 1) * 4));
  HS_HIP(h, d_off.reserve(((size_t)n_seq + 1) * 4));
  HS_HIP(h, d_pos.reserve((size_t)m * 4));
  HS_HIP(h, d_blk.reserve((size_t)m * k));
  HS_HIP(h, hipMemcpyAsync(d_res.p, residues, (size_t)n_residues, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipMemcpyAsync(d_starts.p, starts.data(), ((size_t)n_seq + 1) * 4, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipMemcpyAsync(d_off.p, win_off.data(), ((size_t)n_seq + 1) * 4, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hs_launch_windows(d_res.as<uint8_t>(), (uint32_t)n_residues, d_starts.as<uint32_t>(), d_off.as<uint32_t>(),
                              (uint32_t)n_seq, (int)k, d_blk.as<uint8_t>(), d_pos.as<uint32_t>(), h->stream));
  // (window_pos is written only once the block has passed its checks: index_append_resident's first step)
  hs_status st = index_append_resident(h, d_blk.as<uint8_t>(), m);
  if (st != HS_OK) return st;
  if (window_pos) {
    HS_HIP(h, hipMemcpyAsync(window_pos, d_pos.p, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  *n_windows = m;
  return HS_OK;
}

hs_status hs_index_table_append(const uint32_t* ids, const uint64_t* dir_key, const uint32_t* dir_start,
                                const int32_t* dir_tuple, uint64_t n, uint64_t nb, const int32_t* block_ints, uint64_t m,
                                uint32_t K, uint32_t seed, uint32_t* out_ids, uint64_t* out_dir_key,
                                uint32_t* out_dir_start, int32_t* out_dir_tuple, uint64_t dir_cap, uint64_t* nb_out,
                                uint32_t* collided) {
  return (hs_status)hs_table_append_host(ids, dir_key, dir_start, dir_tuple, n, nb, block_ints, m, K, seed, out_ids,
                                         out_dir_key, out_dir_start, out_dir_tuple, dir_cap, nb_out, collided);
}

// ---- hs_index_remove: a built index without a set of its k-mers (hs_remove.hip) -----------------------------------
namespace {
// the scratch of one removal, carved out of one allocation: 4 n bytes for new_id, n / 8 for the dead bitmap, 16 bytes
// per 64 entries for the masks, counts and scans of the id order and as much for one table's, one table's directory
struct RemoveScratch {
  uint64_t *dead, *imask, *tmask;
  uint32_t *icnt, *iscan, *tcnt, *tscan, *new_id, *alive, *alive_scan, *retuple, *retuple_scan, *out_count, *need_id,
      *need_bucket, *small;
  uint8_t* need_codes;
  int32_t* need_ints;
  void* scan_temp;
  size_t scan_temp_bytes;
};
size_t carve_remove_scratch(RemoveScratch& r, char* base, uint64_t n, int k, int K, uint64_t nb_max) {
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + at : nullptr;
    at += (bytes + 255) & ~(size_t)255;
    return p;
  };
  const uint64_t nw = (n + 63) / 64;
  r.dead = (uint64_t*)take((nw + 1) * 8);
  r.imask = (uint64_t*)take((nw + 1) * 8);
  r.tmask = (uint64_t*)take((nw + 1) * 8);
  r.icnt = (uint32_t*)take((nw + 1) * 4);
  r.iscan = (uint32_t*)take((nw + 1) * 4);
  r.tcnt = (uint32_t*)take((nw + 1) * 4);
  r.tscan = (uint32_t*)take((nw + 1) * 4);
  r.new_id = (uint32_t*)take(n * 4);
  r.alive = (uint32_t*)take((nb_max + 1) * 4);
  r.alive_scan = (uint32_t*)take((nb_max + 1) * 4);
  r.retuple = (uint32_t*)take((nb_max + 1) * 4);
  r.retuple_scan = (uint32_t*)take((nb_max + 1) * 4);
  r.out_count = (uint32_t*)take((nb_max + 1) * 4);
  r.need_id = (uint32_t*)take(nb_max * 4);
  r.need_bucket = (uint32_t*)take(nb_max * 4);
  r.small = (uint32_t*)take(64);
  r.need_codes = (uint8_t*)take(nb_max * k);
  r.need_ints = (int32_t*)take(nb_max * K * 4);
  r.scan_temp_bytes = hs_scan_u32_temp(std::max(nw, nb_max) + 2) + 256;
  r.scan_temp = take(r.scan_temp_bytes);
  return at;
}
}  // namespace

static hs_status remove_check(hs_handle* h) {
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_remove: no index to remove from (hs_index_build has not been called)");
  return HS_OK;
}

// the scratch of a removal from the handle's index, the dead bitmap and the flag word (small[0]) zeroed
static hs_status remove_begin(hs_handle* h, DevBuf& arena, RemoveScratch& r) {
  const uint64_t n = h->n;
  uint64_t nb_max = 0;
  for (uint32_t l = 0; l < h->p.L; ++l) nb_max = std::max<uint64_t>(nb_max, h->info.n_buckets[l]);
  HS_HIP(h, arena.reserve(carve_remove_scratch(r, nullptr, n, (int)h->p.k, (int)h->p.K, nb_max)));
  carve_remove_scratch(r, arena.as<char>(), n, (int)h->p.k, (int)h->p.K, nb_max);
  HS_HIP(h, hipMemsetAsync(r.dead, 0, ((n + 63) / 64 + 1) * 8, h->stream));
  HS_HIP(h, hipMemsetAsync(r.small, 0, 64, h->stream));
  return HS_OK;
}

// The L tables of the index compacted under the dead bitmap (r.dead, r.new_id; n2 survivors, 0 < n2 < n; h->n and
// h->codes are still the old ones: the new first members' codes are read from there).  On success the shrunken arrays
// are the handle's and the old ones are gone (finish_index is the caller's).
static hs_status remove_tables(hs_handle* h, RemoveScratch& r, uint64_t n2) {
  const uint64_t n = h->n, nw = (n + 63) / 64;
  const int K = (int)h->p.K, L = (int)h->p.L, k = (int)h->p.k, PW = h->PW;
  NewTables shrunk(h);
  HS_CHECK(reserve_table_rows(h, shrunk.packed, shrunk.rec8, shrunk.rho, shrunk.pos, n2));
  uint64_t new_nb[HS_MAX_L], new_max[HS_MAX_L], dead_buckets = 0, retupled = 0;
  double ms_hash = 0, ms_sort = 0, ms_gather = 0;
  for (int l = 0; l < L; ++l) {
    const uint32_t nb = (uint32_t)h->info.n_buckets[l];
    const hs_table_dev& tb = h->tabs.t[l];
    const RowSlice old = table_slice(h, l, n), dst = shrunk.slice(h, l, n2);
    HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
    // 1. the keep masks in table order, the buckets that survive and those that need a tuple
    HS_HIP(h, hs_launch_remove_masks_tab(tb.ids, r.dead, (uint32_t)n, r.tmask, r.tcnt, h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(r.scan_temp, r.scan_temp_bytes, r.tcnt, r.tscan, nw + 1, h->stream));
    HS_HIP(h, hs_launch_remove_dir_flags(tb.dir_start, nb, r.tmask, r.tscan, r.alive, r.retuple, h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(r.scan_temp, r.scan_temp_bytes, r.alive, r.alive_scan, (size_t)nb + 1, h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(r.scan_temp, r.scan_temp_bytes, r.retuple, r.retuple_scan, (size_t)nb + 1, h->stream));
    uint32_t nb2 = 0, n_need = 0, survivors = 0;
    HS_HIP(h, hipMemcpyAsync(&nb2, r.alive_scan + nb, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(&n_need, r.retuple_scan + nb, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(&survivors, r.tscan + nw, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    if (survivors != n2 || !nb2 || nb2 > nb || n_need > nb2)
      return fail(h, HS_ERR_HIP, "hs_index_remove: the table's survivor counts are inconsistent");
    // 2. the shrunken directory
    HS_HIP(h, shrunk.ids[l].reserve(std::max<size_t>(16, (size_t)n2 * 4)));
    HS_CHECK(reserve_directory(h, shrunk.key[l], shrunk.start[l], shrunk.tuple[l], nb2));
    uint32_t* const dst_ids = shrunk.ids[l].as<uint32_t>();
    uint32_t* const dst_start = shrunk.start[l].as<uint32_t>();
    int32_t* const dst_tuple = shrunk.tuple[l].as<int32_t>();
    HS_HIP(h, hs_launch_remove_dir_write(tb.dir_key, tb.dir_start, tb.dir_tuple, tb.ids, nb, (uint32_t)n, K, r.tmask,
                                         r.tscan, r.alive, r.alive_scan, r.retuple, r.retuple_scan, nb2,
                                         shrunk.key[l].as<uint64_t>(), dst_tuple, r.out_count, r.need_id, r.need_bucket,
                                         h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(r.scan_temp, r.scan_temp_bytes, r.out_count, dst_start, nb2, h->stream));
    HS_HIP(h, hs_launch_set_u32(dst_start + nb2, (uint32_t)n2, h->stream));
    HS_HIP(h, hipMemsetAsync(r.small + 2, 0, 4, h->stream));
    HS_HIP(h, hs_launch_max_u32(r.out_count, nb2, r.small + 2, h->stream));
    HS_HIP(h, hipEventRecord(h->ev[2], h->stream));
    // 3. the tuples of the buckets whose first member went: just those k-mers hashed, with this table's functions
    if (n_need) {
      HS_HIP(h, hs_launch_gather_rows(h->codes.as<uint8_t>(), r.need_id, n_need, k, r.need_codes, h->stream));
      HS_CHECK(hash_dispatch(h, r.need_codes, nullptr, n_need, l, r.need_ints, K, 0, h->stream));
      HS_HIP(h, hs_launch_remove_tuples_put(r.need_ints, r.need_bucket, n_need, K, nb2, dst_tuple, h->stream));
    }
    HS_HIP(h, hipEventRecord(h->ev[3], h->stream));
    // 4. the move
    HS_HIP(h, hs_launch_remove_move((uint32_t)n, (uint32_t)n2, r.tmask, r.tscan, r.new_id, PW, tb.ids, tb.packed,
                                    old.rec8, old.rho, dst_ids, dst.packed, dst.rec8, dst.rho, h->stream));
    HS_HIP(h, hs_launch_invert_perm(dst_ids, (uint32_t)n2, dst.pos, h->stream));
    HS_HIP(h, hipEventRecord(h->ev[4], h->stream));
    uint32_t max_count = 0;
    HS_HIP(h, hipMemcpyAsync(&max_count, r.small + 2, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    ms_sort += ev_ms(h, 1, 2);
    ms_hash += ev_ms(h, 2, 3);
    ms_gather += ev_ms(h, 3, 4);
    if (n_need) HS_CHECK(hash_account(h, n_need, K, 0));
    new_nb[l] = nb2;
    new_max[l] = max_count;
    dead_buckets += nb - nb2;
    retupled += n_need;
  }
  // every table is compacted: the shrunken arrays become the handle's (and the old ones go with `shrunk`)
  adopt_tables(h, n2, shrunk, new_nb, new_max);
  h->prof.ms_hash = ms_hash;
  h->prof.ms_sort = ms_sort;
  h->prof.ms_gather = ms_gather;
  h->prof.remove_dead_buckets = dead_buckets;
  h->prof.remove_retupled = retupled;
  return HS_OK;
}

// The dead bitmap is marked (r.dead; r.small[0] != 0: an id >= n).  Validation and new_id first; from drop_index on,
// every failure leaves the handle without an index.  new_id (optional): [n] of the old n, host or device memory.
static hs_status index_remove_marked(hs_handle* h, DevBuf& arena, RemoveScratch& r, uint32_t* new_id, bool new_id_dev) {
  const uint64_t n = h->n, nw = (n + 63) / 64;
  const int k = (int)h->p.k, PW = h->PW;
  HS_HIP(h, hs_launch_remove_masks_ids(r.dead, (uint32_t)n, r.imask, r.icnt, h->stream));
  HS_HIP(h, hs_exclusive_scan_u32(r.scan_temp, r.scan_temp_bytes, r.icnt, r.iscan, nw + 1, h->stream));
  HS_HIP(h, hs_launch_remove_new_id(r.imask, r.iscan, (uint32_t)n, r.new_id, h->stream));
  uint32_t bad = 0, n2_32 = 0;
  HS_HIP(h, hipMemcpyAsync(&bad, r.small, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(&n2_32, r.iscan + nw, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (bad) return fail(h, HS_ERR_INVALID, "hs_index_remove: an id is not below the index's n");
  const uint64_t n2 = n2_32;
  if (n2 > n) return fail(h, HS_ERR_HIP, "hs_index_remove: the survivor count is inconsistent");
  if (new_id && n) {
    HS_HIP(h, hipMemcpyAsync(new_id, r.new_id, (size_t)n * 4, new_id_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                             h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  if (n2 == n) return HS_OK;  // nothing was marked: the index stays as it is
  uint64_t nb_before = 0;
  for (uint32_t l = 0; l < h->p.L; ++l) nb_before += h->info.n_buckets[l];
  bool reseed = h->key_seed != 0;
#ifdef HS_TEST_HOOKS
  if (h->knobs.test_remove_reseed) reseed = true;
#endif
  // ---- the handle changes from here on
  drop_index(h);
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  DevBuf ncodes, npacked_all;
  BufGuard guard;
  guard.b = {&ncodes, &npacked_all};
  const bool rebuild = reseed || !n2;
  if (!rebuild) HS_CHECK(remove_tables(h, r, n2));
  // codes and packed k-mers in id order (after the tables: their new first members were read from the old codes)
  HS_HIP(h, ncodes.reserve(std::max<size_t>(16, (size_t)n2 * k)));
  if (!rebuild) HS_HIP(h, npacked_all.reserve(std::max<size_t>(16, (size_t)n2 * PW * 16)));
  HS_HIP(h, hs_launch_remove_compact_ids(h->codes.as<uint8_t>(), h->packed_all.as<uint4>(), n, k, PW, r.new_id,
                                         (uint32_t)n2, ncodes.as<uint8_t>(), rebuild ? nullptr : npacked_all.as<uint4>(),
                                         h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  std::swap(h->codes, ncodes);
  ncodes.release();
  if (!rebuild) {
    std::swap(h->packed_all, npacked_all);
    npacked_all.release();
  }
  arena.release();
  h->n = n2;
  if (!rebuild) {
    h->info.n = n2;
    return end_index(h);
  }
  // a seed above 0, or nothing left: the build loop over the compacted codes, resident already, from seed 0 -- where
  // hs_index_build over the survivors would have ended too
  memset(&h->info, 0, sizeof(h->info));
  hs_status st = index_build_resident(h, n2);
  if (st != HS_OK) return st;
  uint64_t nb_after = 0;
  for (uint32_t l = 0; l < h->p.L; ++l) nb_after += h->info.n_buckets[l];
  h->prof.remove_rebuilds = reseed && n2 ? 1 : 0;
  h->prof.remove_dead_buckets = nb_before > nb_after ? nb_before - nb_after : 0;
  return HS_OK;
}

hs_status hs_index_remove(hs_handle* h, const uint32_t* ids, uint64_t m, uint32_t* new_id) {
  if (!h || (m && !ids)) return HS_ERR_INVALID;
  HS_CHECK(remove_check(h));
  const uint64_t n = h->n;
  if (!m) {
    if (new_id)
      for (uint64_t i = 0; i < n; ++i) new_id[i] = (uint32_t)i;
    return HS_OK;
  }
  HS_CHECK(ensure_device(h));
  DevBuf arena, d_ids;
  BufGuard guard;
  guard.b = {&arena, &d_ids};
  RemoveScratch r;
  HS_HIP(h, d_ids.reserve((size_t)m * 4));
  HS_CHECK(remove_begin(h, arena, r));
  HS_HIP(h, hipMemcpyAsync(d_ids.p, ids, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hs_launch_remove_mark_ids(d_ids.as<uint32_t>(), m, (uint32_t)n, r.dead, r.small, h->stream));
  return index_remove_marked(h, arena, r, new_id, false);
}

hs_status hs_index_remove_dev(hs_handle* h, const uint32_t* d_ids, uint64_t m, uint32_t* d_new_id) {
  if (!h || (m && !d_ids)) return HS_ERR_INVALID;
  HS_CHECK(remove_check(h));
  HS_CHECK(ensure_device(h));
  const uint64_t n = h->n;
  if (!m) {
    if (d_new_id && n) {
      HS_HIP(h, hs_launch_iota_u32(d_new_id, (uint32_t)n, h->stream));
      HS_HIP(h, hipStreamSynchronize(h->stream));
    }
    return HS_OK;
  }
  DevBuf arena;
  BufGuard guard;
  guard.b = {&arena};
  RemoveScratch r;
  HS_CHECK(remove_begin(h, arena, r));
  HS_HIP(h, hs_launch_remove_mark_ids(d_ids, m, (uint32_t)n, r.dead, r.small, h->stream));
  return index_remove_marked(h, arena, r, d_new_id, true);
}

hs_status hs_index_remove_ranges(hs_handle* h, const uint64_t* first, const uint64_t* count, uint64_t n_ranges,
                                 uint32_t* new_id) {
  if (!h || (n_ranges && (!first || !count))) return HS_ERR_INVALID;
  HS_CHECK(remove_check(h));
  const uint64_t n = h->n;
  uint64_t marked = 0;
  for (uint64_t i = 0; i < n_ranges; ++i) {
    if (first[i] > n || count[i] > n - first[i])
      return fail(h, HS_ERR_INVALID, "hs_index_remove_ranges: a range ends beyond the index's n");
    marked |= count[i];
  }
  if (!marked) {
    if (new_id)
      for (uint64_t i = 0; i < n; ++i) new_id[i] = (uint32_t)i;
    return HS_OK;
  }
  HS_CHECK(ensure_device(h));
  DevBuf arena, d_ranges;
  BufGuard guard;
  guard.b = {&arena, &d_ranges};
  RemoveScratch r;
  HS_HIP(h, d_ranges.reserve((size_t)n_ranges * 16));
  HS_CHECK(remove_begin(h, arena, r));
  uint64_t* const d_first = d_ranges.as<uint64_t>();
  uint64_t* const d_count = d_first + n_ranges;
  HS_HIP(h, hipMemcpyAsync(d_first, first, (size_t)n_ranges * 8, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipMemcpyAsync(d_count, count, (size_t)n_ranges * 8, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hs_launch_remove_mark_ranges(d_first, d_count, n_ranges, (uint32_t)n, r.dead, h->stream));
  return index_remove_marked(h, arena, r, new_id, false);
}

hs_status hs_index_table_remove(const uint32_t* ids, const uint64_t* dir_key, const uint32_t* dir_start,
                                const int32_t* dir_tuple, uint64_t n, uint64_t nb, const uint32_t* dead_ids, uint64_t m,
                                const int32_t* ints, uint32_t K, uint32_t seed, uint32_t* out_ids, uint64_t* out_dir_key,
                                uint32_t* out_dir_start, int32_t* out_dir_tuple, uint64_t dir_cap, uint64_t* n_out,
                                uint64_t* nb_out) {
  return (hs_status)hs_table_remove_host(ids, dir_key, dir_start, dir_tuple, n, nb, dead_ids, m, ints, K, seed, out_ids,
                                         out_dir_key, out_dir_start, out_dir_tuple, dir_cap, n_out, nb_out);
}

// ---- persistent index --------------------------------------------------------------------------
// File = IndexFileHeader, then the payload: planes a, b, coordinate table (32 x 8 doubles), codes
// [n][k], and per table ids [n] u32, dir_key [nb] u64, dir_start [nb + 1] u32, dir_tuple [nb][K] i32.
// The header carries the payload's length and a 64-bit hash of it; hs_index_load checks both, then
// checks every table's CONTENT on the device before any kernel indexes with it (ids a permutation
// of 0..n-1 ascending inside a bucket, boundaries strictly ascending from 0 to n, fingerprints
// strictly ascending and equal to the fingerprint of the bucket's tuple): a corrupt, stale or
// hand-edited file gives HS_ERR_IO, never an out-of-bounds access.
namespace {
struct IndexFileHeader {
  char magic[8];  // "HSIDX002"
  uint32_t k, K, L, alphabet;
  double W;
  uint64_t n;
  uint32_t key_seed, pad;
  uint64_t n_buckets[HS_MAX_L], max_bucket[HS_MAX_L];
  uint64_t payload_bytes, payload_hash;
};
const char kIndexMagic[9] = "HSIDX002";
struct FileCloser {
  FILE* f;
  ~FileCloser() { if (f) fclose(f); }
};
// order-dependent 64-bit hash over the payload as a sequence of sections (same sequence on both sides)
struct PayloadHash {
  uint64_t h = 0x9e3779b97f4a7c15ull, bytes = 0;
  static uint64_t mix(uint64_t h, uint64_t w) {
    h = (h ^ w) * 0xff51afd7ed558ccdull;
    return h ^ (h >> 29);
  }
  void add(const void* p, size_t n) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    h = mix(h, (uint64_t)n);
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
      uint64_t w;
      memcpy(&w, c + i, 8);
      h = mix(h, w);
    }
    if (i < n) {
      uint64_t w = 0;
      memcpy(&w, c + i, n - i);
      h = mix(h, w);
    }
    bytes += n;
  }
};
const size_t kFileChunk = (size_t)64 << 20;
bool header_shape_ok(const IndexFileHeader& hd) {
  if (memcmp(hd.magic, kIndexMagic, 8) != 0) return false;
  if (hd.k < 1 || hd.k > 75 || hd.K < 1 || hd.K > HS_MAX_K || hd.L < 1 || hd.L > HS_MAX_L ||
      hd.alphabet < 1 || hd.alphabet > HS_ALPHABET_PAD || hd.n >= (1ull << 31))
    return false;
  for (uint32_t l = 0; l < hd.L; ++l)
    if (hd.n_buckets[l] > hd.n || (hd.n != 0) != (hd.n_buckets[l] != 0)) return false;
  return true;
}
uint64_t payload_size(const IndexFileHeader& hd) {
  uint64_t b = (uint64_t)hd.L * hd.K * 8 * hd.k * 8 + (uint64_t)hd.L * hd.K * 8 + HS_ALPHABET_PAD * 8 * 8 + hd.n * hd.k;
  for (uint32_t l = 0; l < hd.L; ++l)
    b += hd.n * 4 + hd.n_buckets[l] * 8 + (hd.n_buckets[l] + 1) * 4 + hd.n_buckets[l] * hd.K * 4;
  return b;
}
}  // namespace

static hs_status write_device(hs_handle* h, FILE* f, const void* d_ptr, size_t bytes, std::vector<char>* tmp,
                              PayloadHash* ph) {
  tmp->resize(std::min(bytes, kFileChunk));
  for (size_t off = 0; off < bytes; off += kFileChunk) {
    const size_t m = std::min(kFileChunk, bytes - off);
    HS_HIP(h, hipMemcpy(tmp->data(), (const char*)d_ptr + off, m, hipMemcpyDeviceToHost));
    ph->add(tmp->data(), m);
    if (fwrite(tmp->data(), 1, m, f) != m) return fail(h, HS_ERR_IO, "short write to the index file");
  }
  return HS_OK;
}
static hs_status read_device(hs_handle* h, FILE* f, void* d_ptr, size_t bytes, std::vector<char>* tmp,
                             PayloadHash* ph) {
  tmp->resize(std::min(bytes, kFileChunk));
  for (size_t off = 0; off < bytes; off += kFileChunk) {
    const size_t m = std::min(kFileChunk, bytes - off);
    if (fread(tmp->data(), 1, m, f) != m) return fail(h, HS_ERR_IO, "index file truncated");
    ph->add(tmp->data(), m);
    HS_HIP(h, hipMemcpy((char*)d_ptr + off, tmp->data(), m, hipMemcpyHostToDevice));
  }
  return HS_OK;
}

hs_status hs_index_save(hs_handle* h, const char* path) {
  if (!h || !path) return HS_ERR_INVALID;
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  HS_HIP(h, hipStreamSynchronize(h->stream));
  FILE* f = fopen(path, "wb");
  if (!f) return fail(h, HS_ERR_IO, std::string("cannot create ") + path);
  FileCloser closer = {f};
  IndexFileHeader hd;
  memset(&hd, 0, sizeof(hd));
  memcpy(hd.magic, kIndexMagic, 8);
  hd.k = h->p.k; hd.K = h->p.K; hd.L = h->p.L; hd.alphabet = (uint32_t)h->alphabet;
  hd.W = h->p.W; hd.n = h->n; hd.key_seed = h->key_seed;
  for (uint32_t l = 0; l < h->p.L; ++l) {
    hd.n_buckets[l] = h->info.n_buckets[l];
    hd.max_bucket[l] = h->info.max_bucket[l];
  }
  if (fwrite(&hd, sizeof(hd), 1, f) != 1) return fail(h, HS_ERR_IO, "short write to the index file");
  std::vector<char> tmp;
  PayloadHash ph;
  const size_t K = h->p.K, n = (size_t)h->n;
  HS_CHECK(write_device(h, f, h->a.p, (size_t)h->LK * h->d * 8, &tmp, &ph));
  HS_CHECK(write_device(h, f, h->b.p, (size_t)h->LK * 8, &tmp, &ph));
  HS_CHECK(write_device(h, f, h->coords.p, (size_t)HS_ALPHABET_PAD * 8 * 8, &tmp, &ph));
  HS_CHECK(write_device(h, f, h->codes.p, n * h->p.k, &tmp, &ph));
  for (uint32_t l = 0; l < h->p.L; ++l) {
    const size_t nb = (size_t)h->info.n_buckets[l];
    HS_CHECK(write_device(h, f, h->t_ids[l].p, n * 4, &tmp, &ph));
    HS_CHECK(write_device(h, f, h->t_dirkey[l].p, nb * 8, &tmp, &ph));
    HS_CHECK(write_device(h, f, h->t_dirstart[l].p, (nb + 1) * 4, &tmp, &ph));
    HS_CHECK(write_device(h, f, h->t_dirtuple[l].p, nb * K * 4, &tmp, &ph));
  }
  // the header again, now with the payload's length and hash
  hd.payload_bytes = ph.bytes;
  hd.payload_hash = ph.h;
  if (fseek(f, 0, SEEK_SET) != 0 || fwrite(&hd, sizeof(hd), 1, f) != 1 || fflush(f) != 0)
    return fail(h, HS_ERR_IO, "short write to the index file");
  return HS_OK;
}

hs_status hs_index_load(hs_handle* h, const char* path) {
  if (!h || !path) return HS_ERR_INVALID;
  hs_status st = ensure_device(h);
  if (st) return st;
  FILE* f = fopen(path, "rb");
  if (!f) return fail(h, HS_ERR_IO, std::string("cannot open ") + path);
  FileCloser closer = {f};
  IndexFileHeader hd;
  if (fread(&hd, sizeof(hd), 1, f) != 1 || !header_shape_ok(hd))
    return fail(h, HS_ERR_IO, "not an index file (or written by another version)");
  if (hd.k != h->p.k || hd.K != h->p.K || hd.L != h->p.L || hd.alphabet != (uint32_t)h->alphabet ||
      hd.W != h->p.W)
    return fail(h, HS_ERR_IO, "index file written for other parameters (k, K, L, W, alphabet)");
  if (hd.payload_bytes != payload_size(hd)) return fail(h, HS_ERR_IO, "index file inconsistent (payload length)");
  drop_index(h);
  memset(&h->prof, 0, sizeof(h->prof));
  memset(&h->info, 0, sizeof(h->info));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  std::vector<char> tmp, mine;
  PayloadHash ph;
  // planes and coordinate table must be the handle's, bit for bit
  const size_t sizes[3] = {(size_t)h->LK * h->d * 8, (size_t)h->LK * 8, (size_t)HS_ALPHABET_PAD * 8 * 8};
  const void* dev[3] = {h->a.p, h->b.p, h->coords.p};
  for (int i = 0; i < 3; ++i) {
    tmp.resize(sizes[i]);
    mine.resize(sizes[i]);
    if (fread(tmp.data(), 1, sizes[i], f) != sizes[i]) return fail(h, HS_ERR_IO, "index file truncated");
    ph.add(tmp.data(), sizes[i]);
    HS_HIP(h, hipMemcpy(mine.data(), dev[i], sizes[i], hipMemcpyDeviceToHost));
    if (memcmp(tmp.data(), mine.data(), sizes[i]) != 0)
      return fail(h, HS_ERR_IO, "index file written for other planes or another coordinate table");
  }
  const uint64_t n = hd.n;
  const int K = (int)h->p.K, L = (int)h->p.L, k = (int)h->p.k, PW = h->PW;
  h->n = n;
  h->key_seed = hd.key_seed;
  HS_HIP(h, h->codes.reserve(std::max<size_t>(16, (size_t)n * k)));
  HS_HIP(h, h->packed_all.reserve(std::max<size_t>(16, (size_t)n * PW * 16)));
  HS_HIP(h, h->counters.reserve(256));
  HS_CHECK(read_device(h, f, h->codes.p, (size_t)n * k, &tmp, &ph));
  if (n)
    HS_CHECK(pack_checked(h, h->codes.as<uint8_t>(), n, h->packed_all.as<uint4>(), HS_ERR_IO,
                          "index file holds a residue code outside the alphabet"));
  HS_CHECK(reserve_table_rows(h, h->t_packed, h->t_rec8, h->t_rho, h->t_pos, n));
  uint32_t* d_flag = h->counters.as<uint32_t>() + 16;  // [16] failure bits, [17 + l] largest bucket
  HS_HIP(h, hipMemsetAsync(d_flag, 0, (1 + HS_MAX_L) * 4, h->stream));
  for (int l = 0; l < L; ++l) {
    const size_t nb = (size_t)hd.n_buckets[l];
    HS_HIP(h, h->t_ids[l].reserve(std::max<size_t>(16, (size_t)n * 4)));
    HS_CHECK(reserve_directory(h, l, nb));
    HS_CHECK(read_device(h, f, h->t_ids[l].p, (size_t)n * 4, &tmp, &ph));
    HS_CHECK(read_device(h, f, h->t_dirkey[l].p, nb * 8, &tmp, &ph));
    HS_CHECK(read_device(h, f, h->t_dirstart[l].p, (nb + 1) * 4, &tmp, &ph));
    HS_CHECK(read_device(h, f, h->t_dirtuple[l].p, nb * K * 4, &tmp, &ph));
    // content checks BEFORE anything indexes with the table; pos_of comes out of them
    HS_HIP(h, hs_launch_validate_table(h->t_ids[l].as<uint32_t>(), (uint32_t)n, table_slice(h, l, n).pos,
                                       h->t_dirstart[l].as<uint32_t>(), h->t_dirkey[l].as<uint64_t>(),
                                       h->t_dirtuple[l].as<int32_t>(), (uint32_t)nb, K, hd.key_seed, d_flag,
                                       d_flag + 1 + l, h->stream));
    uint32_t flag = 0;
    HS_HIP(h, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    if (flag) {
      char msg[160];
      snprintf(msg, sizeof(msg), "index file corrupt: table %d fails its content checks (bits 0x%x: 1 id range, 2 id twice, "
               "4 boundaries, 8 key order, 16 key/tuple, 32 id order)", l, flag);
      return fail(h, HS_ERR_IO, msg);
    }
    HS_CHECK(gather_table_rows(h, l, n, false));
    publish_table(h, l, n, nb);
  }
  uint32_t maxb[HS_MAX_L] = {0};
  HS_HIP(h, hipMemcpyAsync(maxb, d_flag + 1, (size_t)L * 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  for (int l = 0; l < L; ++l) h->info.max_bucket[l] = maxb[l];  // recomputed, not taken on trust
  char extra;
  if (ph.bytes != hd.payload_bytes || ph.h != hd.payload_hash || fread(&extra, 1, 1, f) != 0)
    return fail(h, HS_ERR_IO, "index file corrupt (payload hash or length does not match the header)");
  return finish_index(h);
}

// Host-only check of an index file (no GPU, no handle): header, payload length and hash, and the
// content rules hs_index_load enforces on the device.  HS_OK or HS_ERR_IO with a message.
hs_status hs_index_file_check(const char* path, char* err, uint32_t err_cap) {
  auto say = [&](hs_status st, const std::string& msg) {
    if (err && err_cap) {
      strncpy(err, msg.c_str(), err_cap - 1);
      err[err_cap - 1] = 0;
    }
    return st;
  };
  if (!path) return say(HS_ERR_INVALID, "null path");
  FILE* f = fopen(path, "rb");
  if (!f) return say(HS_ERR_IO, std::string("cannot open ") + path);
  FileCloser closer = {f};
  IndexFileHeader hd;
  if (fread(&hd, sizeof(hd), 1, f) != 1 || !header_shape_ok(hd))
    return say(HS_ERR_IO, "not an index file (or written by another version)");
  if (hd.payload_bytes != payload_size(hd)) return say(HS_ERR_IO, "payload length does not match the header");
  PayloadHash ph;
  std::vector<char> buf;
  auto section = [&](size_t bytes, std::vector<char>* keep) -> bool {
    std::vector<char>& dst = keep ? *keep : buf;
    if (keep) {
      dst.resize(bytes);
      if (bytes && fread(dst.data(), 1, bytes, f) != bytes) return false;
      // hashed in the chunks read_device/write_device use
      for (size_t off = 0; off < bytes; off += kFileChunk) ph.add(dst.data() + off, std::min(kFileChunk, bytes - off));
      return true;
    }
    dst.resize(std::min(bytes, kFileChunk));
    for (size_t off = 0; off < bytes; off += kFileChunk) {
      const size_t m = std::min(kFileChunk, bytes - off);
      if (fread(dst.data(), 1, m, f) != m) return false;
      ph.add(dst.data(), m);
    }
    return true;
  };
  const size_t d = 8 * (size_t)hd.k, LK = (size_t)hd.L * hd.K, n = (size_t)hd.n, K = hd.K;
  // planes, offsets and the coordinate table are hashed one section each (sizes well under a chunk
  // for any admissible parameters except the planes of very long k-mers, chunked like the rest)
  std::vector<char> codes;
  if (!section(LK * d * 8, nullptr) || !section(LK * 8, nullptr) || !section(HS_ALPHABET_PAD * 8 * 8, nullptr) ||
      !section(n * hd.k, &codes))
    return say(HS_ERR_IO, "index file truncated");
  for (size_t i = 0; i < codes.size(); ++i)
    if ((unsigned char)codes[i] >= hd.alphabet) return say(HS_ERR_IO, "residue code outside the alphabet");
  std::vector<char> ids_b, key_b, start_b, tup_b;
  std::vector<unsigned char> seen;
  for (uint32_t l = 0; l < hd.L; ++l) {
    const size_t nb = (size_t)hd.n_buckets[l];
    if (!section(n * 4, &ids_b) || !section(nb * 8, &key_b) || !section((nb + 1) * 4, &start_b) ||
        !section(nb * K * 4, &tup_b))
      return say(HS_ERR_IO, "index file truncated");
    const uint32_t* ids = reinterpret_cast<const uint32_t*>(ids_b.data());
    const uint64_t* key = reinterpret_cast<const uint64_t*>(key_b.data());
    const uint32_t* start = reinterpret_cast<const uint32_t*>(start_b.data());
    const int32_t* tup = reinterpret_cast<const int32_t*>(tup_b.data());
    const std::string where = " (table " + std::to_string(l) + ")";
    seen.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
      if (ids[i] >= n) return say(HS_ERR_IO, "id out of range" + where);
      if (seen[ids[i]]) return say(HS_ERR_IO, "id listed twice" + where);
      seen[ids[i]] = 1;
    }
    if ((nb ? start[0] : 0u) != 0u || start[nb] != n) return say(HS_ERR_IO, "bucket boundaries do not span 0..n" + where);
    for (size_t b = 0; b < nb; ++b) {
      if (!(start[b] < start[b + 1]) || start[b + 1] > n) return say(HS_ERR_IO, "bucket boundaries not ascending" + where);
      if (b + 1 < nb && !(key[b] < key[b + 1])) return say(HS_ERR_IO, "fingerprints not ascending" + where);
      if (hs_key_of(tup + b * K, (int)K, hd.key_seed) != key[b])
        return say(HS_ERR_IO, "a bucket's tuple does not have its fingerprint" + where);
      for (uint32_t i = start[b] + 1; i < start[b + 1]; ++i)
        if (!(ids[i - 1] < ids[i])) return say(HS_ERR_IO, "ids not ascending inside a bucket" + where);
    }
  }
  char extra;
  if (ph.bytes != hd.payload_bytes || ph.h != hd.payload_hash || fread(&extra, 1, 1, f) != 0)
    return say(HS_ERR_IO, "payload hash or length does not match the header");
  return HS_OK;
}

hs_status hs_index_info_get(const hs_handle* h, hs_index_info* out) {
  if (!h || !out) return HS_ERR_INVALID;
  if (!h->built) return HS_ERR_STATE;
  *out = h->info;
  return HS_OK;
}

}  // extern "C"
