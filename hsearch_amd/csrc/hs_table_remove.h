// hs_table_remove.h -- hs_index_table_remove (include/hsearch.h): one table of an index without a set of its ids,
// on the host.  Plain C++ (no HIP): hs_capi_index.hip wraps it, and the tests compile it with a stand-alone main under
// the sanitizers.  The rule is hs_remove.hip's: entries ordered by (fingerprint, id), survivors renumbered in
// their old order, so the table over the remainder is a compaction of the entries and of the directory.  A bucket
// keeps its fingerprint (it belongs to the HashKey string); its tuple is copied while its first member survives
// and otherwise read from `ints`, the bucket ints of the member that is now its first.
// Returns 0 (HS_OK), 1 (HS_ERR_INVALID) or 4 (HS_ERR_CAPACITY).
#ifndef HS_TABLE_REMOVE_H
#define HS_TABLE_REMOVE_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "hs_key.h"

inline int hs_table_remove_host(const uint32_t* ids, const uint64_t* dir_key, const uint32_t* dir_start,
                                const int32_t* dir_tuple, uint64_t n, uint64_t nb, const uint32_t* dead_ids,
                                uint64_t m, const int32_t* ints, uint32_t K, uint32_t seed, uint32_t* out_ids,
                                uint64_t* out_dir_key, uint32_t* out_dir_start, int32_t* out_dir_tuple,
                                uint64_t dir_cap, uint64_t* n_out, uint64_t* nb_out) {
  if (!n_out || !nb_out || K < 1 || K > HS_MAX_K || n >= (1ull << 31) || nb > n || (n != 0) != (nb != 0)) return 1;
  if ((n && !ids) || (nb && (!dir_key || !dir_tuple)) || !dir_start || (m && !dead_ids)) return 1;
  *n_out = 0;
  *nb_out = 0;
  // the table's structure: what the compaction indexes with (hs_index_file_check's content rules)
  {
    std::vector<unsigned char> seen((size_t)n, 0);
    for (uint64_t i = 0; i < n; ++i) {
      if (ids[i] >= n || seen[ids[i]]) return 1;
      seen[ids[i]] = 1;
    }
    if ((nb ? dir_start[0] : 0u) != 0u || dir_start[nb] != n) return 1;
    for (uint64_t b = 0; b < nb; ++b) {
      if (!(dir_start[b] < dir_start[b + 1]) || dir_start[b + 1] > n) return 1;
      if (b + 1 < nb && !(dir_key[b] < dir_key[b + 1])) return 1;
      for (uint32_t i = dir_start[b] + 1; i < dir_start[b + 1]; ++i)
        if (!(ids[i - 1] < ids[i])) return 1;
      if (hs_key_of(dir_tuple + b * K, (int)K, seed) != dir_key[b]) return 1;
    }
  }
  // mark (any order, duplicates allowed), then the new id of every survivor
  std::vector<unsigned char> dead((size_t)n, 0);
  for (uint64_t i = 0; i < m; ++i) {
    if (dead_ids[i] >= n) return 1;
    dead[dead_ids[i]] = 1;
  }
  std::vector<uint32_t> new_id((size_t)n);
  uint64_t n2 = 0;
  for (uint64_t i = 0; i < n; ++i) new_id[i] = dead[i] ? 0xffffffffu : (uint32_t)n2++;
  // the directory that survives; a bucket whose first member went needs the ints of its new first member
  uint64_t nb2 = 0;
  for (uint64_t b = 0; b < nb; ++b) {
    uint32_t i = dir_start[b];
    while (i < dir_start[b + 1] && dead[ids[i]]) ++i;
    if (i == dir_start[b + 1]) continue;
    if (i != dir_start[b] && !ints) return 1;
    ++nb2;
  }
  *n_out = n2;
  *nb_out = nb2;
  if (dir_cap < nb2) return 4;
  if (!out_ids || !out_dir_key || !out_dir_start || !out_dir_tuple) {  // (arrays of no elements may be null)
    if (n2 || nb2) return 1;
    if (out_dir_start) out_dir_start[0] = 0;
    return 0;
  }
  uint64_t ob = 0, at = 0;
  for (uint64_t b = 0; b < nb; ++b) {
    const uint64_t at0 = at;
    uint32_t first = 0xffffffffu;
    for (uint32_t i = dir_start[b]; i < dir_start[b + 1]; ++i) {
      if (dead[ids[i]]) continue;
      if (first == 0xffffffffu) first = i;
      out_ids[at++] = new_id[ids[i]];
    }
    if (at == at0) continue;
    out_dir_key[ob] = dir_key[b];
    out_dir_start[ob] = (uint32_t)at0;
    memcpy(out_dir_tuple + ob * K, first == dir_start[b] ? dir_tuple + b * K : ints + (uint64_t)ids[first] * K,
           (size_t)K * 4);
    ++ob;
  }
  out_dir_start[ob] = (uint32_t)at;
  return 0;
}

#endif
