// hs_table_append.h -- hs_index_table_append (include/hsearch.h): one table of an index merged with the bucket ints
// of an appended block, on the host.  Plain C++ (no HIP): hs_capi_index.hip wraps it, and the tests compile it with a
// stand-alone main under the sanitizers.  The rule is hs_append.hip's: entries ordered by (fingerprint, id), the
// block's ids all larger than the table's, an old bucket keeps its tuple.
// Returns 0 (HS_OK), 1 (HS_ERR_INVALID) or 4 (HS_ERR_CAPACITY).
#ifndef HS_TABLE_APPEND_H
#define HS_TABLE_APPEND_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "hs_key.h"

inline int hs_table_append_host(const uint32_t* ids, const uint64_t* dir_key, const uint32_t* dir_start,
                                const int32_t* dir_tuple, uint64_t n, uint64_t nb, const int32_t* block_ints,
                                uint64_t m, uint32_t K, uint32_t seed, uint32_t* out_ids, uint64_t* out_dir_key,
                                uint32_t* out_dir_start, int32_t* out_dir_tuple, uint64_t dir_cap, uint64_t* nb_out,
                                uint32_t* collided) {
  if (!nb_out || !collided || K < 1 || K > HS_MAX_K || n + m >= (1ull << 31) || nb > n || (n != 0) != (nb != 0))
    return 1;
  if ((n && !ids) || (nb && (!dir_key || !dir_tuple)) || !dir_start || (m && !block_ints)) return 1;
  *nb_out = 0;
  *collided = 0;
  // the table's structure: what the merge indexes with (hs_index_file_check's rules but the key-of-tuple one)
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
    }
  }
  // the block grouped as a build groups a table: (fingerprint, id) order, exact string equality inside a run
  std::vector<uint64_t> fp((size_t)m);
  for (uint64_t i = 0; i < m; ++i) fp[i] = hs_key_of(block_ints + i * K, (int)K, seed);
  std::vector<uint32_t> order((size_t)m);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return fp[x] != fp[y] ? fp[x] < fp[y] : x < y; });
  struct Run { uint64_t key; uint32_t first, count, old; bool is_new; };  // first: position in `order`
  std::vector<Run> runs;
  for (uint64_t i = 0; i < m; ++i) {
    const uint32_t id = order[i];
    if (runs.empty() || runs.back().key != fp[id]) {
      runs.push_back(Run{fp[id], (uint32_t)i, 1u, 0u, true});
    } else {
      if (!hs_key_equal(block_ints + (uint64_t)order[runs.back().first] * K, block_ints + (uint64_t)id * K, (int)K)) {
        *collided = 1;
        return 0;
      }
      ++runs.back().count;
    }
  }
  // match: the bucket, or the insertion rank
  uint64_t n_new = 0;
  for (Run& r : runs) {
    const uint64_t at = (uint64_t)(std::lower_bound(dir_key, dir_key + nb, r.key) - dir_key);
    r.old = (uint32_t)at;
    r.is_new = !(at < nb && dir_key[at] == r.key);
    if (!r.is_new && !hs_key_equal(block_ints + (uint64_t)order[r.first] * K, dir_tuple + at * K, (int)K)) {
      *collided = 1;
      return 0;
    }
    n_new += r.is_new;
  }
  for (uint64_t b = 0; b < nb; ++b)
    if (hs_key_of(dir_tuple + b * K, (int)K, seed) != dir_key[b]) return 1;
  *nb_out = nb + n_new;
  if (dir_cap < *nb_out) return 4;
  if (!out_ids || !out_dir_key || !out_dir_start || !out_dir_tuple) return n + m || *nb_out ? 1 : 0;
  // merge of the two directories, the entries moved behind one another
  uint64_t b = 0, j = 0, ob = 0, at = 0;
  while (b < nb || j < runs.size()) {
    const bool take_old = b < nb && (j >= runs.size() || dir_key[b] <= runs[j].key);
    const bool take_blk = j < runs.size() && (b >= nb || runs[j].key <= dir_key[b]);
    out_dir_key[ob] = take_old ? dir_key[b] : runs[j].key;
    out_dir_start[ob] = (uint32_t)at;
    memcpy(out_dir_tuple + ob * K, take_old ? dir_tuple + b * K : block_ints + (uint64_t)order[runs[j].first] * K,
           (size_t)K * 4);
    if (take_old) {
      for (uint32_t i = dir_start[b]; i < dir_start[b + 1]; ++i) out_ids[at++] = ids[i];
      ++b;
    }
    if (take_blk) {
      for (uint32_t i = 0; i < runs[j].count; ++i) out_ids[at++] = (uint32_t)(n + order[runs[j].first + i]);
      ++j;
    }
    ++ob;
  }
  out_dir_start[ob] = (uint32_t)at;
  return 0;
}

#endif
