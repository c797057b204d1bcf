// hs_pssm_seq.h -- the rule of hs_pssm_seq_scan (include/hsearch.h) on the host for any list of (m, id, score) tuples
// (hs_pssm_seq_hits), and the id_start check both forms of the call share.  Host-compilable: nothing here needs hipcc.
//
// THE RULE.  A hit (m, id) belongs to the sequence s = the LAST s with id_start[s] <= id (equal neighbours are
// sequences without ids; the last one that starts at or below id is the one that owns it).  One row per distinct
// (m, s), ascending: the number of hits, the best hit under (score descending, id ascending) -- hs_pssm_topk.h's order
// and key transform --, the smallest and the largest id - id_start[s].
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "hs_pssm_topk.h"

// id_start [n_seq + 1] as the contract wants it, but for its end (the caller compares id_start[n_seq] with n)
inline bool hs_pssm_seq_id_start_ok(const uint64_t* id_start, uint64_t n_seq) {
  if (!id_start || n_seq > (1ull << 32) || id_start[0] != 0) return false;
  for (uint64_t s = 0; s < n_seq; ++s)
    if (id_start[s + 1] < id_start[s]) return false;
  return true;
}

// Returns 0; 1 for an argument the contract refuses (nothing is written then); 2 when memory ran out; 3 when the rows
// exceed cap (*n_out is set, no row is written).  -0.0 in a tuple is read as +0.0 (no scan produces it).
inline int hs_pssm_seq_hits_host(const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                 uint64_t nm, const uint64_t* id_start, uint64_t n_seq, uint32_t* out_m,
                                 uint32_t* out_seq, uint32_t* out_count, double* out_best_score, uint32_t* out_best_id,
                                 uint32_t* out_lo, uint32_t* out_hi, uint64_t cap, uint64_t* n_out) {
  if (!n_out) return 1;
  *n_out = 0;
  if (n_tuples && (!m || !id || !score)) return 1;
  if (cap && (!out_m || !out_seq || !out_count || !out_best_score || !out_best_id || !out_lo || !out_hi)) return 1;
  if (!hs_pssm_seq_id_start_ok(id_start, n_seq) || id_start[n_seq] > (1ull << 32)) return 1;
  try {
    std::vector<uint64_t> live(n_tuples), key(n_tuples);
    for (uint64_t i = 0; i < n_tuples; ++i) {
      if (m[i] >= nm || id[i] >= id_start[n_seq] || score[i] != score[i]) return 1;
      const double s = score[i] == 0.0 ? 0.0 : score[i];
      uint64_t bits;
      memcpy(&bits, &s, 8);
      key[i] = hs_pssm_desc_key(bits);
      live[i] = i;
    }
    // (m, id, key): a repeated (m, id) lands side by side, and a row's hits are one run in id order
    std::sort(live.begin(), live.end(), [&](uint64_t x, uint64_t y) {
      if (m[x] != m[y]) return m[x] < m[y];
      if (id[x] != id[y]) return id[x] < id[y];
      return key[x] < key[y];
    });
    size_t kept = 0;
    for (size_t i = 0; i < live.size(); ++i) {
      if (i && m[live[i]] == m[live[i - 1]] && id[live[i]] == id[live[i - 1]]) {
        if (key[live[i]] != key[live[i - 1]]) return 1;  // two scores for one (m, id)
        continue;
      }
      live[kept++] = live[i];
    }
    live.resize(kept);
    struct Row {
      uint32_t m, s, count, best_id, lo, hi;
      uint64_t key;
    };
    std::vector<Row> rows;
    for (size_t i = 0; i < live.size(); ++i) {
      const uint64_t j = live[i];
      const uint32_t s = (uint32_t)(std::upper_bound(id_start, id_start + n_seq + 1, (uint64_t)id[j]) - id_start - 1);
      const uint32_t off = (uint32_t)(id[j] - id_start[s]);
      if (rows.empty() || rows.back().m != m[j] || rows.back().s != s) {
        rows.push_back(Row{m[j], s, 1u, id[j], off, off, key[j]});
        continue;
      }
      Row& r = rows.back();  // (ids ascend within the run: an equal key keeps the earlier, smaller id)
      ++r.count;
      r.hi = off;
      if (key[j] < r.key) {
        r.key = key[j];
        r.best_id = id[j];
      }
    }
    // everything is checked: the rows
    *n_out = rows.size();
    if (rows.size() > cap) return 3;
    for (size_t i = 0; i < rows.size(); ++i) {
      const uint64_t bits = hs_pssm_desc_bits(rows[i].key);
      out_m[i] = rows[i].m;
      out_seq[i] = rows[i].s;
      out_count[i] = rows[i].count;
      memcpy(&out_best_score[i], &bits, 8);
      out_best_id[i] = rows[i].best_id;
      out_lo[i] = rows[i].lo;
      out_hi[i] = rows[i].hi;
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}
