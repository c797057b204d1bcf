// hs_cluster_pssm.h -- the rules of hs_cluster_weighted_profile and hs_cluster_pssm_cover (include/hsearch.h) on the
// host: hs_cluster_weights_codes and hs_cluster_cover_codes.  Host-compilable: nothing here needs hipcc.  Compile with
// -ffp-contract=off (the score is a chain of rounded fp64 sums).
//
// ROWS are hs_cluster_profile's: the label values with at least min_size members, in ascending value.
// WEIGHTS: hs_pssm_weights.h's rule with the sites of row r being the members of row r -- the tuples (m = row, id =
// member) given to hs_pssm_weight_hits_host without id_start.  Integer sums: a pure function of (codes, labels, min_size).
// COVER: score(r, x) = the sum over p of S[r][p][x_p] from +0.0, left to right in fp64 (hs_pssm_scan's, bit for bit);
// min_score[r] = the smallest member score, compared on hs_pssm_order_key of the bits (no score is a NaN or -0.0: the
// entries are finite and at most 2^100, and x + y is -0.0 only for two negative zeros, which a sum from +0.0 never
// holds); argmin[r] = the smallest id among the members at the minimum.
#pragma once
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "hs_pssm_tables.h"
#include "hs_pssm_topk.h"
#include "hs_pssm_weights.h"

#define HS_CP_NOISE 0xffffffffu /* HS_NOISE */
#define HS_CP_MAX_K 75u

// What both rules refuse of (codes, n, k, alphabet, label, min_size), and the rows: row_of [n] (HS_CP_NOISE: no row),
// size [n].  Returns 0, or 1 for a refused argument.
inline int hs_cp_rows_host(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet, const uint32_t* label,
                           uint32_t min_size, std::vector<uint32_t>& row_of, std::vector<uint32_t>& size,
                           uint64_t* rows) {
  if (!min_size || k < 1 || k > HS_CP_MAX_K || alphabet < 1 || alphabet > 32 || n >= (1ull << 31) ||
      (n && (!codes || !label)))
    return 1;
  for (uint64_t i = 0; i < n; ++i)
    if (label[i] != HS_CP_NOISE && label[i] >= n) return 1;
  for (uint64_t i = 0; i < n * k; ++i)
    if (codes[i] >= alphabet) return 1;
  size.assign(n, 0u);
  row_of.assign(n, HS_CP_NOISE);
  for (uint64_t i = 0; i < n; ++i)
    if (label[i] != HS_CP_NOISE) ++size[label[i]];
  *rows = 0;
  for (uint64_t v = 0; v < n; ++v)
    if (size[v] >= min_size) row_of[v] = (uint32_t)(*rows)++;
  return 0;
}

// counts, wsum, distinct may be null.  Returns 0; 1 for a refused argument; 2 when memory ran out; 3 when the rows
// exceed cap (*n_out is set, nothing else is written).  Nothing is written on 1 and 2 but *n_out.
inline int hs_cluster_weights_codes_host(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet,
                                         const uint32_t* label, uint32_t min_size, uint32_t* out_label,
                                         uint32_t* out_size, uint32_t* counts, uint64_t* wcounts, uint64_t* wsum,
                                         uint32_t* distinct, uint64_t cap, uint64_t* n_out) {
  if (!n_out) return 1;
  *n_out = 0;
  if (cap && (!out_label || !out_size || !wcounts)) return 1;
  try {
    std::vector<uint32_t> row_of, size;
    uint64_t rows = 0;
    if (hs_cp_rows_host(codes, n, k, alphabet, label, min_size, row_of, size, &rows)) return 1;
    *n_out = rows;
    if (rows > cap) return 3;
    const size_t cells = (size_t)k * alphabet;
    std::vector<uint32_t> c(rows * cells, 0u);
    std::vector<uint64_t> u(rows * cells);
    for (uint64_t i = 0; i < n; ++i) {
      if (label[i] == HS_CP_NOISE || row_of[label[i]] == HS_CP_NOISE) continue;
      uint32_t* const dst = c.data() + row_of[label[i]] * cells;
      for (uint32_t p = 0; p < k; ++p) ++dst[(size_t)p * alphabet + codes[i * k + p]];
    }
    // everything is checked and allocated: the outputs
    for (uint64_t v = 0; v < n; ++v)
      if (row_of[v] != HS_CP_NOISE) {
        out_label[row_of[v]] = (uint32_t)v;
        out_size[row_of[v]] = size[v];
      }
    for (uint64_t r = 0; r < rows; ++r) {
      const uint32_t d = hs_pssm_weight_table(c.data() + r * cells, k, alphabet, u.data() + r * cells);
      if (distinct) distinct[r] = d;
      if (wsum) wsum[r] = 0;
    }
    if (rows) memset(wcounts, 0, rows * cells * 8);
    if (counts && rows) memcpy(counts, c.data(), rows * cells * 4);
    for (uint64_t i = 0; i < n; ++i) {
      if (label[i] == HS_CP_NOISE || row_of[label[i]] == HS_CP_NOISE) continue;
      const size_t at = row_of[label[i]] * cells;
      const uint8_t* const row = codes + i * k;
      uint64_t w = 0;
      for (uint32_t p = 0; p < k; ++p) w += u[at + (size_t)p * alphabet + row[p]];
      for (uint32_t p = 0; p < k; ++p) wcounts[at + (size_t)p * alphabet + row[p]] += w;
      if (wsum) wsum[row_of[label[i]]] += w;
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}

// the contract's score of one k-mer under one profile
inline double hs_cp_score(const double* S_row, const uint8_t* x, uint32_t k, uint32_t alphabet) {
  double s = 0.0;
  for (uint32_t p = 0; p < k; ++p) s = s + S_row[(size_t)p * alphabet + x[p]];
  return s;
}

// S [n_rows][k][alphabet] -> min_score [n_rows], argmin [n_rows].  Returns 0; 1 for a refused argument (hs_cp_rows_host's,
// a null array with rows, an entry hs_pssm_scan refuses, n_rows other than the rows the labels give); 2 when memory
// ran out.  Nothing is written unless 0 is returned.
inline int hs_cluster_cover_codes_host(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet,
                                       const uint32_t* label, uint32_t min_size, const double* S, uint64_t n_rows,
                                       double* min_score, uint32_t* argmin) {
  if (n_rows && (!S || !min_score || !argmin)) return 1;
  try {
    std::vector<uint32_t> row_of, size;
    uint64_t rows = 0;
    if (hs_cp_rows_host(codes, n, k, alphabet, label, min_size, row_of, size, &rows)) return 1;
    if (rows != n_rows) return 1;
    const size_t cells = (size_t)k * alphabet;
    for (uint64_t e = 0; e < rows * cells; ++e)
      if (hs_pssm_bad_value(S[e], HS_PSSM_MAX_ABS)) return 1;
    std::vector<uint64_t> best(rows, 0);
    std::vector<uint32_t> at(rows, HS_CP_NOISE);
    for (uint64_t i = 0; i < n; ++i) {  // ascending id: the first member at the minimum is the argmin
      if (label[i] == HS_CP_NOISE || row_of[label[i]] == HS_CP_NOISE) continue;
      const uint64_t r = row_of[label[i]];
      const double s = hs_cp_score(S + r * cells, codes + i * k, k, alphabet);
      uint64_t b;
      memcpy(&b, &s, 8);
      const uint64_t key = hs_pssm_order_key(b);
      if (at[r] == HS_CP_NOISE || key < best[r]) {
        best[r] = key;
        at[r] = (uint32_t)i;
      }
    }
    for (uint64_t r = 0; r < rows; ++r) {
      const uint64_t b = hs_pssm_order_bits(best[r]);
      memcpy(&min_score[r], &b, 8);
      argmin[r] = at[r];
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}
