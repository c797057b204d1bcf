// hs_pssm_weights.h -- the rules of hs_pssm_weighted_counts / hs_pssm_refine_weighted (include/hsearch.h) on the host:
// position-based sequence weights (Henikoff and Henikoff 1994) in integers over any list of (m, id, score) tuples
// (hs_pssm_weight_hits), and the log-odds of such weighted counts (hs_pssm_log_odds_weighted).  Host-compilable:
// nothing here needs hipcc.  Compile with -ffp-contract=off: every operation of the log-odds is rounded to fp64 on its
// own.
//
// THE WEIGHTING RULE.  The sites of profile m are hs_pssm_counts.h's, c[p][a] its raw counts.
//   r[p]        = the residues a with c[p][a] > 0;  distinct[m] = the sum over p of r[p]
//   u[p][a]     = floor(2^56 / (r[p] * c[p][a])), 0 where c[p][a] == 0          (hs_pssm_weight_unit; r c <= 32 * 2^32)
//   W(i)        = the sum over p of u[p][x_ip]                                   (the weight of site i, a uint64)
//   wcounts[m][p][a] = the sum of W(i) over the sites with x_ip == a;  wsum[m] = the sum of W(i) over the sites
// Every site adds W(i) to one bin of every position, so the sum over a of wcounts[m][p][a] is wsum[m] for every p.
// NOTHING OVERFLOWS.  wsum = sum_i sum_p u[p][x_ip] = sum_p sum_a c[p][a] * u[p][a], and c * floor(2^56 / (r c)) <=
// 2^56 / r for each of the r residues that occur, so a position adds at most 2^56 and wsum <= k * 2^56 < 2^63 for k <=
// 127.  Every W(i) and every wcounts entry is a partial sum of wsum's terms.  All sums are integer sums: the result
// does not depend on the order of the sites.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "hs_pssm_counts.h"

#if defined(__HIPCC__)
#define HS_PW_HD __host__ __device__
#else
#define HS_PW_HD
#endif

#define HS_PSSM_WEIGHT_ONE (1ull << 56) /* what one position shares out among its sites */
#define HS_PSSM_WEIGHT_MAX_K 127u       /* k * 2^56 < 2^63 */

// u(r, c): r = the residues that occur at the position (1 .. 32), c = how often this one does (0: it does not)
HS_PW_HD inline uint64_t hs_pssm_weight_unit(uint32_t r, uint32_t c) {
  return r && c ? HS_PSSM_WEIGHT_ONE / ((uint64_t)r * c) : 0ull;
}

// One profile's table: u_out [k][alphabet] from counts_row [k][alphabet]; returns distinct.
inline uint32_t hs_pssm_weight_table(const uint32_t* counts_row, uint32_t k, uint32_t alphabet, uint64_t* u_out) {
  uint32_t distinct = 0;
  for (uint32_t p = 0; p < k; ++p) {
    const uint32_t* const c = counts_row + (size_t)p * alphabet;
    uint32_t r = 0;
    for (uint32_t a = 0; a < alphabet; ++a) r += c[a] > 0;
    for (uint32_t a = 0; a < alphabet; ++a) u_out[(size_t)p * alphabet + a] = hs_pssm_weight_unit(r, c[a]);
    distinct += r;
  }
  return distinct;
}

// The rule over any tuple list in any order; the site selection and its refusals are hs_pssm_count_hits_host's.
// counts, wsum, distinct and used may be null.  Returns 0; 1 for an argument the contract refuses (nothing is written
// then); 2 when memory ran out.
inline int hs_pssm_weight_hits_host(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet, const uint32_t* m,
                                    const uint32_t* id, const double* score, uint64_t n_tuples, uint64_t nm,
                                    const uint64_t* id_start, uint64_t n_seq, uint32_t* counts, uint64_t* wcounts,
                                    uint64_t* wsum, uint32_t* distinct, uint64_t* used) {
  if ((nm && !wcounts) || k > HS_PSSM_WEIGHT_MAX_K) return 1;
  try {
    std::vector<uint32_t> site_m, site_id;
    const int r = hs_pssm_sites_host(codes, n, k, alphabet, m, id, score, n_tuples, nm, id_start, n_seq, site_m, site_id);
    if (r) return r;
    const size_t cells = (size_t)k * alphabet;
    std::vector<uint32_t> c((size_t)nm * cells, 0u);
    std::vector<uint64_t> u((size_t)nm * cells);
    for (size_t i = 0; i < site_id.size(); ++i) {
      uint32_t* const dst = c.data() + (size_t)site_m[i] * cells;
      const uint8_t* const row = codes + (size_t)site_id[i] * k;
      for (uint32_t p = 0; p < k; ++p) ++dst[(size_t)p * alphabet + row[p]];
    }
    // everything is checked and allocated: the outputs
    for (uint64_t j = 0; j < nm; ++j) {
      const uint32_t d = hs_pssm_weight_table(c.data() + j * cells, k, alphabet, u.data() + j * cells);
      if (distinct) distinct[j] = d;
      if (wsum) wsum[j] = 0;
      if (used) used[j] = 0;
    }
    if (nm) memset(wcounts, 0, (size_t)nm * cells * 8);
    if (counts && nm) memcpy(counts, c.data(), (size_t)nm * cells * 4);
    for (size_t i = 0; i < site_id.size(); ++i) {
      const size_t at = (size_t)site_m[i] * cells;
      const uint8_t* const row = codes + (size_t)site_id[i] * k;
      uint64_t w = 0;
      for (uint32_t p = 0; p < k; ++p) w += u[at + (size_t)p * alphabet + row[p]];
      for (uint32_t p = 0; p < k; ++p) wcounts[at + (size_t)p * alphabet + row[p]] += w;
      if (wsum) wsum[site_m[i]] += w;
      if (used) ++used[site_m[i]];
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}

// one entry: wc of the position's wsum, scaled to n_eff observations
inline double hs_pssm_log_odds_weighted_entry(uint64_t wc, uint64_t wsum, double n_eff, double bg, double pseudo) {
  const double f = wsum ? (double)wc / (double)wsum : 0.0;
  const double a = f * n_eff;
  const double b = pseudo * bg;
  const double num = a + b;
  const double den = n_eff + pseudo;
  const double freq = num / den;
  const double ratio = freq / bg;
  return log2(ratio);
}

// S[m][p][a] = log2(((f * n_eff[m] + pseudo * bg[a]) / (n_eff[m] + pseudo)) / bg[a]), f = wcounts[m][p][a] / wsum[m] (0
// where wsum[m] == 0).  Returns 0; 1 for what hs_pssm_log_odds_host refuses, an n_eff that is not finite or below 0, a
// wcounts entry above its wsum, or an entry that would not be finite (nothing is written then).
inline int hs_pssm_log_odds_weighted_host(const uint64_t* wcounts, const uint64_t* wsum, const double* n_eff,
                                          uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg, double pseudo,
                                          double* S_out) {
  if (!k || !alphabet || alphabet > 32 || nm >= (1ull << 27)) return 1;
  if (nm && (!wcounts || !wsum || !n_eff || !S_out)) return 1;
  if (!hs_pssm_bg_ok(bg, alphabet, pseudo)) return 1;
  const size_t cells = (size_t)k * alphabet;
  for (uint64_t j = 0; j < nm; ++j) {
    if (!(n_eff[j] >= 0.0 && n_eff[j] <= 1.7976931348623157e308)) return 1;
    for (size_t e = 0; e < cells; ++e)
      if (wcounts[j * cells + e] > wsum[j]) return 1;
  }
  for (int pass = 0; pass < 2; ++pass)
    for (uint64_t j = 0; j < nm; ++j)
      for (size_t e = 0; e < cells; ++e) {
        const double v = hs_pssm_log_odds_weighted_entry(wcounts[j * cells + e], wsum[j], n_eff[j], bg[e % alphabet],
                                                         pseudo);
        if (pass)
          S_out[j * cells + e] = v;
        else if (!(v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308))
          return 1;
      }
  return 0;
}
