// hs_pssm_counts.h -- the rules of hs_pssm_hit_counts / hs_pssm_refine (include/hsearch.h) on the host: the position
// frequency matrices of any list of (m, id, score) tuples (hs_pssm_count_hits), the log-odds of such counts
// (hs_pssm_log_odds) and the residue composition of one profile's counts (hs_pssm_background).  Host-compilable: nothing
// here needs hipcc.  Compile with -ffp-contract=off: every operation of the log-odds is rounded to fp64 on its own.
//
// THE COUNTING RULE.  Without id_start every distinct (m, id) is a site; with id_start the sites are the best hits of
// the rows of hs_pssm_seq.h's rule, one per distinct (m, sequence).  counts[m][p][a] = the sites (m, id) with
// codes[id][p] == a; used[m] = the sites of m.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "hs_pssm_seq.h"

// The sites of a tuple list, each once, with everything the counting rule refuses about the list checked (the output
// arrays are the caller's business).  Returns 0; 1 for a refused argument; 2 when memory ran out.
// id_start == nullptr: every site counts (n_seq is not looked at); else id_start [n_seq + 1] must ascend from 0 to n.
inline int hs_pssm_sites_host(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet, const uint32_t* m,
                              const uint32_t* id, const double* score, uint64_t n_tuples, uint64_t nm,
                              const uint64_t* id_start, uint64_t n_seq, std::vector<uint32_t>& site_m,
                              std::vector<uint32_t>& site_id) {
  if (!k || !alphabet || alphabet > 32 || n > (1ull << 32) || nm >= (1ull << 27)) return 1;
  if (n_tuples && (!m || !id || !score)) return 1;
  if (n && !codes) return 1;
  if (id_start && (!hs_pssm_seq_id_start_ok(id_start, n_seq) || id_start[n_seq] != n)) return 1;
  try {
    if (id_start) {
      std::vector<uint32_t> seq(n_tuples), count(n_tuples), lo(n_tuples), hi(n_tuples);
      std::vector<double> best(n_tuples);
      site_m.resize(n_tuples);
      site_id.resize(n_tuples);
      uint64_t rows = 0;
      // (with no tuple the vectors are empty: cap = 0 takes no array)
      const int r = hs_pssm_seq_hits_host(m, id, score, n_tuples, nm, id_start, n_seq, site_m.data(), seq.data(),
                                          count.data(), best.data(), site_id.data(), lo.data(), hi.data(), n_tuples,
                                          &rows);
      if (r) return r == 2 ? 2 : 1;
      site_m.resize(rows);
      site_id.resize(rows);
    } else {
      std::vector<uint64_t> live(n_tuples), key(n_tuples);
      for (uint64_t i = 0; i < n_tuples; ++i) {
        if (m[i] >= nm || id[i] >= n || score[i] != score[i]) return 1;
        const double s = score[i] == 0.0 ? 0.0 : score[i];
        memcpy(&key[i], &s, 8);
        live[i] = i;
      }
      std::sort(live.begin(), live.end(), [&](uint64_t x, uint64_t y) {
        if (m[x] != m[y]) return m[x] < m[y];
        if (id[x] != id[y]) return id[x] < id[y];
        return key[x] < key[y];
      });
      for (size_t i = 0; i < live.size(); ++i) {
        if (i && m[live[i]] == m[live[i - 1]] && id[live[i]] == id[live[i - 1]]) {
          if (key[live[i]] != key[live[i - 1]]) return 1;  // two scores for one (m, id)
          continue;
        }
        site_m.push_back(m[live[i]]);
        site_id.push_back(id[live[i]]);
      }
    }
    for (size_t i = 0; i < site_id.size(); ++i)
      for (uint32_t p = 0; p < k; ++p)
        if (codes[(size_t)site_id[i] * k + p] >= alphabet) return 1;
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}

// Returns 0; 1 for an argument the contract refuses (nothing is written then); 2 when memory ran out.
inline int hs_pssm_count_hits_host(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet, const uint32_t* m,
                                   const uint32_t* id, const double* score, uint64_t n_tuples, uint64_t nm,
                                   const uint64_t* id_start, uint64_t n_seq, uint32_t* counts, uint64_t* used) {
  if (nm && !counts) return 1;
  try {
    std::vector<uint32_t> site_m, site_id;
    const int r = hs_pssm_sites_host(codes, n, k, alphabet, m, id, score, n_tuples, nm, id_start, n_seq, site_m, site_id);
    if (r) return r;
    // everything is checked: the counts
    const size_t cells = (size_t)k * alphabet;
    if (nm) memset(counts, 0, (size_t)nm * cells * 4);
    if (used)
      for (uint64_t j = 0; j < nm; ++j) used[j] = 0;
    for (size_t i = 0; i < site_id.size(); ++i) {
      uint32_t* const dst = counts + (size_t)site_m[i] * cells;
      const uint8_t* const row = codes + (size_t)site_id[i] * k;
      for (uint32_t p = 0; p < k; ++p) ++dst[(size_t)p * alphabet + row[p]];
      if (used) ++used[site_m[i]];
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}

inline bool hs_pssm_bg_ok(const double* bg, uint32_t alphabet, double pseudo) {
  if (!bg || !(pseudo > 0.0) || !(pseudo <= 1.7976931348623157e308)) return false;
  for (uint32_t a = 0; a < alphabet; ++a)
    if (!(bg[a] > 0.0) || !(bg[a] <= 1.7976931348623157e308)) return false;
  return true;
}

// one entry: size = the sum over a of the position's counts
inline double hs_pssm_log_odds_entry(uint32_t c, uint64_t size, double bg, double pseudo) {
  const double prod = pseudo * bg;
  const double num = (double)c + prod;
  const double den = (double)size + pseudo;
  const double freq = num / den;
  const double ratio = freq / bg;
  return log2(ratio);
}

// S[m][p][a] = log2((((double)c + pseudo * bg[a]) / ((double)size + pseudo)) / bg[a]).  Returns 0; 1 for an argument
// the contract refuses, or a bg / pseudo so extreme that an entry would not be finite (nothing is written then).
inline int hs_pssm_log_odds_host(const uint32_t* counts, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                 double pseudo, double* S_out) {
  if (!k || !alphabet || alphabet > 32 || nm >= (1ull << 27)) return 1;
  if (nm && (!counts || !S_out)) return 1;
  if (!hs_pssm_bg_ok(bg, alphabet, pseudo)) return 1;
  for (int pass = 0; pass < 2; ++pass)
    for (uint64_t r = 0; r < nm * k; ++r) {
      const uint32_t* const c = counts + r * alphabet;
      uint64_t size = 0;
      for (uint32_t a = 0; a < alphabet; ++a) size += c[a];
      for (uint32_t a = 0; a < alphabet; ++a) {
        const double v = hs_pssm_log_odds_entry(c[a], size, bg[a], pseudo);
        if (pass)
          S_out[r * alphabet + a] = v;
        else if (!(v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308))
          return 1;
      }
    }
  return 0;
}

// bg[a] = (the sum over p of counts_row[p][a]) / (the sum over p and a); a zero becomes the smallest positive entry,
// without renormalising.  Returns 0; 1 for a refused argument or all-zero counts (nothing is written then).
inline int hs_pssm_background_host(const uint32_t* counts_row, uint32_t k, uint32_t alphabet, double* bg_out) {
  if (!k || !alphabet || alphabet > 32 || !counts_row || !bg_out) return 1;
  uint64_t col[32], total = 0;
  for (uint32_t a = 0; a < alphabet; ++a) {
    col[a] = 0;
    for (uint32_t p = 0; p < k; ++p) col[a] += counts_row[(size_t)p * alphabet + a];
    total += col[a];
  }
  if (!total) return 1;
  double least = 2.0;
  for (uint32_t a = 0; a < alphabet; ++a) {
    bg_out[a] = (double)col[a] / (double)total;
    if (col[a] && bg_out[a] < least) least = bg_out[a];
  }
  for (uint32_t a = 0; a < alphabet; ++a)
    if (!col[a]) bg_out[a] = least;
  return 0;
}
