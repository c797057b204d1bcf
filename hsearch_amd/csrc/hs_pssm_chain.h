// hs_pssm_chain.h -- the rule of hs_pssm_family_chain (include/hsearch.h) on the host: any list of (m, id, score)
// tuples reduced to the best gapped chain per (family, sequence) (hs_pssm_family_chain_hits), and the argument checks
// both forms of the device call share.  Host-compilable: nothing here needs hipcc.
//
// THE CHAIN RULE.  A hit (m, id) has g, s, off and diag = off - m_off[m] as in hs_pssm_family.h.  Hit j may precede
// hit i iff they share (g, s), m_j < m_i, off_j < off_i and d = |diag_i - diag_j| <= max_shift.  The link costs
// pen(0) = +0.0 and pen(d) = gap_open + gap_ext * (double)d otherwise: the product rounded, then the sum.  With the
// hits of a (g, s) segment in ascending (m, id):
//   v(j)   = C(j) - pen(d), and C(j) itself at d = 0
//   best j = the first predecessor under (v descending, n descending, m descending, id ascending)
//   taken iff v(best) > +0.0:  C(i) = v + score_i, n(i) = n(j) + 1, first(i) = first(j), gaps(i) = gaps(j) + (d != 0)
//   else the chain starts at i: C(i) = +0.0 + score_i, n(i) = 1, first(i) = i, gaps(i) = 0
// A predecessor that is not above +0.0 is never taken, so only those are compared here: the result is the same.
// One row per (g, s): among the hits with n >= min_count and (t_group == NULL or C >= t_group[g]) the first under
// (C descending, n descending, m ascending, id ascending); a segment without such a hit reports nothing.
//
// NO NaN.  Scores are finite (a tuple with an infinite score is refused here; no scan produces one), so every C is a
// sum of at most 4096 finite scores minus non-negative penalties.  pen is +inf at worst (gap_ext * d overflowing), and
// then v = -inf, which is not taken.  C is never -0.0: (+0.0) + x and v + x with v > 0 give -0.0 for no x.
//
// COST.  Inside a segment the hits of one profile are ascending in off, hence in diag, so the predecessors of hit i in
// an earlier profile's run are one contiguous range of at most 2 max_shift + 1 entries found by bisection:
// O(hits x profiles present x (log + 2 max_shift + 1)).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "hs_pssm_family.h"
#include "hs_pssm_seq.h"
#include "hs_pssm_topk.h"

#define HS_PSSM_CHAIN_MAX_SHIFT 65535u /* the largest max_shift: a hit's cost is linear in it */

// max_shift, gap_open, gap_ext alone: refused when false.  (-0.0 passes and is read as +0.0 by hs_pssm_chain_pen.)
inline bool hs_pssm_chain_params_ok(uint32_t max_shift, double gap_open, double gap_ext) {
  if (max_shift > HS_PSSM_CHAIN_MAX_SHIFT) return false;
  if (gap_open != gap_open || gap_ext != gap_ext) return false;
  if (gap_open - gap_open != 0.0 || gap_ext - gap_ext != 0.0) return false;
  return !(gap_open < 0.0) && !(gap_ext < 0.0);
}

// a penalty as the rule reads it: -0.0 is +0.0
inline double hs_pssm_chain_zero(double x) { return x == 0.0 ? 0.0 : x; }

struct HsChainOut {
  uint32_t *group = nullptr, *seq = nullptr, *count = nullptr, *gaps = nullptr;
  double* score = nullptr;
  uint32_t *first_m = nullptr, *first_id = nullptr, *last_m = nullptr, *last_id = nullptr;
  int32_t* shift = nullptr;
  bool all() const {
    return group && seq && count && gaps && score && first_m && first_id && last_m && last_id && shift;
  }
  HsChainOut at(uint64_t i) const {
    return HsChainOut{group + i,    seq + i,    count + i,   gaps + i,  score + i,
                      first_m + i, first_id + i, last_m + i, last_id + i, shift + i};
  }
  // r rows in 44 r bytes of one buffer: the fp64 array, then the nine 32-bit ones
  static HsChainOut in(char* o, size_t r) {
    uint32_t* const w = reinterpret_cast<uint32_t*>(o + r * 8);
    return HsChainOut{w,         w + r,     w + 2 * r, w + 3 * r, reinterpret_cast<double*>(o),
                      w + 4 * r, w + 5 * r, w + 6 * r, w + 7 * r, reinterpret_cast<int32_t*>(w + 8 * r)};
  }
};

struct HsChainPath {
  uint64_t* start = nullptr;  // [n_out + 1]
  uint32_t *m = nullptr, *id = nullptr;
  uint64_t cap = 0;
  uint64_t* n_path = nullptr;
  bool any() const { return start || m || id; }
};

// Returns 0; 1 for an argument the contract refuses (nothing is written then); 2 when memory ran out; 3 when the
// reported rows exceed cap or the paths exceed path.cap (*n_out and *n_path are set, nothing else is written).
// -0.0 in a tuple is read as +0.0 (no scan produces it).
inline int hs_pssm_family_chain_hits_host(const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                          uint64_t nm, const uint32_t* m_group, uint64_t n_groups, const uint32_t* m_off,
                                          const uint64_t* id_start, uint64_t n_seq, uint32_t max_shift, double gap_open,
                                          double gap_ext, uint32_t min_count, const double* t_group,
                                          const HsChainOut& out, uint64_t cap, uint64_t* n_out,
                                          const HsChainPath& path) {
  if (!n_out) return 1;
  *n_out = 0;
  if (path.n_path) *path.n_path = 0;
  if (path.any() && (!path.n_path || !path.start || (path.cap && (!path.m || !path.id)))) return 1;
  if (n_tuples && (!m || !id || !score)) return 1;
  if (cap && !out.all()) return 1;
  if (nm && !m_off) return 1;
  if (!hs_pssm_chain_params_ok(max_shift, gap_open, gap_ext)) return 1;
  if (!hs_pssm_seq_id_start_ok(id_start, n_seq) || id_start[n_seq] > (1ull << 32)) return 1;
  if (!hs_pssm_family_counts_ok(nm, m_group != nullptr, n_groups, min_count)) return 1;
  uint64_t max_off = 0, max_len = 0;
  if (hs_pssm_family_values_bad(nm, m_group, n_groups, m_off, t_group, &max_off)) return 1;
  for (uint64_t s = 0; s < n_seq; ++s) max_len = std::max(max_len, id_start[s + 1] - id_start[s]);
  int wg, ws, wd;
  if (!hs_pssm_family_widths(n_groups, n_seq, max_len, max_off, &wg, &ws, &wd)) return 1;
  const double open = hs_pssm_chain_zero(gap_open), ext = hs_pssm_chain_zero(gap_ext);
  try {
    std::vector<uint64_t> live(n_tuples), key(n_tuples);
    for (uint64_t i = 0; i < n_tuples; ++i) {
      if (m[i] >= nm || id[i] >= id_start[n_seq]) return 1;
      if (score[i] != score[i] || score[i] - score[i] != 0.0) return 1;
      const double s = score[i] == 0.0 ? 0.0 : score[i];
      uint64_t bits;
      memcpy(&bits, &s, 8);
      key[i] = hs_pssm_desc_key(bits);
      live[i] = i;
    }
    // (m, id, key): a repeated (m, id) lands side by side
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
    // the distinct hits in (m, id) order, and a stable sort on (g, s): a segment's hits stay in (m, id), i.e. as runs
    // by profile with off ascending inside a run
    struct Hit {
      uint32_t g, s, off, m, id;
      int64_t diag;
      double score;
    };
    std::vector<Hit> hits(kept);
    for (size_t i = 0; i < kept; ++i) {
      const uint64_t j = live[i];
      Hit& h = hits[i];
      h.m = m[j];
      h.id = id[j];
      h.score = score[j] == 0.0 ? 0.0 : score[j];
      h.g = m_group ? m_group[h.m] : h.m;
      h.s = (uint32_t)(std::upper_bound(id_start, id_start + n_seq + 1, (uint64_t)h.id) - id_start - 1);
      h.off = (uint32_t)(h.id - id_start[h.s]);
      h.diag = (int64_t)h.off - (int64_t)m_off[h.m];
    }
    std::stable_sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) {
      if (a.g != b.g) return a.g < b.g;
      return a.s < b.s;
    });
    const size_t NONE = ~(size_t)0;
    std::vector<double> C(kept);
    std::vector<uint32_t> n(kept), gaps(kept);
    std::vector<size_t> first(kept), pred(kept), run;
    std::vector<size_t> ends;  // the reported rows' last hits
    for (size_t a = 0; a < kept;) {
      size_t b = a;
      run.clear();
      for (; b < kept && hits[b].g == hits[a].g && hits[b].s == hits[a].s; ++b)
        if (b == a || hits[b].m != hits[b - 1].m) run.push_back(b);
      run.push_back(b);
      size_t end = NONE;
      for (size_t r = 0; r + 1 < run.size(); ++r) {
        for (size_t i = run[r]; i < run[r + 1]; ++i) {
          const Hit& h = hits[i];
          double bv = 0.0;
          size_t bj = NONE;
          for (size_t q = 0; q < r; ++q) {
            const size_t qs = run[q], qe = run[q + 1];
            const int64_t moff = (int64_t)m_off[hits[qs].m];
            // off_j in [diag_i - max_shift + moff, diag_i + max_shift + moff] and below off_i
            const int64_t lo = std::max<int64_t>(0, h.diag - (int64_t)max_shift + moff);
            const int64_t hi = std::min<int64_t>((int64_t)h.off - 1, h.diag + (int64_t)max_shift + moff);
            if (hi < lo) continue;
            size_t x = qs, y = qe;
            while (x < y) {
              const size_t mid = x + (y - x) / 2;
              if ((int64_t)hits[mid].off < lo) x = mid + 1;
              else y = mid;
            }
            for (size_t j = x; j < qe && (int64_t)hits[j].off <= hi; ++j) {
              const int64_t dd = h.diag - hits[j].diag;
              const uint64_t d = (uint64_t)(dd < 0 ? -dd : dd);
              double v = C[j];
              if (d) {
                const double step = ext * (double)d;
                const double pen = open + step;
                v = C[j] - pen;
              }
              if (!(v > 0.0)) continue;
              // (v, n) descending, then m descending -- q ascends, so a later run wins a tie --, then id ascending
              if (bj == NONE || v > bv || (v == bv && (n[j] > n[bj] || (n[j] == n[bj] && hits[j].m > hits[bj].m))))
                bv = v, bj = j;
            }
          }
          pred[i] = bj;
          if (bj != NONE) {
            C[i] = bv + h.score;
            n[i] = n[bj] + 1;
            first[i] = first[bj];
            gaps[i] = gaps[bj] + (hits[bj].diag != h.diag ? 1u : 0u);
          } else {
            C[i] = 0.0 + h.score;
            n[i] = 1;
            first[i] = i;
            gaps[i] = 0;
          }
          if (n[i] < min_count || (t_group && !(C[i] >= t_group[h.g]))) continue;
          // (C, n) descending, then (m, id) ascending: i ascends, so the earlier hit keeps a tie
          if (end == NONE || C[i] > C[end] || (C[i] == C[end] && n[i] > n[end])) end = i;
        }
      }
      if (end != NONE) ends.push_back(end);
      a = b;
    }
    // everything is checked: the rows and the paths
    uint64_t n_path = 0;
    for (size_t e : ends) n_path += n[e];
    *n_out = ends.size();
    if (path.n_path) *path.n_path = n_path;
    if (ends.size() > cap || (path.any() && n_path > path.cap)) return 3;
    uint64_t at = 0;
    for (size_t i = 0; i < ends.size(); ++i) {
      const size_t e = ends[i], f = first[e];
      out.group[i] = hits[e].g;
      out.seq[i] = hits[e].s;
      out.count[i] = n[e];
      out.gaps[i] = gaps[e];
      out.score[i] = C[e];
      out.first_m[i] = hits[f].m;
      out.first_id[i] = hits[f].id;
      out.last_m[i] = hits[e].m;
      out.last_id[i] = hits[e].id;
      out.shift[i] = (int32_t)(hits[e].diag - hits[f].diag);
      if (path.any()) {
        path.start[i] = at;
        size_t j = e;
        for (uint32_t c = n[e]; c-- > 0; j = pred[j]) {
          path.m[at + c] = hits[j].m;
          path.id[at + c] = hits[j].id;
        }
        at += n[e];
      }
    }
    if (path.any()) path.start[ends.size()] = at;
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}
