// hs_pssm_family.h -- the rules of hs_pssm_family_scan (include/hsearch.h) on the host: the reduction of any list of
// (m, id, score) tuples to rows per (family, sequence, diagonal) (hs_pssm_family_hits), the layout that turns
// hs_pssm_compare's self-mode hits into families (hs_pssm_family_layout), and the argument checks both forms of the
// scan share.  Host-compilable: nothing here needs hipcc.
//
// THE ROW RULE.  A hit (m, id) has the key (g, s, diag): g = m_group[m] (m itself without m_group), s = the LAST s with
// id_start[s] <= id (hs_pssm_seq.h), off = id - id_start[s], diag = off - m_off[m] (0 without m_off).  One row per
// distinct key, ascending in (g, s, diag as a signed number).  A row's hits are taken in ascending (m, id):
//   count   how many
//   sum     ((+0.0 + score_1) + score_2) + ...: every partial sum rounded to fp64, in that order
//   best    the first hit under (score descending, m ascending, id ascending): hs_pssm_topk.h's key transform
//   lo, hi  the smallest and the largest off
// A row is reported iff count >= min_count and (t_group == NULL or sum >= t_group[g]).
//
// THE LAYOUT RULE.  Hits (x, y, d) say: column p of profile y meets column p + d of profile x, so y lies d to the right
// of x: pos[y] - pos[x] = d.  They are taken in the given order through a union-find that carries every profile's
// position relative to its root.  A hit between two components joins them at that distance; a hit inside one component
// that disagrees with the positions already fixed is counted in n_conflicts and changes nothing.  The result depends
// on the order of the hits; hs_pssm_compare's (x, y) ascending order makes it canonical.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "hs_pssm_seq.h"
#include "hs_pssm_topk.h"

#define HS_PSSM_FAMILY_MAX_GROUP 4096u       /* profiles per group: the scan's default batch */
#define HS_PSSM_FAMILY_MAX_OFF 0x7fffffffull /* the largest m_off */

// bits of BAD in hs_pssm_family_values_bad (the device check kernel of hs_pssm_family.hip sets the same ones)
enum {
  HS_FAM_BAD_GROUP_ORDER = 1,  // m_group decreases
  HS_FAM_BAD_GROUP_VALUE = 2,  // a value >= n_groups
  HS_FAM_BAD_GROUP_SIZE = 4,   // a group above HS_PSSM_FAMILY_MAX_GROUP profiles
  HS_FAM_BAD_OFF = 8,          // an m_off above 2^31 - 1
  HS_FAM_BAD_T_GROUP = 16,     // a t_group entry NaN or infinite
  HS_FAM_BAD_OFF_ORDER = 32    // an m_off below its predecessor's inside one group: refused by hs_pssm_family_chain
                               // (hs_pssm_chain.h) only; the family scan takes any order
};

inline int hs_pssm_family_bits(uint64_t x) {
  int b = 0;
  while (x) {
    ++b;
    x >>= 1;
  }
  return b;
}

// The width rule (hs_seq_match's): bits(n_groups - 1) + bits(n_seq - 1) + bits(max_len + max_off - 1) <= 64
inline bool hs_pssm_family_widths(uint64_t n_groups, uint64_t n_seq, uint64_t max_len, uint64_t max_off, int* wg,
                                  int* ws, int* wd) {
  *wg = hs_pssm_family_bits(n_groups ? n_groups - 1 : 0);
  *ws = hs_pssm_family_bits(n_seq ? n_seq - 1 : 0);
  *wd = max_len + max_off ? hs_pssm_family_bits(max_len + max_off - 1) : 0;
  return *wg + *ws + *wd <= 64;
}

// what the arguments alone refuse (no array is read)
inline bool hs_pssm_family_counts_ok(uint64_t nm, bool has_group, uint64_t n_groups, uint32_t min_count) {
  if (n_groups > (1ull << 32) || min_count < 1) return false;
  return has_group || n_groups == nm;
}

// m_group [nm], m_off [nm], t_group [n_groups] (each may be null) on the host: the HS_FAM_BAD_* bits, and the
// largest m_off
inline uint32_t hs_pssm_family_values_bad(uint64_t nm, const uint32_t* m_group, uint64_t n_groups, const uint32_t* m_off,
                                          const double* t_group, uint64_t* max_off) {
  uint32_t bad = 0;
  *max_off = 0;
  for (uint64_t m = 0; m_group && m < nm; ++m) {
    if (m && m_group[m] < m_group[m - 1]) bad |= HS_FAM_BAD_GROUP_ORDER;
    if (m_group[m] >= n_groups) bad |= HS_FAM_BAD_GROUP_VALUE;
    if (m >= HS_PSSM_FAMILY_MAX_GROUP && m_group[m] == m_group[m - HS_PSSM_FAMILY_MAX_GROUP])
      bad |= HS_FAM_BAD_GROUP_SIZE;  // (with a non-decreasing m_group: 4097 profiles of one group)
  }
  for (uint64_t m = 0; m_off && m < nm; ++m) {
    if (m_off[m] > HS_PSSM_FAMILY_MAX_OFF) bad |= HS_FAM_BAD_OFF;
    if (m_group && m && m_group[m] == m_group[m - 1] && m_off[m] < m_off[m - 1]) bad |= HS_FAM_BAD_OFF_ORDER;
    *max_off = std::max<uint64_t>(*max_off, m_off[m]);
  }
  for (uint64_t g = 0; t_group && g < n_groups; ++g)
    if (t_group[g] != t_group[g] || t_group[g] - t_group[g] != 0.0) bad |= HS_FAM_BAD_T_GROUP;
  return bad;
}

struct HsFamilyOut {
  uint32_t *group = nullptr, *seq = nullptr;
  int32_t* diag = nullptr;
  uint32_t* count = nullptr;
  double *sum = nullptr, *best_score = nullptr;
  uint32_t *best_m = nullptr, *best_id = nullptr, *lo = nullptr, *hi = nullptr;
  bool all() const { return group && seq && diag && count && sum && best_score && best_m && best_id && lo && hi; }
  HsFamilyOut at(uint64_t i) const {
    return HsFamilyOut{group + i, seq + i,     diag + i,    count + i, sum + i,
                       best_score + i, best_m + i, best_id + i, lo + i,    hi + i};
  }
  // r rows in 48 r bytes of one buffer: the two fp64 arrays, then the eight 32-bit ones
  static HsFamilyOut in(char* o, size_t r) {
    double* const f = reinterpret_cast<double*>(o);
    uint32_t* const w = reinterpret_cast<uint32_t*>(o + r * 16);
    return HsFamilyOut{w,     w + r,     reinterpret_cast<int32_t*>(w + 2 * r), w + 3 * r, f, f + r, w + 4 * r,
                       w + 5 * r, w + 6 * r, w + 7 * r};
  }
};

// Returns 0; 1 for an argument the contract refuses (nothing is written then); 2 when memory ran out; 3 when the
// reported rows exceed cap (*n_out is set, no row is written).  -0.0 in a tuple is read as +0.0 (no scan produces it).
inline int hs_pssm_family_hits_host(const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                    uint64_t nm, const uint32_t* m_group, uint64_t n_groups, const uint32_t* m_off,
                                    const uint64_t* id_start, uint64_t n_seq, uint32_t min_count, const double* t_group,
                                    const HsFamilyOut& out, uint64_t cap, uint64_t* n_out) {
  if (!n_out) return 1;
  *n_out = 0;
  if (n_tuples && (!m || !id || !score)) return 1;
  if (cap && !out.all()) return 1;
  if (!hs_pssm_seq_id_start_ok(id_start, n_seq) || id_start[n_seq] > (1ull << 32)) return 1;
  if (!hs_pssm_family_counts_ok(nm, m_group != nullptr, n_groups, min_count)) return 1;
  uint64_t max_off = 0, max_len = 0;
  if (hs_pssm_family_values_bad(nm, m_group, n_groups, m_off, t_group, &max_off) & ~(uint32_t)HS_FAM_BAD_OFF_ORDER)
    return 1;
  for (uint64_t s = 0; s < n_seq; ++s) max_len = std::max(max_len, id_start[s + 1] - id_start[s]);
  int wg, ws, wd;
  if (!hs_pssm_family_widths(n_groups, n_seq, max_len, max_off, &wg, &ws, &wd)) return 1;
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
    // the distinct hits in (m, id) order, their row keys, and a stable sort on those: a row's hits stay in (m, id)
    struct Hit {
      uint32_t g, s, off, m, id;
      int64_t diag;
      uint64_t key;
    };
    std::vector<Hit> hits(kept);
    for (size_t i = 0; i < kept; ++i) {
      const uint64_t j = live[i];
      Hit& h = hits[i];
      h.m = m[j];
      h.id = id[j];
      h.key = key[j];
      h.g = m_group ? m_group[h.m] : h.m;
      h.s = (uint32_t)(std::upper_bound(id_start, id_start + n_seq + 1, (uint64_t)h.id) - id_start - 1);
      h.off = (uint32_t)(h.id - id_start[h.s]);
      h.diag = m_off ? (int64_t)h.off - (int64_t)m_off[h.m] : 0;
    }
    std::stable_sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) {
      if (a.g != b.g) return a.g < b.g;
      if (a.s != b.s) return a.s < b.s;
      return a.diag < b.diag;
    });
    struct Row {
      uint32_t g, s, count, best_m, best_id, lo, hi;
      int64_t diag;
      uint64_t key;
      double sum;
    };
    std::vector<Row> rows;
    for (size_t i = 0; i < kept;) {
      const Hit& f = hits[i];
      Row r{f.g, f.s, 0u, f.m, f.id, f.off, f.off, f.diag, f.key, 0.0};
      for (; i < kept && hits[i].g == r.g && hits[i].s == r.s && hits[i].diag == r.diag; ++i) {
        const Hit& h = hits[i];
        const uint64_t bits = hs_pssm_desc_bits(h.key);
        double sc;
        memcpy(&sc, &bits, 8);
        ++r.count;
        r.sum = r.sum + sc;
        r.lo = std::min(r.lo, h.off);
        r.hi = std::max(r.hi, h.off);
        if (h.key < r.key) {  // (strictly better: an equal score keeps the earlier (m, id))
          r.key = h.key;
          r.best_m = h.m;
          r.best_id = h.id;
        }
      }
      if (r.count >= min_count && (!t_group || r.sum >= t_group[r.g])) rows.push_back(r);
    }
    // everything is checked: the rows
    *n_out = rows.size();
    if (rows.size() > cap) return 3;
    for (size_t i = 0; i < rows.size(); ++i) {
      const uint64_t bits = hs_pssm_desc_bits(rows[i].key);
      out.group[i] = rows[i].g;
      out.seq[i] = rows[i].s;
      out.diag[i] = (int32_t)(uint32_t)(uint64_t)rows[i].diag;
      out.count[i] = rows[i].count;
      out.sum[i] = rows[i].sum;
      memcpy(&out.best_score[i], &bits, 8);
      out.best_m[i] = rows[i].best_m;
      out.best_id[i] = rows[i].best_id;
      out.lo[i] = rows[i].lo;
      out.hi[i] = rows[i].hi;
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}

// Returns 0; 1 for an argument the contract refuses (nothing is written then); 2 when memory ran out.
inline int hs_pssm_family_layout_host(const uint32_t* hit_x, const uint32_t* hit_y, const int32_t* hit_d,
                                      uint64_t n_hits, uint64_t nm, uint32_t* out_group, uint32_t* out_off,
                                      uint32_t* out_order, uint64_t* n_groups, uint64_t* n_conflicts) {
  if (!n_groups || !n_conflicts) return 1;
  if (n_hits && (!hit_x || !hit_y || !hit_d)) return 1;
  if (nm > (1ull << 32) || (nm && (!out_group || !out_off || !out_order))) return 1;
  for (uint64_t i = 0; i < n_hits; ++i) {
    if (hit_x[i] == hit_y[i] || hit_x[i] >= nm || hit_y[i] >= nm) return 1;
    if (hit_d[i] >= (1 << 30) || hit_d[i] <= -(1 << 30)) return 1;
  }
  try {
    // rel[v] = pos[v] - pos[parent[v]]; a root has rel 0
    std::vector<uint32_t> parent(nm), size(nm, 1u);
    std::vector<int64_t> rel(nm, 0);
    for (uint64_t v = 0; v < nm; ++v) parent[v] = (uint32_t)v;
    // the root of v and pos[v] - pos[root]; the path is then hung on the root
    auto find = [&](uint32_t v, int64_t* pos) -> uint32_t {
      uint32_t r = v;
      int64_t p = 0;
      while (parent[r] != r) {
        p += rel[r];
        r = parent[r];
      }
      *pos = p;
      while (parent[v] != r && v != r) {
        const uint32_t up = parent[v];
        const int64_t step = rel[v];
        parent[v] = r;
        rel[v] = p;
        p -= step;
        v = up;
      }
      return r;
    };
    uint64_t conflicts = 0;
    for (uint64_t i = 0; i < n_hits; ++i) {
      int64_t px, py;
      const uint32_t rx = find(hit_x[i], &px), ry = find(hit_y[i], &py);
      if (rx == ry) {
        if (py - px != (int64_t)hit_d[i]) ++conflicts;
        continue;
      }
      if ((uint64_t)size[rx] + size[ry] > HS_PSSM_FAMILY_MAX_GROUP) return 1;
      // pos[y] - pos[x] = d: the smaller tree goes under the larger one's root
      if (size[rx] >= size[ry]) {
        parent[ry] = rx;
        rel[ry] = px + hit_d[i] - py;
        size[rx] += size[ry];
      } else {
        parent[rx] = ry;
        rel[rx] = py - hit_d[i] - px;
        size[ry] += size[rx];
      }
    }
    // components numbered by their smallest member; positions from the component's minimum
    std::vector<uint32_t> group_of_root(nm, 0xffffffffu), group(nm);
    std::vector<int64_t> pos(nm), low;
    uint64_t groups = 0;
    for (uint64_t v = 0; v < nm; ++v) {
      const uint32_t r = find((uint32_t)v, &pos[v]);
      if (group_of_root[r] == 0xffffffffu) {
        group_of_root[r] = (uint32_t)groups++;
        low.push_back(pos[v]);
      }
      group[v] = group_of_root[r];
      low[group[v]] = std::min(low[group[v]], pos[v]);
    }
    for (uint64_t v = 0; v < nm; ++v)
      if (pos[v] - low[group[v]] > (int64_t)HS_PSSM_FAMILY_MAX_OFF) return 1;
    // everything is checked
    std::vector<uint32_t> order(nm);
    for (uint64_t v = 0; v < nm; ++v) {
      out_group[v] = group[v];
      out_off[v] = (uint32_t)(pos[v] - low[group[v]]);
      order[v] = (uint32_t)v;
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      if (out_group[a] != out_group[b]) return out_group[a] < out_group[b];
      if (out_off[a] != out_off[b]) return out_off[a] < out_off[b];
      return a < b;
    });
    for (uint64_t v = 0; v < nm; ++v) out_order[v] = order[v];
    *n_groups = groups;
    *n_conflicts = conflicts;
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}
