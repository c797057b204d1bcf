// Stand-alone driver of hsearch_amd/csrc/hs_pssm_chain.h for the sanitizer run of tests/test_pssm_chain_cpu.py: the
// chain rule on shuffled tuple lists with ties and repeats -- against a plain quadratic loop over every pair of a
// segment's hits --, the paths, the capacity protocol for rows and paths, and the refused inputs on sentinel-filled
// outputs.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "../hsearch_amd/csrc/hs_pssm_chain.h"

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #c);           \
      return 1;                                               \
    }                                                         \
  } while (0)

struct Rows {
  std::vector<uint32_t> group, seq, count, gaps, first_m, first_id, last_m, last_id;
  std::vector<int32_t> shift;
  std::vector<double> score;
  std::vector<uint64_t> pstart;
  std::vector<uint32_t> pm, pid;
  uint64_t n_path = 77;
  Rows(size_t cap, size_t path_cap)
      : group(cap, 9), seq(cap, 9), count(cap, 9), gaps(cap, 9), first_m(cap, 9), first_id(cap, 9), last_m(cap, 9),
        last_id(cap, 9), shift(cap, 9), score(cap, 9.0), pstart(cap + 1, 9), pm(path_cap, 9), pid(path_cap, 9) {}
  HsChainOut out() {
    return HsChainOut{group.data(),   seq.data(),      count.data(),  gaps.data(),    score.data(),
                      first_m.data(), first_id.data(), last_m.data(), last_id.data(), shift.data()};
  }
  HsChainPath path(bool want) {
    HsChainPath p;
    if (want) {
      p.start = pstart.data();
      p.m = pm.data();
      p.id = pid.data();
      p.cap = pm.size();
      p.n_path = &n_path;
    }
    return p;
  }
  bool untouched() const {
    for (size_t i = 0; i < group.size(); ++i)
      if (group[i] != 9 || seq[i] != 9 || count[i] != 9 || gaps[i] != 9 || score[i] != 9.0 || first_m[i] != 9 ||
          first_id[i] != 9 || last_m[i] != 9 || last_id[i] != 9 || shift[i] != 9)
        return false;
    for (uint64_t v : pstart)
      if (v != 9) return false;
    for (size_t i = 0; i < pm.size(); ++i)
      if (pm[i] != 9 || pid[i] != 9) return false;
    return true;
  }
};

struct Args {
  std::vector<uint32_t> m, id;
  std::vector<double> sc;
  uint64_t nm = 0;
  std::vector<uint32_t> m_group, m_off;
  bool has_group = true, has_off = true, has_t = false;
  uint64_t n_groups = 0;
  std::vector<uint64_t> id_start;
  uint32_t max_shift = 0, min_count = 1;
  double gap_open = 0.0, gap_ext = 0.0;
  std::vector<double> t_group;
};

static int call(const Args& a, Rows& r, uint64_t cap, uint64_t* n_out, bool want_path) {
  return hs_pssm_family_chain_hits_host(a.m.data(), a.id.data(), a.sc.data(), a.m.size(), a.nm,
                                        a.has_group ? a.m_group.data() : nullptr, a.n_groups,
                                        a.has_off ? a.m_off.data() : nullptr, a.id_start.data(), a.id_start.size() - 1,
                                        a.max_shift, a.gap_open, a.gap_ext, a.min_count,
                                        a.has_t ? a.t_group.data() : nullptr, r.out(), cap, n_out, r.path(want_path));
}

struct Hit {
  uint32_t m, id, off, n, gaps;
  int64_t diag;
  double score, C;
  int first, pred;
};

static int chain_rule() {
  std::mt19937_64 rng(37);
  const std::vector<std::vector<uint64_t>> layouts = {
      {0, 0, 0, 5, 5, 5, 12, 40, 40, 41, 60, 60, 60}, {0, 60}, {0, 1, 2, 3, 60}, {0, 0, 60, 60}};
  const double pens[3][2] = {{0.0, 0.0}, {1.0, 0.25}, {0.1, 1.0 / 1048576.0}};
  const uint32_t shifts[4] = {0, 1, 3, 65535};
  uint64_t gapped = 0, long_chains = 0;
  for (int round = 0; round < 120; ++round) {
    Args a;
    a.id_start = layouts[round % layouts.size()];
    const uint64_t n_seq = a.id_start.size() - 1, n = a.id_start[n_seq];
    a.nm = 1 + rng() % 9;
    a.has_group = round % 3 != 0;
    a.m_group.resize(a.nm);
    a.m_off.resize(a.nm);
    uint32_t g = 0;
    for (uint64_t i = 0; i < a.nm; ++i) {
      const bool next = i && rng() % 4 == 0;
      if (next) g += 1 + (uint32_t)(rng() % 2);  // (a group may stay empty)
      a.m_group[i] = g;
      // not decreasing inside a group (without m_group every profile is its own group)
      a.m_off[i] = (i && !next && a.has_group ? a.m_off[i - 1] : 0) + (uint32_t)(rng() % 4);
    }
    a.n_groups = a.has_group ? g + 1 : a.nm;
    a.min_count = 1 + (uint32_t)(rng() % 3);
    a.has_t = round % 4 == 1;
    a.t_group.assign(a.n_groups, 0.75);
    a.max_shift = shifts[rng() % 4];
    a.gap_open = pens[round % 3][0];
    a.gap_ext = pens[round % 3][1];
    // a score per (m, id): small dyadic values with heavy ties; the tuples shuffled and with repeats
    std::vector<double> table(a.nm * n);
    for (double& v : table) v = (double)((int)(rng() % 13) - 4) / 4.0;
    const size_t nt = rng() % 500;
    for (size_t i = 0; i < nt; ++i) {
      a.m.push_back((uint32_t)(rng() % a.nm));
      a.id.push_back((uint32_t)(rng() % n));
      a.sc.push_back(table[a.m[i] * n + a.id[i]]);
    }
    // the plain loop: every distinct (m, id) in ascending order into its segment, then every pair
    std::map<std::pair<uint32_t, uint32_t>, std::vector<Hit>> segs;
    std::vector<char> present(a.nm * n, 0);
    for (size_t i = 0; i < nt; ++i) present[a.m[i] * n + a.id[i]] = 1;
    for (uint64_t m = 0; m < a.nm; ++m)
      for (uint64_t id = 0; id < n; ++id) {
        if (!present[m * n + id]) continue;
        uint32_t s = 0;
        for (uint64_t q = 0; q < n_seq; ++q)
          if (a.id_start[q] <= id) s = (uint32_t)q;
        Hit h{};
        h.m = (uint32_t)m;
        h.id = (uint32_t)id;
        h.off = (uint32_t)(id - a.id_start[s]);
        h.diag = (int64_t)h.off - (int64_t)a.m_off[m];
        h.score = table[m * n + id] == 0.0 ? 0.0 : table[m * n + id];
        segs[{a.has_group ? a.m_group[m] : (uint32_t)m, s}].push_back(h);
      }
    struct Want {
      uint32_t g, s;
      Hit end, first;
      std::vector<std::pair<uint32_t, uint32_t>> path;
    };
    std::vector<Want> want;
    for (auto& kv : segs) {
      std::vector<Hit>& hs = kv.second;
      int end = -1;
      for (int i = 0; i < (int)hs.size(); ++i) {
        Hit& h = hs[i];
        int bj = -1;
        double bv = 0.0;
        for (int j = 0; j < i; ++j) {
          const Hit& p = hs[j];
          const int64_t dd = h.diag - p.diag;
          const uint64_t d = (uint64_t)(dd < 0 ? -dd : dd);
          if (!(p.m < h.m && p.off < h.off && d <= a.max_shift)) continue;
          double v = p.C;
          if (d) {
            const double step = a.gap_ext * (double)d;
            v = p.C - (a.gap_open + step);
          }
          bool better = bj < 0 || v > bv;
          if (bj >= 0 && v == bv) {
            const Hit& b = hs[bj];
            better = p.n > b.n || (p.n == b.n && (p.m > b.m || (p.m == b.m && p.id < b.id)));
          }
          if (better) bv = v, bj = j;
        }
        if (bj >= 0 && bv > 0.0) {
          h.C = bv + h.score;
          h.n = hs[bj].n + 1;
          h.first = hs[bj].first;
          h.gaps = hs[bj].gaps + (hs[bj].diag != h.diag);
          h.pred = bj;
        } else {
          h.C = 0.0 + h.score;
          h.n = 1;
          h.first = i;
          h.gaps = 0;
          h.pred = -1;
        }
        if (h.n < a.min_count || (a.has_t && !(h.C >= a.t_group[kv.first.first]))) continue;
        if (end < 0 || h.C > hs[end].C || (h.C == hs[end].C && h.n > hs[end].n)) end = i;
      }
      if (end < 0) continue;
      Want w{kv.first.first, kv.first.second, hs[end], hs[hs[end].first], {}};
      for (int j = end; j >= 0; j = hs[j].pred) w.path.push_back({hs[j].m, hs[j].id});
      std::reverse(w.path.begin(), w.path.end());
      gapped += hs[end].gaps;
      long_chains += hs[end].n > 2;
      want.push_back(w);
    }
    Rows r(nt + 1, nt + 1);
    uint64_t n_out = 77;
    CHECK(call(a, r, nt + 1, &n_out, true) == 0);
    CHECK(n_out == want.size());
    uint64_t at = 0;
    for (size_t i = 0; i < want.size(); ++i) {
      const Want& w = want[i];
      CHECK(r.group[i] == w.g && r.seq[i] == w.s && r.count[i] == w.end.n && r.gaps[i] == w.end.gaps);
      CHECK(memcmp(&r.score[i], &w.end.C, 8) == 0);
      CHECK(r.first_m[i] == w.first.m && r.first_id[i] == w.first.id && r.last_m[i] == w.end.m && r.last_id[i] == w.end.id);
      CHECK(r.shift[i] == (int32_t)(w.end.diag - w.first.diag));
      CHECK(r.pstart[i] == at && w.path.size() == w.end.n);
      for (size_t c = 0; c < w.path.size(); ++c, ++at) CHECK(r.pm[at] == w.path[c].first && r.pid[at] == w.path[c].second);
    }
    CHECK(r.pstart[want.size()] == at && r.n_path == at);
    // without the path the same rows; the capacity protocol for both
    Rows r2(nt + 1, 0);
    CHECK(call(a, r2, nt + 1, &n_out, false) == 0 && n_out == want.size());
    CHECK(r2.score == r.score && r2.count == r.count && r2.last_id == r.last_id && r2.n_path == 77);
    if (!want.empty()) {
      Rows small(want.size() - 1, at);
      CHECK(call(a, small, want.size() - 1, &n_out, true) == 3 && n_out == want.size() && small.n_path == at);
      CHECK(small.untouched());
      Rows narrow(want.size(), at - 1);
      CHECK(call(a, narrow, want.size(), &n_out, true) == 3 && n_out == want.size() && narrow.n_path == at);
      CHECK(narrow.untouched());
      Rows exact(want.size(), at);
      CHECK(call(a, exact, want.size(), &n_out, true) == 0 && exact.pm == std::vector<uint32_t>(r.pm.begin(), r.pm.begin() + at));
    }
  }
  CHECK(gapped > 50 && long_chains > 50);
  return 0;
}

static int refusals() {
  Args good;
  good.m = {0, 0, 1};
  good.id = {4, 4, 6};
  good.sc = {1.0, 1.0, 0.5};
  good.nm = 2;
  good.m_group = {0, 0};
  good.m_off = {0, 1};
  good.n_groups = 1;
  good.id_start = {0, 3, 10};
  good.max_shift = 2;
  uint64_t n_out = 5;
  {
    Rows r(4, 4);
    CHECK(call(good, r, 4, &n_out, true) == 0 && n_out == 1 && r.count[0] == 2 && r.gaps[0] == 1 && r.score[0] == 1.5);
    CHECK(r.shift[0] == 1 && r.n_path == 2 && r.pid[0] == 4 && r.pid[1] == 6);
  }
  std::vector<Args> bad;
  Args a = good;
  a.has_off = false;  // m_off is required
  bad.push_back(a);
  a = good;
  a.m_off = {1, 0};  // decreases inside a group
  bad.push_back(a);
  a = good;
  a.max_shift = 65536;
  bad.push_back(a);
  for (double x : {(double)NAN, (double)INFINITY, -(double)INFINITY, -1.0, -5e-324}) {
    a = good;
    a.gap_open = x;
    bad.push_back(a);
    a = good;
    a.gap_ext = x;
    bad.push_back(a);
  }
  a = good;
  a.min_count = 0;
  bad.push_back(a);
  a = good;
  a.sc = {1.0, 2.0, 0.5};  // two scores for (0, 4)
  bad.push_back(a);
  a = good;
  a.sc = {1.0, 1.0, (double)NAN};
  bad.push_back(a);
  a = good;
  a.sc = {1.0, 1.0, (double)INFINITY};
  bad.push_back(a);
  a = good;
  a.id_start = {0, 3, 6};  // an id at id_start[n_seq]
  bad.push_back(a);
  a = good;
  a.id_start = {0, 11, 10};
  bad.push_back(a);
  a = good;
  a.m_group = {1, 0};
  a.m_off = {0, 0};
  a.n_groups = 2;
  bad.push_back(a);
  a = good;
  a.n_groups = 0;  // a value >= n_groups
  bad.push_back(a);
  a = good;
  a.has_group = false;  // n_groups != nm without m_group
  bad.push_back(a);
  a = good;
  a.has_t = true;
  a.t_group = {(double)NAN};
  bad.push_back(a);
  a = good;
  a.m_off = {0, 1u << 31};
  bad.push_back(a);
  for (const Args& b : bad) {
    Rows r(4, 4);
    n_out = 5;
    CHECK(call(b, r, 4, &n_out, true) == 1 && n_out == 0 && r.n_path == 0 && r.untouched());
  }
  // ... but an offset may fall across a group boundary, and -0.0 is +0.0 everywhere
  a = good;
  a.m_off = {1, 0};
  a.m_group = {0, 1};
  a.n_groups = 2;
  a.gap_open = -0.0;
  a.gap_ext = -0.0;
  a.sc = {1.0, 1.0, -0.0};
  Rows r(4, 4);
  CHECK(call(a, r, 4, &n_out, false) == 0 && n_out == 2 && r.score[1] == 0.0 && !signbit(r.score[1]));
  // a path array missing, a null n_out
  Rows q(4, 4);
  HsChainPath p = q.path(true);
  p.id = nullptr;
  CHECK(hs_pssm_family_chain_hits_host(good.m.data(), good.id.data(), good.sc.data(), 3, 2, good.m_group.data(), 1,
                                       good.m_off.data(), good.id_start.data(), 2, 2, 0.0, 0.0, 1, nullptr, q.out(), 4,
                                       &n_out, p) == 1);
  CHECK(hs_pssm_family_chain_hits_host(good.m.data(), good.id.data(), good.sc.data(), 3, 2, good.m_group.data(), 1,
                                       good.m_off.data(), good.id_start.data(), 2, 2, 0.0, 0.0, 1, nullptr, q.out(), 4,
                                       nullptr, HsChainPath()) == 1);
  CHECK(q.untouched());
  // nothing at all
  Args none;
  none.id_start = {0};
  none.has_group = none.has_off = false;
  Rows e(1, 1);
  CHECK(call(none, e, 0, &n_out, false) == 0 && n_out == 0);
  return 0;
}

int main() {
  if (chain_rule()) return 1;
  if (refusals()) return 1;
  printf("pssm_chain_san ok\n");
  return 0;
}
