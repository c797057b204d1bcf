// Stand-alone driver of hsearch_amd/csrc/hs_pssm_family.h for the sanitizer run of tests/test_pssm_family_cpu.py: the
// row rule on shuffled tuple lists with ties and repeats -- against a plain loop over (group, sequence, diagonal) slots
// --, the capacity protocol, the refused inputs on sentinel-filled outputs, and the layout rule on chains, an
// inconsistent triangle, a component of 4097 and the refused hits.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "../hsearch_amd/csrc/hs_pssm_family.h"

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #c);           \
      return 1;                                               \
    }                                                         \
  } while (0)

struct Rows {
  std::vector<uint32_t> group, seq, count, best_m, best_id, lo, hi;
  std::vector<int32_t> diag;
  std::vector<double> sum, best_score;
  explicit Rows(size_t cap)
      : group(cap, 9), seq(cap, 9), count(cap, 9), best_m(cap, 9), best_id(cap, 9), lo(cap, 9), hi(cap, 9),
        diag(cap, 9), sum(cap, 9.0), best_score(cap, 9.0) {}
  HsFamilyOut out() {
    return HsFamilyOut{group.data(), seq.data(),        diag.data(),   count.data(),   sum.data(),
                       best_score.data(), best_m.data(), best_id.data(), lo.data(), hi.data()};
  }
  bool untouched() const {
    for (size_t i = 0; i < group.size(); ++i)
      if (group[i] != 9 || seq[i] != 9 || diag[i] != 9 || count[i] != 9 || sum[i] != 9.0 || best_score[i] != 9.0 ||
          best_m[i] != 9 || best_id[i] != 9 || lo[i] != 9 || hi[i] != 9)
        return false;
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
  uint32_t min_count = 1;
  std::vector<double> t_group;
};

static int call(const Args& a, Rows& r, uint64_t cap, uint64_t* n_out) {
  return hs_pssm_family_hits_host(a.m.data(), a.id.data(), a.sc.data(), a.m.size(), a.nm,
                                  a.has_group ? a.m_group.data() : nullptr, a.n_groups,
                                  a.has_off ? a.m_off.data() : nullptr, a.id_start.data(), a.id_start.size() - 1,
                                  a.min_count, a.has_t ? a.t_group.data() : nullptr, r.out(), cap, n_out);
}

static int rows_rule() {
  std::mt19937_64 rng(31);
  const std::vector<std::vector<uint64_t>> layouts = {
      {0, 0, 0, 5, 5, 5, 12, 40, 40, 41, 60, 60, 60}, {0, 60}, {0, 1, 2, 3, 60}, {0, 0, 60, 60}};
  for (int round = 0; round < 80; ++round) {
    Args a;
    a.id_start = layouts[round % layouts.size()];
    const uint64_t n_seq = a.id_start.size() - 1, n = a.id_start[n_seq];
    a.nm = 1 + rng() % 7;
    a.has_group = round % 3 != 0;
    a.has_off = round % 2 == 0;
    a.m_group.resize(a.nm);
    a.m_off.resize(a.nm);
    uint32_t g = 0;
    for (uint64_t i = 0; i < a.nm; ++i) {
      if (i && rng() % 3 == 0) g += 1 + (uint32_t)(rng() % 2);  // (a group may stay empty)
      a.m_group[i] = g;
      a.m_off[i] = (uint32_t)(rng() % 9);
    }
    a.n_groups = a.has_group ? g + 1 : a.nm;
    a.min_count = 1 + (uint32_t)(rng() % 3);
    a.has_t = round % 4 == 1;
    a.t_group.assign(a.n_groups, 0.25);
    // a score per (m, id): small dyadic values with heavy ties; the tuples shuffled and with repeats
    std::vector<double> table(a.nm * n);
    for (double& v : table) v = (double)((int)(rng() % 13) - 6) / 4.0;
    const size_t nt = rng() % 400;
    for (size_t i = 0; i < nt; ++i) {
      a.m.push_back((uint32_t)(rng() % a.nm));
      a.id.push_back((uint32_t)(rng() % n));
      a.sc.push_back(table[a.m[i] * n + a.id[i]]);
    }
    // the plain loop: every distinct (m, id) in ascending order into its slot
    struct Slot {
      uint32_t count = 0, best_m = 0, best_id = 0, lo = 0, hi = 0;
      double sum = 0.0, best = 0.0;
    };
    std::map<std::tuple<uint32_t, uint32_t, int64_t>, Slot> slots;
    std::vector<char> present(a.nm * n, 0);
    for (size_t i = 0; i < nt; ++i) present[a.m[i] * n + a.id[i]] = 1;
    for (uint64_t m = 0; m < a.nm; ++m)
      for (uint64_t id = 0; id < n; ++id) {
        if (!present[m * n + id]) continue;
        uint32_t s = 0;
        for (uint64_t q = 0; q < n_seq; ++q)
          if (a.id_start[q] <= id) s = (uint32_t)q;
        const uint32_t off = (uint32_t)(id - a.id_start[s]);
        const int64_t diag = a.has_off ? (int64_t)off - (int64_t)a.m_off[m] : 0;
        Slot& sl = slots[std::make_tuple(a.has_group ? a.m_group[m] : (uint32_t)m, s, diag)];
        const double sc = table[m * n + id];
        if (!sl.count || sc > sl.best) {
          sl.best = sc;
          sl.best_m = (uint32_t)m;
          sl.best_id = (uint32_t)id;
        }
        sl.lo = sl.count ? std::min(sl.lo, off) : off;
        sl.hi = sl.count ? std::max(sl.hi, off) : off;
        sl.sum = sl.sum + sc;
        ++sl.count;
      }
    Rows r(nt + 1);
    uint64_t n_out = 77;
    CHECK(call(a, r, nt + 1, &n_out) == 0);
    size_t at = 0;
    for (const auto& kv : slots) {
      const Slot& sl = kv.second;
      if (sl.count < a.min_count || (a.has_t && !(sl.sum >= 0.25))) continue;
      CHECK(at < n_out);
      CHECK(r.group[at] == std::get<0>(kv.first) && r.seq[at] == std::get<1>(kv.first));
      CHECK(r.diag[at] == (int32_t)std::get<2>(kv.first) && r.count[at] == sl.count);
      CHECK(memcmp(&r.sum[at], &sl.sum, 8) == 0 && memcmp(&r.best_score[at], &sl.best, 8) == 0);
      CHECK(r.best_m[at] == sl.best_m && r.best_id[at] == sl.best_id && r.lo[at] == sl.lo && r.hi[at] == sl.hi);
      ++at;
    }
    CHECK(at == n_out && r.group[n_out] == 9);
    // the capacity protocol: the count with no arrays, then one row short
    uint64_t need = 0;
    const int st = hs_pssm_family_hits_host(a.m.data(), a.id.data(), a.sc.data(), nt, a.nm,
                                            a.has_group ? a.m_group.data() : nullptr, a.n_groups,
                                            a.has_off ? a.m_off.data() : nullptr, a.id_start.data(), n_seq, a.min_count,
                                            a.has_t ? a.t_group.data() : nullptr, HsFamilyOut(), 0, &need);
    CHECK(need == n_out && st == (n_out ? 3 : 0));
    if (n_out) {
      Rows small(n_out - 1);
      CHECK(call(a, small, n_out - 1, &need) == 3 && need == n_out && small.untouched());
    }
  }
  return 0;
}

static int rows_refusals() {
  Args a;
  a.m = {0, 0, 1};
  a.id = {4, 4, 2};
  a.sc = {1.0, 1.0, 0.5};
  a.nm = 2;
  a.m_group = {0, 0};
  a.m_off = {0, 1};
  a.n_groups = 1;
  a.id_start = {0, 3, 10};
  a.t_group = {0.0};
  Rows r(4);
  uint64_t n_out = 5;
  CHECK(call(a, r, 4, &n_out) == 0 && n_out == 2);
  Rows s(4);
  Args b = a;
  b.sc[1] = 2.0;  // two scores for (0, 4)
  CHECK(call(b, s, 4, &n_out) == 1 && n_out == 0);
  b = a;
  b.sc[2] = NAN;
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.nm = 1;
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.id_start = {0, 3, 4};  // an id at id_start[n_seq]
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.id_start = {1, 3, 10};
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.id_start = {0, 11, 10};
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.m_group = {1, 0};  // decreasing
  b.n_groups = 2;
  b.t_group = {0.0, 0.0};
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.m_group = {0, 1};  // a value >= n_groups
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.has_group = false;  // n_groups != nm without m_group
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.min_count = 0;
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.has_t = true;
  b.t_group = {NAN};
  CHECK(call(b, s, 4, &n_out) == 1);
  b.t_group = {-INFINITY};
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.m_off = {0, 0x80000000u};
  CHECK(call(b, s, 4, &n_out) == 1);
  b = a;
  b.n_groups = (1ull << 32) + 1;
  CHECK(call(b, s, 4, &n_out) == 1);
  {  // a null output with cap > 0
    HsFamilyOut o = s.out();
    o.sum = nullptr;
    CHECK(hs_pssm_family_hits_host(a.m.data(), a.id.data(), a.sc.data(), 3, 2, a.m_group.data(), 1, a.m_off.data(),
                                   a.id_start.data(), 2, 1, nullptr, o, 4, &n_out) == 1);
    CHECK(hs_pssm_family_hits_host(a.m.data(), a.id.data(), a.sc.data(), 3, 2, a.m_group.data(), 1, a.m_off.data(),
                                   a.id_start.data(), 2, 1, nullptr, s.out(), 4, nullptr) == 1);
  }
  CHECK(s.untouched());
  {  // a group of 4097 profiles; 4096 pass
    Args c;
    c.nm = 4097;
    c.m_group.assign(4097, 0);
    c.m_off.assign(4097, 0);
    c.n_groups = 1;
    c.id_start = {0, 10};
    CHECK(call(c, s, 4, &n_out) == 1 && s.untouched());
    c.nm = 4096;
    c.m_group.resize(4096);
    c.m_off.resize(4096);
    CHECK(call(c, s, 4, &n_out) == 0 && n_out == 0);
  }
  {  // the width rule: 2^32 groups x 2^32 sequences leave no bit for a diagonal of two values
    int wg, ws, wd;
    CHECK(hs_pssm_family_widths(1ull << 32, 1ull << 32, 1, 0, &wg, &ws, &wd) && wg == 32 && ws == 32 && wd == 0);
    CHECK(!hs_pssm_family_widths(1ull << 32, 1ull << 32, 2, 0, &wg, &ws, &wd));
    CHECK(hs_pssm_family_widths(1, 1, 0, 0, &wg, &ws, &wd) && wg + ws + wd == 0);
  }
  return 0;
}

static int layout_rule() {
  uint64_t ng = 77, nc = 77;
  {  // a chain of windows at shifts 0, 3, 6, 9 as a spanning set given backwards, two families and a loner
    const std::vector<uint32_t> x = {2, 1, 0, 5}, y = {3, 2, 1, 4};
    const std::vector<int32_t> d = {3, 3, 3, -2};
    std::vector<uint32_t> g(7, 9), off(7, 9), order(7, 9);
    CHECK(hs_pssm_family_layout_host(x.data(), y.data(), d.data(), 4, 7, g.data(), off.data(), order.data(), &ng,
                                     &nc) == 0);
    CHECK(ng == 3 && nc == 0);
    const uint32_t want_g[7] = {0, 0, 0, 0, 1, 1, 2}, want_off[7] = {0, 3, 6, 9, 0, 2, 0};
    const uint32_t want_order[7] = {0, 1, 2, 3, 4, 5, 6};
    for (int i = 0; i < 7; ++i) CHECK(g[i] == want_g[i] && off[i] == want_off[i] && order[i] == want_order[i]);
  }
  {  // an inconsistent triangle: the third hit only counts
    const std::vector<uint32_t> x = {0, 1, 0}, y = {1, 2, 2};
    const std::vector<int32_t> d = {3, 3, 7};
    std::vector<uint32_t> g(3, 9), off(3, 9), order(3, 9);
    CHECK(hs_pssm_family_layout_host(x.data(), y.data(), d.data(), 3, 3, g.data(), off.data(), order.data(), &ng,
                                     &nc) == 0);
    CHECK(ng == 1 && nc == 1 && off[0] == 0 && off[1] == 3 && off[2] == 6);
  }
  {  // refusals write nothing
    std::vector<uint32_t> g(3, 9), off(3, 9), order(3, 9);
    ng = nc = 77;
    const auto refused = [&](std::vector<uint32_t> x, std::vector<uint32_t> y, std::vector<int32_t> d) {
      const int st = hs_pssm_family_layout_host(x.data(), y.data(), d.data(), x.size(), 3, g.data(), off.data(),
                                                order.data(), &ng, &nc);
      for (int i = 0; i < 3; ++i)
        if (g[i] != 9 || off[i] != 9 || order[i] != 9) return false;
      return st == 1 && ng == 77 && nc == 77;
    };
    CHECK(refused({0, 1}, {1, 1}, {1, 1}));
    CHECK(refused({0, 3}, {1, 1}, {1, 1}));
    CHECK(refused({0, 1}, {1, 2}, {1, 1 << 30}));
    CHECK(refused({0, 1}, {1, 2}, {-(1 << 30), 1}));
    CHECK(refused({0, 1}, {1, 2}, {(1 << 30) - 1, (1 << 30) - 1}) == false);  // spans 2^31 - 2: passes
    for (int i = 0; i < 3; ++i) g[i] = off[i] = order[i] = 9;
    ng = nc = 77;
    CHECK(refused({0, 1, 0}, {1, 2, 1}, {(1 << 30) - 1, (1 << 30) - 1, 0}) == false);
  }
  {  // an offset that passes 2^31 - 1: three steps of 2^30 - 1 do not, a fourth one does
    const int32_t big = (1 << 30) - 1;
    std::vector<uint32_t> x = {0, 1, 2}, y = {1, 2, 3};
    std::vector<int32_t> d = {big, big, 5};
    std::vector<uint32_t> g(4, 9), off(4, 9), order(4, 9);
    ng = nc = 77;
    CHECK(hs_pssm_family_layout_host(x.data(), y.data(), d.data(), 3, 4, g.data(), off.data(), order.data(), &ng,
                                     &nc) == 1);
    CHECK(g[0] == 9 && off[3] == 9 && ng == 77);
    d[2] = 1;
    CHECK(hs_pssm_family_layout_host(x.data(), y.data(), d.data(), 3, 4, g.data(), off.data(), order.data(), &ng,
                                     &nc) == 0);
    CHECK(off[3] == 0x7fffffffu);
  }
  {  // a component of 4097 is refused, one of 4096 passes; long chains exercise the path compression
    const uint32_t n = 4097;
    std::vector<uint32_t> x(n - 1), y(n - 1), g(n, 9), off(n, 9), order(n, 9);
    std::vector<int32_t> d(n - 1, 1);
    for (uint32_t i = 0; i + 1 < n; ++i) {
      x[i] = i + 1;  // x > y
      y[i] = i;
      d[i] = -1;
    }
    ng = 77;
    CHECK(hs_pssm_family_layout_host(x.data(), y.data(), d.data(), n - 1, n, g.data(), off.data(), order.data(), &ng,
                                     &nc) == 1);
    CHECK(g[0] == 9 && order[n - 1] == 9 && ng == 77);
    CHECK(hs_pssm_family_layout_host(x.data(), y.data(), d.data(), n - 2, n, g.data(), off.data(), order.data(), &ng,
                                     &nc) == 0);
    CHECK(ng == 2 && nc == 0 && g[n - 1] == 1 && off[n - 1] == 0);
    for (uint32_t i = 0; i + 1 < n; ++i) CHECK(g[i] == 0 && off[i] == i && order[i] == i);
  }
  CHECK(hs_pssm_family_layout_host(nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, &ng, &nc) == 0 && ng == 0);
  return 0;
}

int main() {
  if (rows_rule() || rows_refusals() || layout_rule()) return 1;
  printf("pssm_family_san ok\n");
  return 0;
}
