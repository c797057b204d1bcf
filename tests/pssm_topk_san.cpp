// Stand-alone driver of hsearch_amd/csrc/hs_pssm_topk.h for the sanitizer run of tests/test_pssm_topk_cpu.py: the key
// transform over the doubles a score can be, and the host rule on tuple lists with ties, duplicates, padding and the
// refused inputs -- against a plain sort.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../hsearch_amd/csrc/hs_pssm_topk.h"

static uint64_t bits_of(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #c);           \
      return 1;                                               \
    }                                                         \
  } while (0)

int main() {
  std::mt19937_64 rng(11);
  // the transform: round trip and order, subnormals and both signs
  std::vector<double> v = {0.0, 4.9406564584124654e-324, -4.9406564584124654e-324, 2.2250738585072014e-308,
                           -2.2250738585072014e-308, 1.0, -1.0, 1.7976931348623157e308, -1.7976931348623157e308};
  for (int i = 0; i < 20000; ++i) {
    uint64_t b = rng();
    double d;
    memcpy(&d, &b, 8);
    if (d != d || isinf(d) || (d == 0.0 && signbit(d))) continue;
    v.push_back(d);
  }
  for (double d : v) {
    CHECK(hs_pssm_order_bits(hs_pssm_order_key(bits_of(d))) == bits_of(d));
    CHECK(hs_pssm_desc_bits(hs_pssm_desc_key(bits_of(d))) == bits_of(d));
    CHECK(hs_pssm_desc_key(bits_of(d)) != HS_PSSM_TOPK_PAD);
  }
  for (size_t i = 0; i + 1 < v.size(); ++i) {
    const double a = v[i], b = v[i + 1];
    CHECK((a < b) == (hs_pssm_order_key(bits_of(a)) < hs_pssm_order_key(bits_of(b))));
    CHECK((a > b) == (hs_pssm_desc_key(bits_of(a)) < hs_pssm_desc_key(bits_of(b))));
  }
  // the rule against a plain sort: small integer scores (heavy ties), duplicates, padding
  for (int round = 0; round < 50; ++round) {
    const uint64_t nm = 1 + rng() % 5;
    const uint32_t topk = 1 + (uint32_t)(rng() % 64);
    const size_t nt = rng() % 400;
    std::vector<uint32_t> m(nt), id(nt);
    std::vector<double> sc(nt);
    for (size_t i = 0; i < nt; ++i) {
      m[i] = (uint32_t)(rng() % nm);
      id[i] = (uint32_t)(rng() % 60);
      sc[i] = (double)((int)((id[i] * 7u + m[i] * 3u) % 5u) - 2);  // a function of (m, id): duplicates agree
      if (rng() % 16 == 0) id[i] = 0xffffffffu;
    }
    std::vector<uint32_t> tid(nm * topk, 5u), tc(nm, 5u);
    std::vector<double> ts(nm * topk, 5.0);
    CHECK(hs_pssm_topk_hits_host(m.data(), id.data(), sc.data(), nt, nm, topk, 64, tid.data(), ts.data(), tc.data()) == 0);
    for (uint64_t r = 0; r < nm; ++r) {
      std::vector<std::pair<double, uint32_t>> want;
      for (size_t i = 0; i < nt; ++i)
        if (m[i] == r && id[i] != 0xffffffffu) want.push_back({-sc[i], id[i]});
      std::sort(want.begin(), want.end());
      want.erase(std::unique(want.begin(), want.end()), want.end());
      const size_t c = std::min<size_t>(topk, want.size());
      CHECK(tc[r] == c);
      for (size_t j = 0; j < topk; ++j) {
        if (j < c) {
          CHECK(tid[r * topk + j] == want[j].second && ts[r * topk + j] == -want[j].first);
          CHECK(!signbit(ts[r * topk + j]) || ts[r * topk + j] != 0.0);
        } else {
          CHECK(tid[r * topk + j] == 0xffffffffu && ts[r * topk + j] == -INFINITY);
        }
      }
    }
  }
  // refusals: nothing is written
  {
    uint32_t m[3] = {0, 0, 1}, id[3] = {4, 4, 2}, tid[4] = {9, 9, 9, 9}, tc[2] = {9, 9};
    double sc[3] = {1.0, 2.0, 0.5}, ts[4] = {9, 9, 9, 9};
    CHECK(hs_pssm_topk_hits_host(m, id, sc, 3, 2, 2, 64, tid, ts, tc) == 1);   // two scores for (0, 4)
    sc[1] = 1.0;
    CHECK(hs_pssm_topk_hits_host(m, id, sc, 3, 2, 0, 64, tid, ts, tc) == 1);   // topk
    CHECK(hs_pssm_topk_hits_host(m, id, sc, 3, 2, 65, 64, tid, ts, tc) == 1);
    CHECK(hs_pssm_topk_hits_host(m, id, sc, 3, 1, 2, 64, tid, ts, tc) == 1);   // m >= nm
    CHECK(hs_pssm_topk_hits_host(m, id, sc, 3, 2, 2, 64, nullptr, ts, tc) == 1);
    sc[2] = NAN;
    CHECK(hs_pssm_topk_hits_host(m, id, sc, 3, 2, 2, 64, tid, ts, tc) == 1);
    for (int i = 0; i < 4; ++i) CHECK(tid[i] == 9 && ts[i] == 9.0);
    CHECK(tc[0] == 9 && tc[1] == 9);
    sc[2] = -0.0;
    CHECK(hs_pssm_topk_hits_host(m, id, sc, 3, 2, 2, 64, tid, ts, tc) == 0);
    CHECK(tc[0] == 1 && tc[1] == 1 && tid[0] == 4 && tid[1] == 0xffffffffu && tid[2] == 2 && !signbit(ts[2]));
    CHECK(hs_pssm_topk_hits_host(nullptr, nullptr, nullptr, 0, 0, 1, 64, nullptr, nullptr, nullptr) == 0);
  }
  printf("pssm_topk_san ok\n");
  return 0;
}
