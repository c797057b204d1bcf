// pssm_rank_san.cpp -- hs_pssm_rank.h under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program
// (tests/test_pssm_rank_cpu.py compiles and runs it).  The host rule against a plain sort, the sample rule at its
// edges, and every refusal on sentinel-filled outputs.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "../hsearch_amd/csrc/hs_pssm_rank.h"

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      return 1;                                               \
    }                                                         \
  } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static int one_shape(uint32_t k, uint32_t A, uint64_t n, uint64_t nm, bool coarse) {
  std::vector<uint8_t> codes(n * k);
  for (auto& c : codes) c = (uint8_t)(rnd() % A);
  std::vector<double> S(nm * k * A);
  for (auto& v : S) v = coarse ? (double)((int)(rnd() % 3) - 1) : (double)((int)(rnd() % 129) - 64) / 8.0;
  if (nm > 1)
    for (uint32_t p = 0; p < k; ++p) S[(1 * k + p) * A + 0] = -1e30;  // a forbidden residue
  std::vector<uint64_t> rank(nm), ge(nm), gt(nm);
  std::vector<double> t(nm);
  for (uint64_t m = 0; m < nm; ++m) rank[m] = m == 0 ? 1 : m == 1 ? n : 1 + rnd() % n;
  CHECK(hs_pssm_rank_scores_host(codes.data(), n, k, A, S.data(), nm, rank.data(), t.data(), ge.data(), gt.data()) == 0);
  for (uint64_t m = 0; m < nm; ++m) {
    std::vector<double> sc(n);
    for (uint64_t i = 0; i < n; ++i) {
      double s = 0.0;
      for (uint32_t p = 0; p < k; ++p) s = s + S[(m * k + p) * A + codes[i * k + p]];
      sc[i] = s;
    }
    std::sort(sc.begin(), sc.end(), std::greater<double>());
    const double want = sc[rank[m] - 1];
    uint64_t wge = 0, wgt = 0;
    for (uint64_t i = 0; i < n; ++i) {
      wge += sc[i] >= want;
      wgt += sc[i] > want;
    }
    CHECK(memcmp(&want, &t[m], 8) == 0);
    CHECK(ge[m] == wge && gt[m] == wgt && wgt < rank[m] && rank[m] <= wge);
  }
  return 0;
}

int main() {
  if (one_shape(25, 20, 500, 5, false)) return 1;
  if (one_shape(3, 4, 200, 7, true)) return 1;   // ties fill every rank
  if (one_shape(75, 32, 65, 3, false)) return 1;
  if (one_shape(1, 1, 1, 2, false)) return 1;

  // the key transform round-trips and orders
  const double vals[] = {-1e300, -2.5, -4.9e-324, 0.0, 4.9e-324, 1.0, 3e200};
  uint64_t prev = 0;
  for (size_t i = 0; i < sizeof(vals) / sizeof(vals[0]); ++i) {
    uint64_t bits;
    memcpy(&bits, &vals[i], 8);
    const uint64_t key = hs_pssm_desc_key(bits);
    CHECK(hs_pssm_desc_bits(key) == bits);
    CHECK(i == 0 || key < prev);  // ascending values: descending keys
    prev = key;
  }

  // the sample rule
  uint64_t r = 99;
  CHECK(hs_pssm_rank_plan_rule(65, 5000, 64, 0, &r) == 0 && r == 13);
  CHECK(hs_pssm_rank_plan_rule(65, 5000, 64, 1, &r) == 0 && r == 49);
  CHECK(hs_pssm_rank_plan_rule(65, 5000, 64, 2, &r) == 0 && r == 65);
  CHECK(hs_pssm_rank_plan_rule(100, 5000, 64, 0, &r) == 0 && r == 18);
  CHECK(hs_pssm_rank_plan_rule(100, 5000, 64, 1, &r) == 0 && r == 65);
  CHECK(hs_pssm_rank_plan_rule(777, 5000, 5000, 5, &r) == 0 && r == 777);
  CHECK(hs_pssm_rank_plan_rule(1, 5000, 1, 0, &r) == 0 && r == 2);
  for (uint32_t round = 0; round < 40; ++round) {
    CHECK(hs_pssm_rank_plan_rule(0xfffffffeull, 0xffffffffull, 0xfffffffeull, round, &r) == 0);
    CHECK(r >= 1 && r <= 0xffffffffull);
  }
  CHECK(hs_pssm_rank_isqrt_up(0) == 0 && hs_pssm_rank_isqrt_up(1) == 1 && hs_pssm_rank_isqrt_up(2) == 2 &&
        hs_pssm_rank_isqrt_up(16) == 4 && hs_pssm_rank_isqrt_up(17) == 5 &&
        hs_pssm_rank_isqrt_up(0xffffffffull) == 65536);
  r = 99;
  CHECK(hs_pssm_rank_plan_rule(0, 10, 5, 0, &r) == 1 && hs_pssm_rank_plan_rule(11, 10, 5, 0, &r) == 1);
  CHECK(hs_pssm_rank_plan_rule(1, 10, 0, 0, &r) == 1 && hs_pssm_rank_plan_rule(1, 10, 11, 0, &r) == 1);
  CHECK(hs_pssm_rank_plan_rule(1, 1ull << 32, 5, 0, &r) == 1 && hs_pssm_rank_plan_rule(1, 10, 5, 0, nullptr) == 1);
  CHECK(r == 99);

  // refusals write nothing
  const uint32_t k = 3, A = 4;
  const uint64_t n = 10, nm = 2;
  std::vector<uint8_t> codes(n * k, 1);
  std::vector<double> S(nm * k * A, 0.5);
  uint64_t rank[2] = {1, 10}, ge[2] = {9, 9}, gt[2] = {9, 9};
  double t[2] = {9.0, 9.0};
  auto call = [&](const uint8_t* c, uint64_t nn, uint32_t kk, uint32_t AA, const double* SS, uint64_t m,
                  const uint64_t* rk, double* tt, uint64_t* g1, uint64_t* g2) {
    return hs_pssm_rank_scores_host(c, nn, kk, AA, SS, m, rk, tt, g1, g2);
  };
  CHECK(call(codes.data(), n, 0, A, S.data(), nm, rank, t, ge, gt) == 1);
  CHECK(call(codes.data(), n, k, 0, S.data(), nm, rank, t, ge, gt) == 1);
  CHECK(call(codes.data(), n, k, 33, S.data(), nm, rank, t, ge, gt) == 1);
  CHECK(call(nullptr, n, k, A, S.data(), nm, rank, t, ge, gt) == 1);
  CHECK(call(codes.data(), n, k, A, nullptr, nm, rank, t, ge, gt) == 1);
  CHECK(call(codes.data(), n, k, A, S.data(), nm, nullptr, t, ge, gt) == 1);
  CHECK(call(codes.data(), n, k, A, S.data(), nm, rank, nullptr, ge, gt) == 1);
  CHECK(call(codes.data(), n, k, A, S.data(), nm, rank, t, nullptr, gt) == 1);
  CHECK(call(codes.data(), n, k, A, S.data(), nm, rank, t, ge, nullptr) == 1);
  CHECK(call(codes.data(), n, k, A, S.data(), 1ull << 27, rank, t, ge, gt) == 1);
  CHECK(call(codes.data(), 0, k, A, S.data(), nm, rank, t, ge, gt) == 1);  // an empty index refuses every rank
  {
    uint64_t bad[2] = {0, 10};
    CHECK(call(codes.data(), n, k, A, S.data(), nm, bad, t, ge, gt) == 1);
    bad[0] = 1;
    bad[1] = 11;
    CHECK(call(codes.data(), n, k, A, S.data(), nm, bad, t, ge, gt) == 1);
    std::vector<double> S2 = S;
    const double nan = strtod("nan", nullptr), inf = strtod("inf", nullptr);
    S2[5] = nan;
    CHECK(call(codes.data(), n, k, A, S2.data(), nm, rank, t, ge, gt) == 1);
    S2[5] = -inf;
    CHECK(call(codes.data(), n, k, A, S2.data(), nm, rank, t, ge, gt) == 1);
    S2[5] = 2.6e30;
    CHECK(call(codes.data(), n, k, A, S2.data(), nm, rank, t, ge, gt) == 1);
    std::vector<uint8_t> c2 = codes;
    c2[17] = (uint8_t)A;
    CHECK(call(c2.data(), n, k, A, S.data(), nm, rank, t, ge, gt) == 1);
  }
  CHECK(t[0] == 9.0 && t[1] == 9.0 && ge[0] == 9 && ge[1] == 9 && gt[0] == 9 && gt[1] == 9);
  CHECK(call(codes.data(), n, k, A, S.data(), 0, nullptr, nullptr, nullptr, nullptr) == 0);  // nm == 0
  CHECK(call(codes.data(), n, k, A, S.data(), nm, rank, t, ge, gt) == 0);
  CHECK(t[0] == 1.5 && t[1] == 1.5 && ge[0] == 10 && ge[1] == 10 && gt[0] == 0 && gt[1] == 0);
  printf("pssm_rank_san ok\n");
  return 0;
}
