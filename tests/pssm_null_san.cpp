// pssm_null_san.cpp -- hs_pssm_null.h under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program
// (tests/test_pssm_null_cpu.py compiles and runs it).  The tables at both ends of the bin range and at shapes that are
// no multiple of a block, the bracket against a brute-force enumeration, the threshold's two properties, the extreme
// inputs (a forbidden residue, entries at +-2^100, infinite hit scores, a dead profile), and every refusal on
// sentinel-filled outputs.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../hsearch_amd/csrc/hs_pssm_null.h"

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

static int one_shape(uint32_t k, uint32_t A, uint32_t B, uint64_t nm, int kind) {
  std::vector<double> S(nm * k * A), bg(A), t_lo(nm);
  for (auto& v : S) v = (double)((int)(rnd() % 257) - 128) / 16.0;
  double sum = 0;
  for (auto& v : bg) sum += v = (double)(1 + rnd() % 100);
  for (auto& v : bg) v /= sum * 1.0000001;
  if (kind == 1)
    for (uint32_t p = 1; p < k; ++p) S[p * A] = -1e30;  // a forbidden residue in profile 0
  if (kind == 2) {
    S[0] = 1.2676506002282294e30;
    S[A - 1] = -1.2676506002282294e30;
  }
  for (uint64_t m = 0; m < nm; ++m) t_lo[m] = m == 1 ? 1e9 : m == 2 ? -1e6 : -3.0;  // profile 1 is dead
  std::vector<uint16_t> qd(nm * k * A), qu(nm * k * A);
  std::vector<double> delta(nm), cd(nm * B), cu(nm * B);
  std::vector<uint8_t> dead(nm);
  CHECK(hs_pssm_null_tables_host(S.data(), nm, k, A, bg.data(), t_lo.data(), B, qd.data(), qu.data(), delta.data(),
                                 dead.data(), cd.data(), cu.data()) == 0);
  for (uint64_t m = 0; m < nm; ++m) {
    CHECK(dead[m] == (m == 1 ? 1 : 0) && delta[m] > 0.0);
    for (uint32_t j = 0; j < B; ++j) {
      CHECK(cd[m * B + j] >= 0.0 && cu[m * B + j] >= 0.0 && cd[m * B + j] <= 1.0 && cu[m * B + j] <= cd[m * B + j] * 1.000001);
      CHECK(j == 0 || (cd[m * B + j] >= cd[m * B + j - 1] && cu[m * B + j] >= cu[m * B + j - 1]));
    }
    for (size_t i = 0; i < (size_t)k * A; ++i) CHECK(qd[m * k * A + i] <= B && qu[m * k * A + i] <= B && qd[m * k * A + i] <= qu[m * k * A + i]);
  }
  // hits in any order, at the extremes
  const double inf = strtod("inf", nullptr);
  std::vector<uint32_t> hm;
  std::vector<double> hs;
  for (uint64_t m = nm; m-- > 0;)
    for (double s : {-inf, -1.7e308, -1e31, -3.0, 0.0, 1.0, 7.5, 1e9, 1.3e30, 1.7e308, inf}) {
      hm.push_back((uint32_t)m);
      hs.push_back(s);
    }
  std::vector<double> hi(hm.size(), 9.0), lo(hm.size(), 9.0), hi1(hm.size(), 9.0);
  CHECK(hs_pssm_pvalue_host_rule(S.data(), nm, k, A, bg.data(), t_lo.data(), B, hm.data(), hs.data(), hm.size(),
                                 hi.data(), lo.data()) == 0);
  CHECK(hs_pssm_pvalue_host_rule(S.data(), nm, k, A, bg.data(), t_lo.data(), B, hm.data(), hs.data(), hm.size(),
                                 hi1.data(), nullptr) == 0);
  for (size_t i = 0; i < hm.size(); ++i) {
    CHECK(lo[i] >= 0.0 && lo[i] <= hi[i] && hi[i] <= 1.0 && hi[i] == hi1[i]);
    if (hs[i] == inf || hs[i] == 1.7e308) CHECK(hi[i] == 0.0);
    if (hs[i] == -inf) CHECK(hi[i] == 1.0);
    if (hm[i] == 1 && hs[i] >= 1e9) CHECK(hi[i] == 0.0);
  }
  // thresholds: admissible, and the next double below is not
  std::vector<double> p(nm), tp(nm), th(nm), tl(nm);
  std::vector<uint32_t> fl(nm);
  for (double pv : {1.0, 0.3, 1e-2, 1e-4, 1e-12, 1e-300}) {
    for (auto& v : p) v = pv;
    CHECK(hs_pssm_threshold_host_rule(S.data(), nm, k, A, bg.data(), t_lo.data(), B, p.data(), tp.data(), th.data(),
                                      tl.data(), fl.data()) == 0);
    for (uint64_t m = 0; m < nm; ++m) {
      CHECK(fl[m] <= 2 && th[m] <= pv && tl[m] <= th[m]);
      if (fl[m] == 2) CHECK(tp[m] == 1.7976931348623157e308 && th[m] == 0.0);
      if (fl[m] == 1) CHECK(tp[m] == t_lo[m]);
      if (fl[m] == 0) {
        const uint32_t one = (uint32_t)m;
        const double below = nextafter(tp[m], -inf);
        double h2 = 9.0;
        CHECK(hs_pssm_pvalue_host_rule(S.data(), nm, k, A, bg.data(), t_lo.data(), B, &one, &below, 1, &h2, nullptr) == 0);
        CHECK(h2 > pv);
      }
    }
  }
  return 0;
}

// the bracket against every k-mer (k = 3, alphabet 4; long double sums with a relative slack far inside the margins)
static int brute(uint32_t B) {
  const uint32_t k = 3, A = 4;
  std::vector<double> S(k * A), bg = {0.1, 0.2, 0.3, 0.39};
  for (auto& v : S) v = (double)((int)(rnd() % 257) - 128) / 16.0;
  const double t_lo = -30.0;
  for (int i = -200; i <= 200; ++i) {
    const double t = (double)i / 8.0 + 1.0 / 32.0;  // off every attainable score: no tie at t
    long double P = 0;
    for (uint32_t x = 0; x < 64; ++x) {
      const uint32_t c[3] = {x & 3u, (x >> 2) & 3u, x >> 4};
      double s = 0.0;
      long double w = 1;
      for (uint32_t pp = 0; pp < k; ++pp) {
        s = s + S[pp * A + c[pp]];
        w *= bg[c[pp]];
      }
      if (s >= t) P += w;
    }
    const uint32_t m = 0;
    double hi = 9, lo = 9;
    CHECK(hs_pssm_pvalue_host_rule(S.data(), 1, k, A, bg.data(), &t_lo, B, &m, &t, 1, &hi, &lo) == 0);
    CHECK((long double)lo <= P * (1 + 1e-15L) && P * (1 - 1e-15L) <= (long double)hi);
  }
  return 0;
}

int main() {
  if (one_shape(1, 20, 64, 3, 0)) return 1;
  if (one_shape(3, 4, 64, 3, 0)) return 1;
  if (one_shape(3, 4, 100, 4, 1)) return 1;    // 100 bins: a partial last block of the cumulative sum
  if (one_shape(25, 20, 257, 3, 1)) return 1;
  if (one_shape(25, 20, 4096, 3, 2)) return 1;
  if (one_shape(75, 32, 8192, 3, 0)) return 1;
  if (one_shape(7, 1, 65, 3, 0)) return 1;     // one letter: one k-mer
  if (brute(64) || brute(100) || brute(4096)) return 1;

  // refusals write nothing
  const uint32_t k = 3, A = 4, B = 64;
  const uint64_t nm = 2;
  std::vector<double> S(nm * k * A, 0.5), bg(A, 0.25), t_lo(nm, 0.0), p(nm, 0.5);
  std::vector<uint16_t> q(nm * k * A, 9);
  std::vector<double> d(nm, 9.0), c(nm * B, 9.0), o(nm, 9.0);
  std::vector<uint8_t> dead(nm, 9);
  std::vector<uint32_t> fl(nm, 9);
  const uint32_t hm[2] = {0, 1}, hm_bad[2] = {0, 2};
  const double hs[2] = {1.0, 2.0}, nan = strtod("nan", nullptr), hs_bad[2] = {1.0, nan};
  auto tab = [&](const double* SS, uint64_t m, uint32_t kk, uint32_t AA, const double* b, const double* tl, uint32_t bins) {
    return hs_pssm_null_tables_host(SS, m, kk, AA, b, tl, bins, q.data(), q.data(), d.data(), dead.data(), c.data(), c.data());
  };
  CHECK(tab(S.data(), nm, 0, A, bg.data(), t_lo.data(), B) == 1 && tab(S.data(), nm, 76, A, bg.data(), t_lo.data(), B) == 1);
  CHECK(tab(S.data(), nm, k, 0, bg.data(), t_lo.data(), B) == 1 && tab(S.data(), nm, k, 33, bg.data(), t_lo.data(), B) == 1);
  CHECK(tab(S.data(), nm, k, A, bg.data(), t_lo.data(), 63) == 1 && tab(S.data(), nm, k, A, bg.data(), t_lo.data(), 8193) == 1);
  CHECK(tab(nullptr, nm, k, A, bg.data(), t_lo.data(), B) == 1 && tab(S.data(), nm, k, A, nullptr, t_lo.data(), B) == 1);
  CHECK(tab(S.data(), 1ull << 27, k, A, bg.data(), t_lo.data(), B) == 1);
  {
    std::vector<double> S2 = S, b2 = bg, t2 = t_lo;
    S2[5] = nan;
    CHECK(tab(S2.data(), nm, k, A, bg.data(), t_lo.data(), B) == 1);
    S2[5] = 2.6e30;
    CHECK(tab(S2.data(), nm, k, A, bg.data(), t_lo.data(), B) == 1);
    b2[1] = -0.1;
    CHECK(tab(S.data(), nm, k, A, b2.data(), t_lo.data(), B) == 1);
    b2[1] = 1.5;
    CHECK(tab(S.data(), nm, k, A, b2.data(), t_lo.data(), B) == 1);
    b2[1] = nan;
    CHECK(tab(S.data(), nm, k, A, b2.data(), t_lo.data(), B) == 1);
    b2.assign(A, 0.0);
    CHECK(tab(S.data(), nm, k, A, b2.data(), t_lo.data(), B) == 1);
    t2[1] = strtod("inf", nullptr);
    CHECK(tab(S.data(), nm, k, A, bg.data(), t2.data(), B) == 1);
  }
  CHECK(hs_pssm_pvalue_host_rule(S.data(), nm, k, A, bg.data(), nullptr, B, hm_bad, hs, 2, o.data(), o.data()) == 1);
  CHECK(hs_pssm_pvalue_host_rule(S.data(), nm, k, A, bg.data(), nullptr, B, hm, hs_bad, 2, o.data(), o.data()) == 1);
  CHECK(hs_pssm_pvalue_host_rule(S.data(), nm, k, A, bg.data(), nullptr, B, nullptr, hs, 2, o.data(), o.data()) == 1);
  CHECK(hs_pssm_pvalue_host_rule(S.data(), nm, k, A, bg.data(), nullptr, B, hm, hs, 2, nullptr, o.data()) == 1);
  for (double bad : {0.0, -1.0, 1.5, nan}) {
    std::vector<double> p2 = p;
    p2[1] = bad;
    CHECK(hs_pssm_threshold_host_rule(S.data(), nm, k, A, bg.data(), nullptr, B, p2.data(), o.data(), o.data(), o.data(), fl.data()) == 1);
  }
  CHECK(hs_pssm_threshold_host_rule(S.data(), nm, k, A, bg.data(), nullptr, B, nullptr, o.data(), o.data(), o.data(), fl.data()) == 1);
  CHECK(hs_pssm_threshold_host_rule(S.data(), nm, k, A, bg.data(), nullptr, B, p.data(), o.data(), o.data(), o.data(), nullptr) == 1);
  for (auto v : q) CHECK(v == 9);
  for (auto v : c) CHECK(v == 9.0);
  CHECK(d[0] == 9.0 && d[1] == 9.0 && o[0] == 9.0 && o[1] == 9.0 && dead[0] == 9 && fl[0] == 9 && fl[1] == 9);
  // nothing to do
  CHECK(hs_pssm_null_tables_host(nullptr, 0, k, A, nullptr, nullptr, B, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(hs_pssm_pvalue_host_rule(S.data(), nm, k, A, bg.data(), nullptr, B, nullptr, nullptr, 0, nullptr, nullptr) == 0);
  // every output optional
  CHECK(hs_pssm_null_tables_host(S.data(), nm, k, A, bg.data(), nullptr, B, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  printf("pssm_null_san ok\n");
  return 0;
}
