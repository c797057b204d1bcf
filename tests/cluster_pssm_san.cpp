// Stand-alone driver of hsearch_amd/csrc/hs_cluster_pssm.h for the sanitizer run of tests/test_cluster_pssm_cpu.py: both
// host rules on random label arrays (noise, clusters below min_size, one cluster of everything, singletons) in every
// shape against hs_pssm_weight_hits_host over the (row, member) tuples and a plain loop over the members, the column
// sums, planted ties of the minimum, extreme profiles, and the refused inputs -- with arrays of exactly the needed size.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../hsearch_amd/csrc/hs_cluster_pssm.h"

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #c);           \
      return 1;                                               \
    }                                                         \
  } while (0)

int main() {
  std::mt19937_64 rng(91);
  const uint32_t shapes[][2] = {{1, 20}, {25, 20}, {26, 20}, {4, 32}, {75, 32}};
  for (int round = 0; round < 40; ++round) {
    const uint32_t k = shapes[round % 5][0], A = shapes[round % 5][1];
    const uint64_t n = 1 + rng() % 150;
    const uint32_t min_size = 1 + (uint32_t)(rng() % 4);
    const size_t cells = (size_t)k * A;
    std::vector<uint8_t> codes(n * k);
    for (auto& c : codes) c = (uint8_t)(rng() % (round % 3 ? A : 3));
    std::vector<uint32_t> label(n);
    const int kind = round % 4;  // mixed with noise, one cluster, singletons, all noise
    for (uint64_t i = 0; i < n; ++i)
      label[i] = kind == 0 ? (rng() % 5 == 0 ? HS_CP_NOISE : (uint32_t)(rng() % (n / 6 + 1)))
                           : kind == 1 ? (uint32_t)(n - 1) : kind == 2 ? (uint32_t)((i * 7 + 3) % n) : HS_CP_NOISE;
    uint64_t rows = 77;
    CHECK(hs_cluster_weights_codes_host(codes.data(), n, k, A, label.data(), min_size, nullptr, nullptr, nullptr,
                                        nullptr, nullptr, nullptr, 0, &rows) == (rows ? 3 : 0));
    CHECK(rows <= n / min_size);
    std::vector<uint32_t> ol(rows, 9), osz(rows, 9), counts(rows * cells, 9), distinct(rows, 9);
    std::vector<uint64_t> wc(rows * cells, 9), wsum(rows, 9);
    uint64_t again = 0;
    const uint64_t cap = rows ? rows : 0;
    CHECK(hs_cluster_weights_codes_host(codes.data(), n, k, A, label.data(), min_size, ol.data(), osz.data(),
                                        counts.data(), wc.data(), wsum.data(), distinct.data(), cap, &again) == 0);
    CHECK(again == rows);
    // the rows, and the tuples (row, member)
    std::vector<uint32_t> tm, ti;
    for (uint64_t r = 0; r < rows; ++r) {
      CHECK(r == 0 || ol[r] > ol[r - 1]);
      uint32_t size = 0;
      for (uint64_t i = 0; i < n; ++i)
        if (label[i] == ol[r]) {
          ++size;
          tm.push_back((uint32_t)r);
          ti.push_back((uint32_t)i);
        }
      CHECK(size == osz[r] && size >= min_size);
    }
    std::vector<double> sc(tm.size(), 0.0);
    std::vector<uint32_t> c2(rows * cells, 7), d2(rows, 7);
    std::vector<uint64_t> w2(rows * cells, 7), s2(rows, 7), used(rows, 7);
    CHECK(hs_pssm_weight_hits_host(codes.data(), n, k, A, tm.data(), ti.data(), sc.data(), tm.size(), rows, nullptr, 0,
                                   c2.data(), w2.data(), s2.data(), d2.data(), used.data()) == 0);
    CHECK(c2 == counts && w2 == wc && s2 == wsum && d2 == distinct);
    for (uint64_t r = 0; r < rows; ++r) {
      CHECK(used[r] == osz[r] && wsum[r] <= ((uint64_t)k << 56));
      for (uint32_t p = 0; p < k; ++p) {
        uint64_t sum = 0;
        for (uint32_t a = 0; a < A; ++a) sum += wc[r * cells + (size_t)p * A + a];
        CHECK(sum == wsum[r]);
      }
    }
    // every optional output left out
    std::vector<uint64_t> bare(rows * cells, 9);
    CHECK(hs_cluster_weights_codes_host(codes.data(), n, k, A, label.data(), min_size, ol.data(), osz.data(), nullptr,
                                        bare.data(), nullptr, nullptr, cap, &again) == 0);
    CHECK(bare == wc);
    // the cover: coarse profiles (ties), every third round with extreme entries
    std::vector<double> S(rows * cells), ms(rows, 9.0);
    std::vector<uint32_t> am(rows, 9);
    for (auto& v : S) v = (double)((int)(rng() % 7) - 3) / 2.0;
    if (round % 3 == 0)
      for (size_t e = 0; e < S.size(); e += 5) S[e] = e % 2 ? -1e30 : (e % 3 ? ldexp(1.0, 100) : -ldexp(1.0, 100));
    CHECK(hs_cluster_cover_codes_host(codes.data(), n, k, A, label.data(), min_size, S.data(), rows, ms.data(),
                                      am.data()) == 0);
    for (uint64_t r = 0; r < rows; ++r) {
      bool any = false;
      double best = 0;
      uint32_t at = 0;
      for (uint64_t i = 0; i < n; ++i) {
        if (label[i] != ol[r]) continue;
        double s = 0.0;
        for (uint32_t p = 0; p < k; ++p) s = s + S[r * cells + (size_t)p * A + codes[i * k + p]];
        CHECK(!isnan(s) && !(s == 0.0 && signbit(s)));
        if (!any || s < best) {
          best = s;
          at = (uint32_t)i;
          any = true;
        }
      }
      CHECK(any && memcmp(&best, &ms[r], 8) == 0 && at == am[r]);
    }
    if (rows) {
      CHECK(hs_cluster_cover_codes_host(codes.data(), n, k, A, label.data(), min_size, S.data(), rows + 1, ms.data(),
                                        am.data()) == 1);
      S[S.size() - 1] = NAN;
      CHECK(hs_cluster_cover_codes_host(codes.data(), n, k, A, label.data(), min_size, S.data(), rows, ms.data(),
                                        am.data()) == 1);
    }
  }
  // refusals: nothing is written
  {
    const uint32_t k = 3, A = 20;
    const uint64_t n = 10;
    std::vector<uint8_t> codes(n * k, 1);
    std::vector<uint32_t> label = {0, 0, 0, 5, 5, HS_CP_NOISE, 5, 0, 9, 9};
    std::vector<uint32_t> ol(3, 9), osz(3, 9), counts(3 * k * A, 9), distinct(3, 9), am(3, 9);
    std::vector<uint64_t> wc(3 * k * A, 9), wsum(3, 9);
    std::vector<double> S(3 * k * A, 0.5), ms(3, 9.0);
    uint64_t rows = 0;
    auto weights = [&](uint32_t kk, uint32_t AA, uint32_t min_size, uint64_t cap, uint64_t* w, uint64_t nn = 10) {
      return hs_cluster_weights_codes_host(codes.data(), nn, kk, AA, label.data(), min_size, ol.data(), osz.data(),
                                           counts.data(), w, wsum.data(), distinct.data(), cap, &rows);
    };
    auto cover = [&](uint32_t kk, uint32_t AA, uint32_t min_size, uint64_t n_rows, const double* s) {
      return hs_cluster_cover_codes_host(codes.data(), n, kk, AA, label.data(), min_size, s, n_rows, ms.data(), am.data());
    };
    CHECK(weights(3, 20, 0, 3, wc.data()) == 1 && weights(0, 20, 2, 3, wc.data()) == 1);
    CHECK(weights(76, 20, 2, 3, wc.data()) == 1 && weights(3, 33, 2, 3, wc.data()) == 1 && weights(3, 0, 2, 3, wc.data()) == 1);
    CHECK(weights(3, 20, 2, 3, nullptr) == 1 && weights(3, 20, 2, 3, wc.data(), 1ull << 31) == 1);
    CHECK(weights(3, 20, 2, 2, wc.data()) == 3 && rows == 3);
    CHECK(cover(3, 20, 0, 3, S.data()) == 1 && cover(0, 20, 2, 3, S.data()) == 1 && cover(3, 33, 2, 3, S.data()) == 1);
    CHECK(cover(3, 20, 2, 2, S.data()) == 1 && cover(3, 20, 2, 3, nullptr) == 1);
    codes[5 * k + 1] = 20;  // a code at the alphabet's size, in a k-mer of no row
    CHECK(weights(3, 20, 2, 3, wc.data()) == 1 && cover(3, 20, 2, 3, S.data()) == 1);
    codes[5 * k + 1] = 1;
    label[2] = 10;  // a label at n
    CHECK(weights(3, 20, 2, 3, wc.data()) == 1 && cover(3, 20, 2, 3, S.data()) == 1);
    label[2] = 0;
    for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY, ldexp(1.0, 101), -1.3e30}) {
      S[7] = bad;
      CHECK(cover(3, 20, 2, 3, S.data()) == 1);
    }
    S[7] = ldexp(1.0, 100);  // the cap itself is legal
    for (uint32_t v : ol) CHECK(v == 9);
    for (uint32_t v : osz) CHECK(v == 9);
    for (uint32_t v : counts) CHECK(v == 9);
    for (uint32_t v : distinct) CHECK(v == 9);
    for (uint32_t v : am) CHECK(v == 9);
    for (uint64_t v : wc) CHECK(v == 9);
    for (uint64_t v : wsum) CHECK(v == 9);
    for (double v : ms) CHECK(v == 9.0);
    CHECK(weights(3, 20, 2, 3, wc.data()) == 0 && rows == 3 && ol[1] == 5 && osz[2] == 2 && distinct[0] == 3);
    CHECK(wsum[0] == 3ull << 56 && wsum[2] == 3ull << 56);
    CHECK(cover(3, 20, 2, 3, S.data()) == 0 && ms[1] == 1.5 && am[0] == 0 && am[1] == 3 && am[2] == 8);
    // an empty database
    CHECK(hs_cluster_weights_codes_host(nullptr, 0, k, A, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        nullptr, 0, &rows) == 0 && rows == 0);
    CHECK(hs_cluster_cover_codes_host(nullptr, 0, k, A, nullptr, 1, nullptr, 0, nullptr, nullptr) == 0);
  }
  printf("cluster_pssm_san ok\n");
  return 0;
}
