// Stand-alone driver of hsearch_amd/csrc/hs_pssm_counts.h for the sanitizer run of tests/test_pssm_counts_cpu.py: the
// counting rule in both modes on shuffled tuple lists with ties and repeats against a plain loop over the slots, the
// log-odds against its own expression and itself, the background, and the refused inputs -- with output arrays of
// exactly the needed size.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../hsearch_amd/csrc/hs_pssm_counts.h"

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #c);           \
      return 1;                                               \
    }                                                         \
  } while (0)

int main() {
  std::mt19937_64 rng(31);
  const std::vector<std::vector<uint64_t>> layouts = {
      {0, 0, 0, 5, 5, 5, 12, 40, 40, 41, 60, 60, 60}, {0, 60}, {0, 1, 2, 3, 60}, {0, 0, 60, 60}};
  const uint32_t shapes[][2] = {{1, 20}, {7, 20}, {25, 20}, {4, 32}, {75, 32}};
  for (int round = 0; round < 60; ++round) {
    const std::vector<uint64_t>& id_start = layouts[round % layouts.size()];
    const uint64_t n_seq = id_start.size() - 1, n = id_start[n_seq];
    const uint32_t k = shapes[round % 5][0], A = shapes[round % 5][1];
    const uint64_t nm = 1 + rng() % 4;
    const size_t nt = rng() % 400, cells = (size_t)k * A;
    std::vector<uint8_t> codes(n * k);
    for (auto& c : codes) c = (uint8_t)(rng() % A);
    std::vector<uint32_t> m(nt), id(nt);
    std::vector<double> sc(nt);
    for (size_t i = 0; i < nt; ++i) {
      m[i] = (uint32_t)(rng() % nm);
      id[i] = (uint32_t)(rng() % n);
      sc[i] = (double)((int)((id[i] * 7u + m[i] * 3u) % 5u) - 2);  // a function of (m, id): repeats agree; heavy ties
    }
    for (int mode = 0; mode < 2; ++mode) {
      // the sites by a plain loop over the slots
      std::vector<uint32_t> want(nm * cells, 0);
      std::vector<uint64_t> want_used(nm, 0);
      for (uint64_t mm = 0; mm < nm; ++mm)
        for (uint64_t s = 0; s < n_seq; ++s) {
          bool any = false;
          uint64_t best = 0;
          double bs = 0;
          for (uint64_t x = id_start[s]; x < id_start[s + 1]; ++x) {
            bool hit = false;
            double v = 0;
            for (size_t i = 0; i < nt && !hit; ++i)
              if (m[i] == mm && id[i] == x) {
                hit = true;
                v = sc[i];
              }
            if (!hit) continue;
            if (!mode) {
              for (uint32_t p = 0; p < k; ++p) ++want[mm * cells + (size_t)p * A + codes[x * k + p]];
              ++want_used[mm];
            } else if (!any || v > bs) {
              bs = v;
              best = x;
            }
            any = true;
          }
          if (mode && any) {
            for (uint32_t p = 0; p < k; ++p) ++want[mm * cells + (size_t)p * A + codes[best * k + p]];
            ++want_used[mm];
          }
        }
      std::vector<uint32_t> counts(nm * cells, 9);
      std::vector<uint64_t> used(nm, 9);
      CHECK(hs_pssm_count_hits_host(codes.data(), n, k, A, m.data(), id.data(), sc.data(), nt, nm,
                                    mode ? id_start.data() : nullptr, n_seq, counts.data(), used.data()) == 0);
      CHECK(counts == want && used == want_used);
      std::vector<uint32_t> again(nm * cells, 9);
      CHECK(hs_pssm_count_hits_host(codes.data(), n, k, A, m.data(), id.data(), sc.data(), nt, nm,
                                    mode ? id_start.data() : nullptr, n_seq, again.data(), nullptr) == 0);
      CHECK(again == want);
      for (uint64_t mm = 0; mm < nm; ++mm)
        for (uint32_t p = 0; p < k; ++p) {
          uint64_t sum = 0;
          for (uint32_t a = 0; a < A; ++a) sum += counts[mm * cells + (size_t)p * A + a];
          CHECK(sum == used[mm]);
        }
      // the log-odds of these counts: the expression, finite, and the function against itself
      std::vector<double> bg(A), S(nm * cells, 9.0), S2(nm * cells, 7.0);
      for (auto& b : bg) b = (double)(1 + rng() % 9) / 64.0;
      const double pseudo = mode ? 0.5 : 1.0;
      CHECK(hs_pssm_log_odds_host(counts.data(), nm, k, A, bg.data(), pseudo, S.data()) == 0);
      CHECK(hs_pssm_log_odds_host(counts.data(), nm, k, A, bg.data(), pseudo, S2.data()) == 0);
      CHECK(memcmp(S.data(), S2.data(), S.size() * 8) == 0);
      for (uint64_t r = 0; r < nm * k; ++r)
        for (uint32_t a = 0; a < A; ++a) {
          const double size = (double)used[r / k];
          const double prod = pseudo * bg[a];
          const double num = (double)counts[r * A + a] + prod;
          const double den = size + pseudo;
          const double freq = num / den;
          const double ratio = freq / bg[a];
          CHECK(S[r * A + a] == log2(ratio) && isfinite(S[r * A + a]));
        }
      // the background of the first profile's counts
      std::vector<double> out(A, 9.0);
      const int rb = hs_pssm_background_host(counts.data(), k, A, out.data());
      if (!want_used[0]) {
        CHECK(rb == 1 && out[0] == 9.0);
      } else {
        CHECK(rb == 0);
        double least = 2.0;
        for (uint32_t a = 0; a < A; ++a) {
          uint64_t col = 0;
          for (uint32_t p = 0; p < k; ++p) col += counts[(size_t)p * A + a];
          if (col) {
            CHECK(out[a] == (double)col / (double)(want_used[0] * k));
            least = std::min(least, out[a]);
          }
        }
        for (uint32_t a = 0; a < A; ++a) CHECK(out[a] > 0.0 && out[a] >= least);
      }
    }
  }
  // refusals: nothing is written
  {
    const std::vector<uint64_t> id_start = {0, 3, 10};
    const uint32_t k = 3, A = 20;
    std::vector<uint8_t> codes(10 * k, 1);
    std::vector<uint32_t> m = {0, 0, 1}, id = {4, 4, 2};
    std::vector<double> sc = {1.0, 2.0, 0.5};
    std::vector<uint32_t> counts(2 * k * A, 9);
    std::vector<uint64_t> used(2, 9);
    auto call = [&](uint64_t nm, const uint64_t* ids, uint64_t n_seq, uint32_t* c, uint32_t kk = 3, uint32_t AA = 20,
                    uint64_t n = 10) {
      return hs_pssm_count_hits_host(codes.data(), n, kk, AA, m.data(), id.data(), sc.data(), 3, nm, ids, n_seq, c,
                                     used.data());
    };
    for (int mode = 0; mode < 2; ++mode) {
      const uint64_t* ids = mode ? id_start.data() : nullptr;
      sc = {1.0, 2.0, 0.5};
      CHECK(call(2, ids, 2, counts.data()) == 1);  // two scores for (0, 4)
      sc[1] = 1.0;
      CHECK(call(1, ids, 2, counts.data()) == 1);  // m >= nm
      CHECK(call(2, ids, 2, nullptr) == 1);        // a null counts
      CHECK(call(2, ids, 2, counts.data(), 0) == 1 && call(2, ids, 2, counts.data(), 3, 33) == 1);
      CHECK(call(2, ids, 2, counts.data(), 3, 20, 4) == 1);  // an id at n
      sc[2] = NAN;
      CHECK(call(2, ids, 2, counts.data()) == 1);
      sc[2] = 0.5;
      codes[4 * k + 1] = 20;  // a counted code at the alphabet's size
      CHECK(call(2, ids, 2, counts.data()) == 1);
      codes[4 * k + 1] = 1;
    }
    const std::vector<uint64_t> ends_early = {0, 3, 9}, starts_late = {1, 3, 10}, descends = {0, 11, 10};
    CHECK(call(2, ends_early.data(), 2, counts.data()) == 1);
    CHECK(call(2, starts_late.data(), 2, counts.data()) == 1);
    CHECK(call(2, descends.data(), 2, counts.data()) == 1);
    CHECK(call(2, id_start.data(), 0, counts.data()) == 1);
    for (uint32_t c : counts) CHECK(c == 9);
    CHECK(used[0] == 9 && used[1] == 9);
    CHECK(call(2, id_start.data(), 2, counts.data()) == 0 && used[0] == 1 && used[1] == 1 && counts[1] == 1);
    // log-odds and background
    std::vector<double> bg(A, 0.05), S(2 * k * A, 9.0);
    CHECK(hs_pssm_log_odds_host(counts.data(), 2, k, A, bg.data(), 0.0, S.data()) == 1);
    CHECK(hs_pssm_log_odds_host(counts.data(), 2, k, A, bg.data(), -1.0, S.data()) == 1);
    CHECK(hs_pssm_log_odds_host(counts.data(), 2, k, A, bg.data(), INFINITY, S.data()) == 1);
    CHECK(hs_pssm_log_odds_host(counts.data(), 2, k, A, bg.data(), NAN, S.data()) == 1);
    CHECK(hs_pssm_log_odds_host(counts.data(), 2, k, A, nullptr, 1.0, S.data()) == 1);
    CHECK(hs_pssm_log_odds_host(counts.data(), 2, k, A, bg.data(), 1.0, nullptr) == 1);
    for (double bad : {0.0, -0.1, (double)INFINITY, (double)NAN}) {
      bg[7] = bad;
      CHECK(hs_pssm_log_odds_host(counts.data(), 2, k, A, bg.data(), 1.0, S.data()) == 1);
    }
    bg[7] = 5e-324;  // pseudo * bg rounds to zero: an entry would be log2(0)
    CHECK(hs_pssm_log_odds_host(counts.data(), 2, k, A, bg.data(), 0.5, S.data()) == 1);
    for (double s : S) CHECK(s == 9.0);
    bg[7] = 0.05;
    CHECK(hs_pssm_log_odds_host(counts.data(), 2, k, A, bg.data(), 1.0, S.data()) == 0);
    CHECK(hs_pssm_log_odds_host(nullptr, 0, k, A, bg.data(), 1.0, nullptr) == 0);
    std::vector<uint32_t> none(k * A, 0);
    std::vector<double> out(A, 9.0);
    CHECK(hs_pssm_background_host(none.data(), k, A, out.data()) == 1 && out[0] == 9.0);
    CHECK(hs_pssm_background_host(nullptr, k, A, out.data()) == 1 && hs_pssm_background_host(none.data(), k, A, nullptr) == 1);
    // no tuples: an empty, successful call in both modes
    const uint64_t zero = 0;
    CHECK(hs_pssm_count_hits_host(nullptr, 0, k, A, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr) == 0);
    CHECK(hs_pssm_count_hits_host(nullptr, 0, k, A, nullptr, nullptr, nullptr, 0, 0, &zero, 0, nullptr, nullptr) == 0);
  }
  printf("pssm_counts_san ok\n");
  return 0;
}
