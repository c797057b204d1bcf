// Stand-alone driver of hsearch_amd/csrc/hs_pssm_weights.h for the sanitizer run of tests/test_pssm_weights_cpu.py: the
// weighting rule in both modes on shuffled tuple lists with ties and repeats against a plain loop in 128-bit integers
// over the raw counts of hs_pssm_count_hits_host, the column sums and the bound on wsum, u at its extremes, the
// weighted log-odds against its own expression, and the refused inputs -- with output arrays of exactly the needed size.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../hsearch_amd/csrc/hs_pssm_weights.h"

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #c);           \
      return 1;                                               \
    }                                                         \
  } while (0)

int main() {
  // u at its extremes
  CHECK(hs_pssm_weight_unit(1, 1) == 1ull << 56);
  CHECK(hs_pssm_weight_unit(32, 4294967295u) == (1ull << 56) / (32ull * 4294967295ull));
  CHECK(hs_pssm_weight_unit(32, 4294967295u) == 524288ull);
  CHECK(hs_pssm_weight_unit(20, 0) == 0 && hs_pssm_weight_unit(0, 5) == 0 && hs_pssm_weight_unit(0, 0) == 0);
  CHECK(hs_pssm_weight_unit(3, 7) == 3431314001806092ull);  // floor(2^56 / 21): 21 * 3431314001806092 + 4 = 2^56
  std::mt19937_64 rng(57);
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
    for (auto& c : codes) c = (uint8_t)(rng() % (round % 3 ? A : 3));  // every third round: few residues, many repeats
    std::vector<uint32_t> m(nt), id(nt);
    std::vector<double> sc(nt);
    for (size_t i = 0; i < nt; ++i) {
      m[i] = (uint32_t)(rng() % nm);
      id[i] = (uint32_t)(rng() % n);
      sc[i] = (double)((int)((id[i] * 7u + m[i] * 3u) % 5u) - 2);  // a function of (m, id): repeats agree; heavy ties
    }
    for (int mode = 0; mode < 2; ++mode) {
      const uint64_t* const ids = mode ? id_start.data() : nullptr;
      std::vector<uint32_t> raw(nm * cells, 9), counts(nm * cells, 9), distinct(nm, 9);
      std::vector<uint64_t> raw_used(nm, 9), used(nm, 9), wc(nm * cells, 9), wsum(nm, 9);
      CHECK(hs_pssm_count_hits_host(codes.data(), n, k, A, m.data(), id.data(), sc.data(), nt, nm, ids, n_seq,
                                    raw.data(), raw_used.data()) == 0);
      CHECK(hs_pssm_weight_hits_host(codes.data(), n, k, A, m.data(), id.data(), sc.data(), nt, nm, ids, n_seq,
                                     counts.data(), wc.data(), wsum.data(), distinct.data(), used.data()) == 0);
      CHECK(counts == raw && used == raw_used);
      // the sites again, by the slots: a site's weight from the raw counts, in 128-bit integers
      std::vector<unsigned __int128> want(nm * cells, 0), want_sum(nm, 0);
      for (uint64_t mm = 0; mm < nm; ++mm) {
        std::vector<uint32_t> r(k, 0);
        uint32_t d = 0;
        for (uint32_t p = 0; p < k; ++p) {
          for (uint32_t a = 0; a < A; ++a) r[p] += raw[mm * cells + (size_t)p * A + a] > 0;
          d += r[p];
        }
        CHECK(distinct[mm] == d);
        for (uint64_t s = 0; s < n_seq; ++s) {
          bool any = false;
          uint64_t best = 0;
          double bs = 0;
          std::vector<uint64_t> sites;
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
              sites.push_back(x);
            } else if (!any || v > bs) {
              bs = v;
              best = x;
            }
            any = true;
          }
          if (mode && any) sites.push_back(best);
          for (uint64_t x : sites) {
            unsigned __int128 w = 0;
            for (uint32_t p = 0; p < k; ++p) {
              const uint64_t c = raw[mm * cells + (size_t)p * A + codes[x * k + p]];
              CHECK(c > 0);
              w += (((unsigned __int128)1) << 56) / ((unsigned __int128)r[p] * c);
            }
            for (uint32_t p = 0; p < k; ++p) want[mm * cells + (size_t)p * A + codes[x * k + p]] += w;
            want_sum[mm] += w;
          }
        }
        CHECK(want_sum[mm] <= ((unsigned __int128)k << 56) && wsum[mm] == (uint64_t)want_sum[mm]);
        for (size_t e = 0; e < cells; ++e) CHECK(wc[mm * cells + e] == (uint64_t)want[mm * cells + e]);
        for (uint32_t p = 0; p < k; ++p) {
          uint64_t sum = 0;
          for (uint32_t a = 0; a < A; ++a) sum += wc[mm * cells + (size_t)p * A + a];
          CHECK(sum == wsum[mm]);
        }
      }
      // every optional output left out
      std::vector<uint64_t> again(nm * cells, 9);
      CHECK(hs_pssm_weight_hits_host(codes.data(), n, k, A, m.data(), id.data(), sc.data(), nt, nm, ids, n_seq, nullptr,
                                     again.data(), nullptr, nullptr, nullptr) == 0);
      CHECK(again == wc);
      // the log-odds of these weighted counts: the expression, finite, and the function against itself
      std::vector<double> bg(A), n_eff(nm), S(nm * cells, 9.0), S2(nm * cells, 7.0);
      for (auto& b : bg) b = (double)(1 + rng() % 9) / 64.0;
      for (uint64_t mm = 0; mm < nm; ++mm) n_eff[mm] = mode ? (double)distinct[mm] / (double)k : (double)used[mm];
      const double pseudo = mode ? 0.5 : 1.0;
      CHECK(hs_pssm_log_odds_weighted_host(wc.data(), wsum.data(), n_eff.data(), nm, k, A, bg.data(), pseudo,
                                           S.data()) == 0);
      CHECK(hs_pssm_log_odds_weighted_host(wc.data(), wsum.data(), n_eff.data(), nm, k, A, bg.data(), pseudo,
                                           S2.data()) == 0);
      CHECK(memcmp(S.data(), S2.data(), S.size() * 8) == 0);
      for (uint64_t r = 0; r < nm * k; ++r)
        for (uint32_t a = 0; a < A; ++a) {
          const uint64_t mm = r / k;
          const double f = wsum[mm] ? (double)wc[r * A + a] / (double)wsum[mm] : 0.0;
          const double x = f * n_eff[mm];
          const double prod = pseudo * bg[a];
          const double num = x + prod;
          const double den = n_eff[mm] + pseudo;
          const double freq = num / den;
          const double ratio = freq / bg[a];
          CHECK(S[r * A + a] == log2(ratio) && isfinite(S[r * A + a]));
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
    std::vector<uint32_t> counts(2 * k * A, 9), distinct(2, 9);
    std::vector<uint64_t> wc(2 * k * A, 9), wsum(2, 9), used(2, 9);
    auto call = [&](uint64_t nm, const uint64_t* ids, uint64_t n_seq, uint64_t* w, uint32_t kk = 3, uint32_t AA = 20,
                    uint64_t n = 10) {
      return hs_pssm_weight_hits_host(codes.data(), n, kk, AA, m.data(), id.data(), sc.data(), 3, nm, ids, n_seq,
                                      counts.data(), w, wsum.data(), distinct.data(), used.data());
    };
    for (int mode = 0; mode < 2; ++mode) {
      const uint64_t* ids = mode ? id_start.data() : nullptr;
      sc = {1.0, 2.0, 0.5};
      CHECK(call(2, ids, 2, wc.data()) == 1);  // two scores for (0, 4)
      sc[1] = 1.0;
      CHECK(call(1, ids, 2, wc.data()) == 1);  // m >= nm
      CHECK(call(2, ids, 2, nullptr) == 1);    // a null wcounts
      CHECK(call(2, ids, 2, wc.data(), 0) == 1 && call(2, ids, 2, wc.data(), 3, 33) == 1);
      CHECK(call(2, ids, 2, wc.data(), 128) == 1);        // k above 127
      CHECK(call(2, ids, 2, wc.data(), 3, 20, 4) == 1);   // an id at n
      sc[2] = NAN;
      CHECK(call(2, ids, 2, wc.data()) == 1);
      sc[2] = 0.5;
      codes[4 * k + 1] = 20;  // a counted code at the alphabet's size
      CHECK(call(2, ids, 2, wc.data()) == 1);
      codes[4 * k + 1] = 1;
    }
    const std::vector<uint64_t> ends_early = {0, 3, 9}, starts_late = {1, 3, 10}, descends = {0, 11, 10};
    CHECK(call(2, ends_early.data(), 2, wc.data()) == 1);
    CHECK(call(2, starts_late.data(), 2, wc.data()) == 1);
    CHECK(call(2, descends.data(), 2, wc.data()) == 1);
    CHECK(call(2, id_start.data(), 0, wc.data()) == 1);
    for (uint32_t c : counts) CHECK(c == 9);
    for (uint64_t c : wc) CHECK(c == 9);
    CHECK(used[0] == 9 && used[1] == 9 && wsum[0] == 9 && wsum[1] == 9 && distinct[0] == 9 && distinct[1] == 9);
    // one site per profile: every position has one residue once, u = 2^56, W = k 2^56
    CHECK(call(2, id_start.data(), 2, wc.data()) == 0 && used[0] == 1 && used[1] == 1 && counts[1] == 1);
    CHECK(wsum[0] == 3ull << 56 && wsum[1] == 3ull << 56 && wc[1] == 3ull << 56 && distinct[0] == 3 && distinct[1] == 3);
    // the weighted log-odds
    std::vector<double> bg(A, 0.05), ne = {1.0, 1.0}, S(2 * k * A, 9.0);
    auto lo = [&](const double* b, double pseudo, double* out, const double* n_eff) {
      return hs_pssm_log_odds_weighted_host(wc.data(), wsum.data(), n_eff, 2, k, A, b, pseudo, out);
    };
    CHECK(lo(bg.data(), 0.0, S.data(), ne.data()) == 1 && lo(bg.data(), -1.0, S.data(), ne.data()) == 1);
    CHECK(lo(bg.data(), INFINITY, S.data(), ne.data()) == 1 && lo(bg.data(), NAN, S.data(), ne.data()) == 1);
    CHECK(lo(nullptr, 1.0, S.data(), ne.data()) == 1 && lo(bg.data(), 1.0, nullptr, ne.data()) == 1);
    CHECK(lo(bg.data(), 1.0, S.data(), nullptr) == 1);
    for (double bad : {0.0, -0.1, (double)INFINITY, (double)NAN}) {
      bg[7] = bad;
      CHECK(lo(bg.data(), 1.0, S.data(), ne.data()) == 1);
    }
    bg[7] = 0.05;
    for (double bad : {-1.0, -5e-324, (double)INFINITY, (double)NAN}) {
      ne[1] = bad;
      CHECK(lo(bg.data(), 1.0, S.data(), ne.data()) == 1);
    }
    ne[1] = 0.0;
    wc[2 * k * A - 1] = wsum[1] + 1;  // an entry above its wsum
    CHECK(lo(bg.data(), 1.0, S.data(), ne.data()) == 1);
    wc[2 * k * A - 1] = 0;
    CHECK(hs_pssm_log_odds_weighted_host(wc.data(), nullptr, ne.data(), 2, k, A, bg.data(), 1.0, S.data()) == 1);
    CHECK(hs_pssm_log_odds_weighted_host(nullptr, wsum.data(), ne.data(), 2, k, A, bg.data(), 1.0, S.data()) == 1);
    for (double s : S) CHECK(s == 9.0);
    CHECK(lo(bg.data(), 1.0, S.data(), ne.data()) == 0);
    for (double s : S) CHECK(isfinite(s));
    CHECK(hs_pssm_log_odds_weighted_host(nullptr, nullptr, nullptr, 0, k, A, bg.data(), 1.0, nullptr) == 0);
    // no tuples: an empty, successful call in both modes
    const uint64_t zero = 0;
    CHECK(hs_pssm_weight_hits_host(nullptr, 0, k, A, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr,
                                   nullptr, nullptr, nullptr) == 0);
    CHECK(hs_pssm_weight_hits_host(nullptr, 0, k, A, nullptr, nullptr, nullptr, 0, 0, &zero, 0, nullptr, nullptr, nullptr,
                                   nullptr, nullptr) == 0);
  }
  printf("pssm_weights_san ok\n");
  return 0;
}
