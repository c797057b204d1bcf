// The PSSM filter's host tables (hsearch_amd/csrc/hs_pssm_tables.h) with a stand-alone main, for
// tests/test_pssm_cpu.py: g++ -fsanitize=address,undefined, no GPU, no library.  Profiles are drawn here by a small
// generator; for k = 3 over 4 residues every one of the 64 k-mers is checked against the invariant, and the largest
// shapes (k = 75 over 32 residues) run through the same routine with exactly sized arrays.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../hsearch_amd/csrc/hs_pssm_tables.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

static int fails = 0;
#define CHECK(c)                                         \
  do {                                                   \
    if (!(c)) {                                          \
      printf("line %d: %s\n", __LINE__, #c);             \
      ++fails;                                           \
    }                                                    \
  } while (0)

// every k-mer of k = 3 over 4 residues against one profile
static void exhaustive(const std::vector<double>& S, double t) {
  const uint32_t k = 3, A = 4;
  std::vector<uint8_t> code(k * A, 0xff);
  double tau = 0.0;
  uint8_t dead = 9;
  CHECK(hs_pssm_tables_host(S.data(), &t, 1, k, A, code.data(), &tau, &dead) == 0);
  for (uint32_t x = 0; x < 64; ++x) {
    const uint32_t r[3] = {x & 3u, (x >> 2) & 3u, x >> 4};
    double sc = 0.0;
    int f8 = 0;
    for (uint32_t p = 0; p < k; ++p) {
      sc = sc + S[p * A + r[p]];
      CHECK(code[p * A + r[p]] < 64);
      f8 += hs_pssm_e2m3_eighths(code[p * A + r[p]]);
    }
    if (sc >= t) {
      CHECK(!dead);
      CHECK((double)f8 / 8.0 >= tau);
    }
  }
}

int main() {
  for (int it = 0; it < 400; ++it) {
    std::vector<double> S(12);
    const double scale = ldexp(1.0, (int)(rnd() % 40) - 20);
    for (double& v : S) v = (uni() * 2.0 - 1.0) * scale;
    if (it % 7 == 0) S[rnd() % 12] = -1e30;
    if (it % 11 == 0)
      for (double& v : S) v = S[0];
    double t = (uni() * 6.0 - 3.0) * scale;
    if (it % 5 == 0) t = (S[rnd() % 4] + S[4 + rnd() % 4]) + S[8 + rnd() % 4];  // an attained score
    exhaustive(S, t);
  }
  const double big = ldexp(1.0, 60);
  const double fam[3] = {-1.0, big, -big};
  for (int perm = 0; perm < 6; ++perm) {
    static const int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    std::vector<double> S(12);
    for (int p = 0; p < 3; ++p)
      for (int a = 0; a < 4; ++a) S[p * 4 + a] = (a & 1 ? -1.0 : 1.0) * fam[P[perm][p]] * (a & 2 ? 0.5 : 1.0);
    exhaustive(S, 0.5);
    exhaustive(S, -0.5);
  }
  {  // the largest shape, exactly sized arrays
    const uint32_t k = 75, A = 32, nm = 3;
    std::vector<double> S((size_t)nm * k * A), t(nm), tau(nm);
    for (double& v : S) v = uni() * 8.0 - 6.0;
    t[0] = 40.0;
    t[1] = 1e9;
    t[2] = -1e9;
    std::vector<uint8_t> code(S.size()), dead(nm);
    CHECK(hs_pssm_tables_host(S.data(), t.data(), nm, k, A, code.data(), tau.data(), dead.data()) == 0);
    CHECK(dead[1] == 1 && dead[0] == 0 && dead[2] == 0);
    CHECK(hs_pssm_steps(k, A) == 19);
    S[5] = NAN;
    CHECK(hs_pssm_tables_host(S.data(), t.data(), nm, k, A, code.data(), tau.data(), dead.data()) == 1);
    S[5] = ldexp(1.0, 101);
    CHECK(hs_pssm_tables_host(S.data(), t.data(), nm, k, A, code.data(), tau.data(), dead.data()) == 1);
    S[5] = 0.0;
    t[2] = INFINITY;
    CHECK(hs_pssm_tables_host(S.data(), t.data(), nm, k, A, code.data(), tau.data(), dead.data()) == 1);
    CHECK(hs_pssm_tables_host(S.data(), t.data(), 0, k, A, nullptr, nullptr, nullptr) == 0);
    CHECK(hs_pssm_tables_host(S.data(), t.data(), 1, 76, A, nullptr, nullptr, nullptr) == 1);
  }
  if (fails) {
    printf("pssm_tables_san: %d checks failed\n", fails);
    return 1;
  }
  printf("pssm_tables_san ok\n");
  return 0;
}
