// pssm_compare_san.cpp -- hs_pssm_compare.h under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program
// (tests/test_pssm_compare_cpu.py compiles and runs it).  The host rule at the shapes' ends (k = 1, min_overlap = 1 and
// k, one profile, self mode), the capacity protocol, the tables at the extremes (all zero, below 2^-900, +-2^100, a
// forbidden residue), the invariant on random pairs, the shapes and step ranges of the filter, the column transform,
// and every refusal on sentinel-filled outputs.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../hsearch_amd/csrc/hs_pssm_compare.h"

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

static int one_shape(uint32_t k, uint32_t A, uint64_t nx, uint64_t ny, int kind) {
  const size_t n = (size_t)k * A;
  std::vector<double> X(nx * n), Y(ny * n), t(nx);
  for (auto& v : X) v = (double)((int)(rnd() % 33) - 16) / 8.0;
  for (auto& v : Y) v = (double)((int)(rnd() % 33) - 16) / 8.0;
  if (kind == 1) X[0] = -1e30;  // a forbidden residue
  if (kind == 2) {
    X[0] = 1.2676506002282294e30;
    Y[n - 1] = -1.2676506002282294e30;
  }
  if (kind == 3)
    for (size_t i = 0; i < n; ++i) X[i] = 0.0, Y[i] *= 1e-290;
  for (uint64_t m = 0; m < nx; ++m) t[m] = m % 3 == 0 ? -1.7976931348623157e308 : 0.5;
  // the tables, the shapes, and the invariant at every offset of every pair
  std::vector<int8_t> qx(nx * n), qy(ny * n);
  std::vector<double> sx(nx), lx(nx), ax(nx), sy(ny), ly(ny), ay(ny);
  CHECK(hs_pssm_compare_tables_host(X.data(), nx, k, A, qx.data(), sx.data(), lx.data(), ax.data()) == 0);
  CHECK(hs_pssm_compare_tables_host(Y.data(), ny, k, A, qy.data(), sy.data(), ly.data(), ay.data()) == 0);
  CHECK(hs_pssm_compare_tables_host(Y.data(), ny, k, A, nullptr, nullptr, nullptr, nullptr) == 0);
  for (uint32_t v : {1u, (k + 1) / 2, k}) {
    const hs_pcmp_shape sh = hs_pcmp_shape_of(k, A, v);
    CHECK(sh.stride % 16 == 0 && sh.stride >= A && sh.xrow == 2 * sh.lead + sh.yrow && sh.n_off == 2 * (k - v) + 1);
    CHECK((sh.steps == 0) == (k * sh.stride > HS_PCMP_MAX_ROW));
    uint64_t issued = 0;
    for (int d = -(int)(k - v); d <= (int)(k - v); ++d) {
      uint32_t lo, hi;
      hs_pcmp_step_range(k, sh.stride, d, &lo, &hi);
      CHECK(lo < hi && (sh.steps == 0 || hi <= sh.steps));
      // the bytes of the overlap's Y columns lie inside the steps kept
      const uint32_t p_lo = d < 0 ? (uint32_t)-d : 0, p_hi = d > 0 ? k - (uint32_t)d : k;
      CHECK(64 * lo <= p_lo * sh.stride && p_hi * sh.stride <= 64 * hi);
      issued += hi - lo;
      for (uint64_t x = 0; x < nx; ++x)
        for (uint64_t y = 0; y < ny; ++y) {
          const double sc = hs_pcmp_score(X.data() + x * n, Y.data() + y * n, k, A, d);
          CHECK(sc == hs_pcmp_score(Y.data() + y * n, X.data() + x * n, k, A, -d));
          int64_t I = 0;
          for (uint32_t p = p_lo; p < p_hi; ++p)
            for (uint32_t r = 0; r < A; ++r) I += (int64_t)qx[x * n + (p + d) * A + r] * qy[y * n + p * A + r];
          CHECK(hs_pcmp_pass(I, sx[x], lx[x], ax[x], sy[y], ly[y], k * A, sc));
        }
    }
    CHECK(sh.steps == 0 || issued == hs_pcmp_steps_issued(k, A, v));
    // the rule: two-call capacity protocol, cnt, self mode
    std::vector<uint64_t> cnt(nx, 99), cnt2(nx, 99);
    uint64_t nh = 0, nh2 = 0;
    CHECK(hs_pssm_compare_host_rule(X.data(), nx, Y.data(), ny, k, A, t.data(), v, nullptr, nullptr, nullptr, nullptr, 0,
                                    &nh, cnt.data()) == (nh ? 2 : 0));
    CHECK(nh >= ny * ((nx + 2) / 3));
    std::vector<uint32_t> hx(nh + 1, 7), hy(nh + 1, 7);
    std::vector<int32_t> hd(nh + 1, 7);
    std::vector<double> hs(nh + 1, 7.0);
    CHECK(hs_pssm_compare_host_rule(X.data(), nx, Y.data(), ny, k, A, t.data(), v, hx.data(), hy.data(), hd.data(),
                                    hs.data(), nh, &nh2, cnt2.data()) == 0);
    CHECK(nh2 == nh && hx[nh] == 7 && hy[nh] == 7 && hd[nh] == 7 && hs[nh] == 7.0);
    uint64_t total = 0;
    for (uint64_t m = 0; m < nx; ++m) {
      CHECK(cnt[m] == cnt2[m]);
      total += cnt[m];
    }
    CHECK(total == nh);
    for (uint64_t i = 0; i < nh; ++i) {
      CHECK(hx[i] < nx && hy[i] < ny && hd[i] >= -(int)(k - v) && hd[i] <= (int)(k - v) && hs[i] >= t[hx[i]]);
      CHECK(i == 0 || hx[i - 1] < hx[i] || (hx[i - 1] == hx[i] && hy[i - 1] < hy[i]));
      CHECK(hs[i] == hs_pcmp_score(X.data() + hx[i] * n, Y.data() + hy[i] * n, k, A, hd[i]));
    }
    if (nh > 1)  // one short: the count comes back, the first nh - 1 hits are written and no more
      CHECK(hs_pssm_compare_host_rule(X.data(), nx, Y.data(), ny, k, A, t.data(), v, hx.data(), hy.data(), hd.data(),
                                      hs.data(), nh - 1, &nh2, nullptr) == 2 && nh2 == nh);
    uint64_t ns = 0;
    CHECK(hs_pssm_compare_host_rule(X.data(), nx, nullptr, 12345, k, A, t.data(), v, hx.data(), hy.data(), hd.data(),
                                    hs.data(), 0, &ns, nullptr) == (ns ? 2 : 0));
    CHECK(ns <= nx * (nx - 1) / 2);
  }
  // the column transform, in place as well
  std::vector<double> out(nx * n), in_place = X;
  for (int mode = 0; mode < 2; ++mode) {
    if (kind == 1 || kind == 2) break;
    CHECK(hs_pssm_compare_columns_host(X.data(), nx, k, A, mode, out.data()) == 0);
    in_place = X;
    CHECK(hs_pssm_compare_columns_host(in_place.data(), nx, k, A, mode, in_place.data()) == 0);
    for (size_t i = 0; i < out.size(); ++i) CHECK(out[i] == in_place[i] && fabs(out[i]) <= 1.0);
  }
  return 0;
}

int main() {
  if (one_shape(1, 20, 3, 2, 0)) return 1;
  if (one_shape(3, 4, 4, 5, 0)) return 1;
  if (one_shape(7, 1, 3, 3, 0)) return 1;
  if (one_shape(25, 20, 3, 4, 1)) return 1;
  if (one_shape(26, 21, 2, 3, 2)) return 1;
  if (one_shape(32, 32, 1, 2, 0)) return 1;
  if (one_shape(33, 32, 2, 1, 3)) return 1;
  if (one_shape(75, 32, 1, 2, 0)) return 1;

  // the degenerate tables
  {
    const uint32_t k = 2, A = 3;
    double X[3][6] = {{0, 0, 0, 0, 0, 0}, {1e-290, -2e-290, 0, 0, 0, 5e-324}, {1.5, -0.5, 0.25, 0, 0, -1.5}};
    int8_t q[18];
    double s[3], l1[3], amax[3];
    CHECK(hs_pssm_compare_tables_host(&X[0][0], 3, k, A, q, s, l1, amax) == 0);
    CHECK(s[0] == 0 && l1[0] == 0 && amax[0] == 0 && s[1] == 0 && l1[1] > 1e308 && amax[1] == 2e-290);
    for (int i = 0; i < 12; ++i) CHECK(q[i] == 0);
    CHECK(q[12] == 127 && q[13] == -42 && q[14] == 21 && q[17] == -127 && l1[2] >= 3.75 && l1[2] < 3.7500001);
    // a pair with an all-zero or a tiny profile passes whatever finite t asks once its bound says so
    CHECK(hs_pcmp_pass(0, s[1], l1[1], amax[1], s[2], l1[2], 6, 1e300) == 1);
    CHECK(hs_pcmp_pass(0, s[0], l1[0], amax[0], s[2], l1[2], 6, 1e-300) == 0);
    CHECK(hs_pcmp_pass(0, s[0], l1[0], amax[0], s[2], l1[2], 6, 0.0) == 1);
    CHECK(hs_pcmp_pass(0, s[0], l1[0], amax[0], s[1], l1[1], 6, 1.0) == 1);  // 0 * inf: a NaN bound passes
  }
  // the tie order
  CHECK(hs_pcmp_rank(0) == 0 && hs_pcmp_rank(-1) == 1 && hs_pcmp_rank(1) == 2 && hs_pcmp_rank(-74) == 147 &&
        hs_pcmp_rank(74) == 148);

  // refusals write nothing
  const uint32_t k = 3, A = 4;
  const double nan = strtod("nan", nullptr), inf = strtod("inf", nullptr);
  std::vector<double> X(2 * k * A, 0.5), Y(3 * k * A, 0.25), t(2, 0.0);
  std::vector<uint32_t> hx(8, 9), hy(8, 9);
  std::vector<int32_t> hd(8, 9);
  std::vector<double> hs(8, 9.0);
  std::vector<uint64_t> cnt(2, 9);
  uint64_t nh = 77;
  auto run = [&](const double* XX, uint64_t nx, const double* YY, uint64_t ny, uint32_t kk, uint32_t AA, const double* tt,
                 uint32_t v, uint32_t* out_x) {
    return hs_pssm_compare_host_rule(XX, nx, YY, ny, kk, AA, tt, v, out_x, hy.data(), hd.data(), hs.data(), 8, &nh,
                                     cnt.data());
  };
  CHECK(run(X.data(), 2, Y.data(), 3, k, A, t.data(), 0, hx.data()) == 1);
  CHECK(run(X.data(), 2, Y.data(), 3, k, A, t.data(), k + 1, hx.data()) == 1);
  CHECK(run(X.data(), 1ull << 27, Y.data(), 3, k, A, t.data(), 1, hx.data()) == 1);
  CHECK(run(X.data(), 2, Y.data(), 1ull << 27, k, A, t.data(), 1, hx.data()) == 1);
  CHECK(run(X.data(), 0, Y.data(), 3, k, A, t.data(), 1, hx.data()) == 1);
  CHECK(run(X.data(), 2, Y.data(), 0, k, A, t.data(), 1, hx.data()) == 1);
  CHECK(run(nullptr, 2, Y.data(), 3, k, A, t.data(), 1, hx.data()) == 1);
  CHECK(run(X.data(), 2, Y.data(), 3, k, A, nullptr, 1, hx.data()) == 1);
  CHECK(run(X.data(), 2, Y.data(), 3, k, A, t.data(), 1, nullptr) == 1);
  CHECK(run(X.data(), 2, Y.data(), 3, 0, A, t.data(), 1, hx.data()) == 1);
  CHECK(run(X.data(), 2, Y.data(), 3, 76, A, t.data(), 1, hx.data()) == 1);
  CHECK(run(X.data(), 2, Y.data(), 3, k, 0, t.data(), 1, hx.data()) == 1);
  CHECK(run(X.data(), 2, Y.data(), 3, k, 33, t.data(), 1, hx.data()) == 1);
  for (double bad : {nan, inf, -inf, 2.6e30}) {
    std::vector<double> X2 = X, Y2 = Y, t2 = t;
    X2[5] = bad;
    CHECK(run(X2.data(), 2, Y.data(), 3, k, A, t.data(), 1, hx.data()) == 1);
    CHECK(run(X2.data(), 2, nullptr, 0, k, A, t.data(), 1, hx.data()) == 1);
    Y2[35] = bad;
    CHECK(run(X.data(), 2, Y2.data(), 3, k, A, t.data(), 1, hx.data()) == 1);
    t2[1] = bad;
    CHECK(run(X.data(), 2, Y.data(), 3, k, A, t2.data(), 1, hx.data()) == (bad == 2.6e30 ? 0 : 1));
    if (bad == 2.6e30) {
      CHECK(nh == 3 && hx[2] == 0 && hx[3] == 9);
      hx.assign(8, 9), hy.assign(8, 9), hd.assign(8, 9), hs.assign(8, 9.0), cnt.assign(2, 9);
    }
    CHECK(hs_pssm_compare_tables_host(X2.data(), 2, k, A, nullptr, hs.data(), hs.data(), hs.data()) == 1);
    CHECK(hs_pssm_compare_columns_host(X2.data(), 2, k, A, 0, hs.data()) == 1);
  }
  CHECK(hs_pssm_compare_columns_host(X.data(), 2, k, A, 2, hs.data()) == 1);
  CHECK(hs_pssm_compare_columns_host(X.data(), 2, k, A, -1, hs.data()) == 1);
  CHECK(hs_pssm_compare_columns_host(nullptr, 2, k, A, 0, hs.data()) == 1);
  for (int i = 0; i < 8; ++i) CHECK(hx[i] == 9 && hy[i] == 9 && hd[i] == 9 && hs[i] == 9.0);
  CHECK(cnt[0] == 9 && cnt[1] == 9);
  // nothing to do
  CHECK(run(nullptr, 0, nullptr, 0, k, A, nullptr, 1, hx.data()) == 0 && nh == 0);
  CHECK(run(nullptr, 0, Y.data(), 0, k, A, nullptr, 1, hx.data()) == 0 && nh == 0);
  CHECK(run(X.data(), 1, nullptr, 0, k, A, t.data(), 1, hx.data()) == 0 && nh == 0);  // one profile: no pair x < y
  printf("pssm_compare_san ok\n");
  return 0;
}
