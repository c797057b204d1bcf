// hs_pssm_compare.h -- profile against profile at every offset (hs_pssm_compare, include/hsearch.h; DESIGN.md section
// 29): the contract on one CPU thread, the tables of the int8 MFMA filter (hs_pssm_compare.hip) as __host__ __device__
// routines -- the device builds them with these, the host exports them, so that the invariant is tested where there
// is no GPU -- and the column transform.  Host-compilable: nothing here needs hipcc.
//
// THE FILTER'S INVARIANT.  For every (x, y, d) with d allowed: if the contract's ROUNDED score(x, y, d) reaches t[x],
// the pair passes hs_pcmp_pass at I = the largest exact integer sum of code products over the allowed offsets.  The
// filter never decides a hit: the exact pass evaluates the contract on every pair it lets through.
//
//  Tables of a profile of n = k * alphabet entries x_i:  amax = max |x_i|;  s = fl(amax / 127);  q_i = rint(fl(x_i / s))
//  in -127 .. 127;  l1 >= sum |x_i|.  A profile with amax = 0 has s = 0, q = 0, l1 = 0.  A profile with 0 < amax <
//  2^-900 (s would be subnormal, its relative error unbounded) has s = 0, q = 0 and l1 = +infinity: every pair with it
//  passes (hs_pcmp_pass lets a NaN or an infinite bound through).  Otherwise s is normal, fl(x / s) = (x / s)(1 + e),
//  |e| <= u = 2^-53, |x / s| <= 127 (1 + 2 u), so |x_i - s q_i| <= s (1/2 + 128 u).
//  (1) Quantisation.  Over the entry pairs (i, j) of an overlap, with x = s_x q + e, y = s_y p + f:
//        sum x y - s_x s_y sum q p = sum e y + sum (s_x q) f,   |s_x q| <= |x| + |e|,
//      so |real sum - s_x s_y I_d| <= E = s_x/2 l1_y + s_y/2 l1_x + n s_x s_y / 4, times (1 + 256 u) for the codes'
//      own roundings.  l1 and n of whole profiles overestimate a partial overlap.
//  (2) From the rounded score to the real sum.  Every product is rounded once and then passes through at most
//      (alphabet - 1) + (k - 1) rounded additions (the additions to +0.0 are exact), k + alphabet - 1 <= n roundings in
//      all: |rounded - real| <= gamma_n sum |x y| <= gamma_n amax_x l1_y, gamma_n = n u / (1 - n u) < n 2^-52.  A
//      product that underflows adds at most 2^-1075 of absolute error; additions have none.
//  (3) The test's own arithmetic.  hs_pcmp_pass evaluates  ub = s_x s_y I + E + R  with R = n 2^-52 amax_x l1_y in
//      fp64; each of its fewer than 16 operations has relative error u on a term of magnitude at most M = |s_x s_y I|
//      + E + R, or an underflow error below 2^-1074.  ub + 2^-40 M + 2^-1000 covers (1), (2) and (3): 2^-40 > 256 u +
//      16 u, 2^-1000 > n 2^-1075 + 16 2^-1074.  Since s_x s_y >= 0, I_d <= I gives the same bound at the largest I.
//  The int32 accumulators cannot overflow: 127^2 * 1024 < 2^24.
//
// THE FILTER'S SHAPE.  A profile is flattened to k * stride bytes, stride = the alphabet rounded up to 16: a shift by
// one column keeps every operand read a 16-byte aligned ds_read_b128 (1.6 x the depth at 20 residues; a 4-byte stride
// would cost four LDS reads per operand instead).  The Y row is 64 * steps bytes, steps = ceil(k * stride / 64); the X
// row carries (k - v) * stride zero bytes in front and behind, so the operand of offset d is the X row read
// (d + k - v) * stride bytes in.  The filter runs wherever k * stride <= 1024.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define HS_PCMP_MAX_ABS 1.2676506002282294e30 /* 2^100: the magnitude cap of an entry (hs_pssm_scan's) */
#define HS_PCMP_MAX_K 75                      /* columns of a profile at most (the index's k); an offset fits 8 bits */
#define HS_PCMP_MAX_ROW 1024                 /* bytes of a flattened profile the filter runs on */
#define HS_PCMP_TINY 1.1832913578315177e-271  /* 2^-900 */

struct hs_pcmp_shape {
  uint32_t stride;  // bytes of a column
  uint32_t steps;   // 64-byte depth steps of the Y row (0: the filter does not run on this shape)
  uint32_t lead;    // zero bytes in front of an X row: (k - v) * stride
  uint32_t xrow;    // bytes of an X row: 2 * lead + 64 * steps
  uint32_t yrow;    // bytes of a Y row: 64 * steps
  uint32_t n_off;   // offsets: 2 (k - v) + 1
};

__host__ __device__ inline hs_pcmp_shape hs_pcmp_shape_of(uint32_t k, uint32_t alphabet, uint32_t v) {
  hs_pcmp_shape sh;
  sh.stride = (alphabet + 15u) & ~15u;
  sh.steps = k * sh.stride <= HS_PCMP_MAX_ROW ? (k * sh.stride + 63u) / 64u : 0u;
  sh.lead = (k - v) * sh.stride;
  sh.yrow = 64u * sh.steps;
  sh.xrow = 2u * sh.lead + sh.yrow;
  sh.n_off = 2u * (k - v) + 1u;
  return sh;
}

// The depth steps of offset d (d = o - (k - v)) that meet the overlap: Y columns max(0, -d) .. min(k, k - d) - 1
__host__ __device__ inline void hs_pcmp_step_range(uint32_t k, uint32_t stride, int d, uint32_t* s_lo, uint32_t* s_hi) {
  const uint32_t p_lo = d < 0 ? (uint32_t)(-d) : 0u, p_hi = d > 0 ? k - (uint32_t)d : k;  // [p_lo, p_hi), never empty
  *s_lo = p_lo * stride / 64u;
  *s_hi = (p_hi * stride - 1u) / 64u + 1u;
}

// the MFMA depth steps of a 16 x 16 tile, summed over the offsets (hs_profile.pssm_cmp_steps)
__host__ __device__ inline uint64_t hs_pcmp_steps_issued(uint32_t k, uint32_t alphabet, uint32_t v) {
  const hs_pcmp_shape sh = hs_pcmp_shape_of(k, alphabet, v);
  uint64_t total = 0;
  if (!sh.steps) return 0;
  for (int d = -(int)(k - v); d <= (int)(k - v); ++d) {
    uint32_t lo, hi;
    hs_pcmp_step_range(k, sh.stride, d, &lo, &hi);
    total += hi - lo;
  }
  return total;
}

__host__ __device__ inline bool hs_pcmp_bad_value(double v, double max_abs) { return !(fabs(v) <= max_abs); }

// The order of a profile's l1 sum, one on the host and on the device: 64 partial sums, partial l over the entries l,
// l + 64, l + 128, ... ascending, combined by the butterfly p[i] = p[i] + p[i ^ w] for w = 32, 16, 8, 4, 2, 1
// (additions commute, so every slot ends with the same bits); then one inflation by 2^-40 > gamma_n for any order.
__host__ __device__ inline double hs_pcmp_l1_finish(double sum) { return sum + sum * 9.094947017729282e-13 /* 2^-40 */; }

struct hs_pcmp_par {
  double s, l1, amax;
};

// from amax and the butterfly's sum
__host__ __device__ inline hs_pcmp_par hs_pcmp_par_of(double amax, double sum) {
  hs_pcmp_par pr;
  pr.amax = amax;
  if (amax == 0.0) {
    pr.s = 0.0;
    pr.l1 = 0.0;
  } else if (amax < HS_PCMP_TINY) {
    pr.s = 0.0;
    pr.l1 = INFINITY;
  } else {
    pr.s = amax / 127.0;
    pr.l1 = hs_pcmp_l1_finish(sum);
  }
  return pr;
}

__host__ __device__ inline int hs_pcmp_code(double x, double s) { return s == 0.0 ? 0 : (int)rint(x / s); }

// The filter's test (the invariant above).  1: the pair goes to the exact pass.
__host__ __device__ inline int hs_pcmp_pass(int64_t I, double s_x, double l1_x, double amax_x, double s_y, double l1_y,
                                            uint32_t n, double t) {
  const double ss = s_x * s_y, c = ss * (double)I;
  const double E = (0.5 * s_x) * l1_y + (0.5 * s_y) * l1_x + (0.25 * (double)n) * ss;
  const double R = ((double)n * 2.220446049250313e-16) * (amax_x * l1_y);
  const double M = fabs(c) + E + R;
  const double ub = c + E + R + 9.094947017729282e-13 * M + 9.332636185032189e-302 /* 2^-1000 */;
  return !(ub < t);
}

// the rank of an offset in the tie order (|d|, d) ascending: 0, -1, +1, -2, +2, ...
__host__ __device__ inline uint32_t hs_pcmp_rank(int d) { return d < 0 ? 2u * (uint32_t)(-d) - 1u : 2u * (uint32_t)d; }

// ---- host: the exported functions' bodies (hs_capi_pssm.hip defines the symbols) ------------------------------------
// one profile's tables; q may be null
inline hs_pcmp_par hs_pcmp_tables_one(const double* x, uint32_t n, int8_t* q) {
  double part[64], amax = 0.0;
  for (int l = 0; l < 64; ++l) part[l] = 0.0;
  for (uint32_t i = 0; i < n; ++i) {
    const double a = fabs(x[i]);
    part[i & 63u] = part[i & 63u] + a;
    if (a > amax) amax = a;
  }
  for (int w = 32; w >= 1; w >>= 1) {
    double nx[64];
    for (int l = 0; l < 64; ++l) nx[l] = part[l] + part[l ^ w];
    for (int l = 0; l < 64; ++l) part[l] = nx[l];
  }
  const hs_pcmp_par pr = hs_pcmp_par_of(amax, part[0]);
  if (q)
    for (uint32_t i = 0; i < n; ++i) q[i] = (int8_t)hs_pcmp_code(x[i], pr.s);
  return pr;
}

// 0 ok, 1 a refused value
inline int hs_pssm_compare_tables_host(const double* X, uint64_t nx, uint32_t k, uint32_t alphabet, int8_t* q, double* s,
                                       double* l1, double* amax) {
  const uint32_t n = k * alphabet;
  for (uint64_t i = 0; i < nx * n; ++i)
    if (hs_pcmp_bad_value(X[i], HS_PCMP_MAX_ABS)) return 1;
  for (uint64_t m = 0; m < nx; ++m) {
    const hs_pcmp_par pr = hs_pcmp_tables_one(X + m * n, n, q ? q + m * n : nullptr);
    if (s) s[m] = pr.s;
    if (l1) l1[m] = pr.l1;
    if (amax) amax[m] = pr.amax;
  }
  return 0;
}

// The contract's score of one pair at one offset (the caller keeps d within -(k - 1) .. k - 1).  volatile-free: the
// build's -ffp-contract=off keeps every product and sum a rounded operation of its own.
__host__ __device__ inline double hs_pcmp_score(const double* x, const double* y, uint32_t k, uint32_t alphabet, int d) {
  const int p_lo = d < 0 ? -d : 0, p_hi = d > 0 ? (int)k - d : (int)k;
  double sc = 0.0;
  for (int p = p_lo; p < p_hi; ++p) {
    const double *xc = x + (size_t)(p + d) * alphabet, *yc = y + (size_t)p * alphabet;
    double col = 0.0;
    for (uint32_t r = 0; r < alphabet; ++r) {
      const double pr = xc[r] * yc[r];
      col = col + pr;
    }
    sc = sc + col;
  }
  return sc;
}

// best offset of a pair under the tie rule
inline double hs_pcmp_best(const double* x, const double* y, uint32_t k, uint32_t alphabet, uint32_t v, int* d_best) {
  double best = hs_pcmp_score(x, y, k, alphabet, 0);
  int bd = 0;
  for (int a = 1; a <= (int)(k - v); ++a)
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      const double sc = hs_pcmp_score(x, y, k, alphabet, sgn * a);
      if (sc > best) {
        best = sc;
        bd = sgn * a;
      }
    }
  *d_best = bd;
  return best;
}

// what hs_pssm_compare refuses from its arguments and values (Y null: self mode).  0 ok, 1 refused.
inline int hs_pcmp_refused(const double* X, uint64_t nx, const double* Y, uint64_t ny, uint32_t k, uint32_t alphabet,
                           const double* t, uint32_t v, const void* hit_x, const void* hit_y, const void* hit_d,
                           const void* hit_score, uint64_t cap) {
  if (k < 1 || k > HS_PCMP_MAX_K || alphabet < 1 || alphabet > 32 || v < 1 || v > k) return 1;
  if (nx >= (1ull << 27) || (Y && ny >= (1ull << 27))) return 1;
  if (Y && (nx == 0) != (ny == 0)) return 1;  // (self mode: ny is not looked at)
  if (nx && (!X || !t)) return 1;
  if (cap && (!hit_x || !hit_y || !hit_d || !hit_score)) return 1;
  return 0;
}

// 0 ok, 1 refused, 2 the hits exceed cap (*n_hits and cnt are valid)
inline int hs_pssm_compare_host_rule(const double* X, uint64_t nx, const double* Y, uint64_t ny, uint32_t k,
                                     uint32_t alphabet, const double* t, uint32_t v, uint32_t* hit_x, uint32_t* hit_y,
                                     int32_t* hit_d, double* hit_score, uint64_t cap, uint64_t* n_hits, uint64_t* cnt) {
  *n_hits = 0;
  if (hs_pcmp_refused(X, nx, Y, ny, k, alphabet, t, v, hit_x, hit_y, hit_d, hit_score, cap)) return 1;
  const size_t n = (size_t)k * alphabet;
  for (uint64_t i = 0; i < nx * n; ++i)
    if (hs_pcmp_bad_value(X[i], HS_PCMP_MAX_ABS)) return 1;
  for (uint64_t i = 0; Y && i < ny * n; ++i)
    if (hs_pcmp_bad_value(Y[i], HS_PCMP_MAX_ABS)) return 1;
  for (uint64_t m = 0; m < nx; ++m)
    if (hs_pcmp_bad_value(t[m], 1.7976931348623157e308)) return 1;
  const bool self = !Y;
  const double* const Yp = self ? X : Y;
  const uint64_t nyy = self ? nx : ny;
  uint64_t total = 0;  // hits are written while they fit; the count and cnt go on
  for (uint64_t x = 0; x < nx; ++x) {
    uint64_t c = 0;
    for (uint64_t y = self ? x + 1 : 0; y < nyy; ++y) {
      int d;
      const double best = hs_pcmp_best(X + x * n, Yp + y * n, k, alphabet, v, &d);
      if (!(best >= t[x])) continue;
      if (total < cap) {
        hit_x[total] = (uint32_t)x;
        hit_y[total] = (uint32_t)y;
        hit_d[total] = d;
        hit_score[total] = best;
      }
      ++total;
      ++c;
    }
    if (cnt) cnt[x] = c;
  }
  *n_hits = total;
  return total > cap ? 2 : 0;
}

// The column transform, out [nm][k][alphabet] (may be X itself).  Per column c of `a` entries, in this order:
//   mode 0: mean = (sum of c[r], r ascending, from +0.0) / a;  z[r] = c[r] - mean;   mode 1: z[r] = c[r];
//   norm = sqrt(sum of z[r] * z[r], r ascending, from +0.0);  out[r] = norm > 0 ? z[r] / norm : +0.0.
// A constant column has z = 0 and becomes zeros (mode 0); so does a column whose squares underflow.  0 ok, 1 refused.
inline int hs_pssm_compare_columns_host(const double* X, uint64_t nm, uint32_t k, uint32_t alphabet, int mode,
                                        double* out) {
  if (k < 1 || alphabet < 1 || (mode != 0 && mode != 1) || (nm && (!X || !out))) return 1;
  const uint64_t cols = nm * k;
  for (uint64_t i = 0; i < cols * alphabet; ++i)
    if (hs_pcmp_bad_value(X[i], HS_PCMP_MAX_ABS)) return 1;
  for (uint64_t c = 0; c < cols; ++c) {
    const double* const in = X + c * alphabet;
    double* const o = out + c * alphabet;
    double mean = 0.0;
    if (mode == 0) {
      double sum = 0.0;
      for (uint32_t r = 0; r < alphabet; ++r) sum = sum + in[r];
      mean = sum / (double)alphabet;
    }
    double ssq = 0.0;
    for (uint32_t r = 0; r < alphabet; ++r) {
      const double z = mode == 0 ? in[r] - mean : in[r];
      const double zz = z * z;
      ssq = ssq + zz;
    }
    const double norm = sqrt(ssq);
    for (uint32_t r = 0; r < alphabet; ++r) {
      const double z = mode == 0 ? in[r] - mean : in[r];
      o[r] = norm > 0.0 ? z / norm : 0.0;
    }
  }
  return 0;
}
