// hs_pssm_null.h -- the rule of hs_pssm_pvalue / hs_pssm_pvalue_threshold (include/hsearch.h) as __host__ __device__
// routines: the kernels of hs_pssm_null.hip build their tables through them, the host exports them
// (hs_pssm_null_tables, hs_pssm_pvalue_host, hs_pssm_threshold_host) so that the invariant is tested where there is no
// GPU.  Host-compilable: nothing here needs hipcc.  Compile with -ffp-contract=off: every product and sum below is
// rounded to fp64 on its own.
//
// The null model: positions independent, residue a with weight bg[a] (0 <= bg[a] <= 1, not renormalised).  P is the
// product measure of bg over the alphabet^k k-mers; fl(x) is the contract's score of hs_pssm_tables.h (the rounded
// sum, left to right from +0.0).
//
// THE INVARIANT:  for every t,   p_lo(t) <= P{ x : fl(x) >= t } <= p_hi(t).
// (For t below the grid, J_hi >= B, the rule answers p_hi = 1: that is "not computed", and it bounds P exactly when the
// total mass (sum bg)^k is at most 1.  Everywhere else the bound holds for any bg the rule accepts.)
//
// Proof, in the order the code goes (DESIGN.md section 26 has the long form).  u = 2^-53, g = hs_pssm_g(k) = (k + 2)
// 2^-52, B = bins.
//  (1) Two-sided entries.  T+ = hs_pssm_inflate(S, g) >= S + gamma_k |S| and T- = hs_pssm_deflate(S, g) = -inflate(-S)
//      <= S - gamma_k |S|.  |fl(x) - sum_p S[p][x_p]| <= gamma_{k-1} sum |S| (step (1) of hs_pssm_tables.h), so over the
//      REALS   sum_p T-[p][x_p] >= t  =>  fl(x) >= t  =>  sum_p T+[p][x_p] >= t.
//  (2) Deficits.  Per side o[p] = max_a T[p][a] (an exact selection), D[p][a] = o[p] - T[p][a] >= 0, O = sum_p o[p]:
//      sum_p T[p][x_p] >= t  <=>  sum_p D[p][x_p] <= O - t.  A forbidden residue of -10^30 is a huge deficit of its own
//      entry; O, and with it the grid, is made of the maxima only.
//  (3) The gap, both ways (hs_pssm_null_gap_hi / _lo).  so = the left-to-right fp64 sum of o[p], c = g * up(sum |o[p]|)
//      + 1e-290 >= |so - O| (as hs_pssm_finish bounds it).  G_hi(t) = up((so+ - t) + c+) >= O+ - t and G_lo(t) =
//      down((so- - t) - c-) <= O- - t, where up(x) = x + |x| 2^-50 and down(x) = x - |x| 2^-50 cover the two roundings
//      inside.  Every step is a monotone function of t.
//  (4) The grid.  span = G_hi(t_lo) (t_lo raised to -2^108, below every score); span < 0: no k-mer reaches t_lo, the
//      profile is DEAD, and delta = 1 (any positive delta keeps the proof; G_hi(t) < 0 for every t >= t_lo then gives
//      p_hi = 0).  Else delta = max((span / (B - 1)) (1 + 2^-48), 1e-300) >= (O+ - t_lo) / (B - 1).
//  (5) Bins.  q_dn = floor((fl(D+) / delta) (1 - 2^-50)) <= D+ / delta and q_up = ceil((fl(D-) / delta) (1 + 2^-50)) >=
//      D- / delta over the reals: the subtraction, the division and the product are three roundings, 3u < 2^-50; a
//      quotient that underflows is below 1, where floor gives 0 (safe) and q_up is set to at least 1 for D- > 0 (safe).
//      Both saturate at B: sum_p q <= j <= B - 1 cannot hold with one q >= B, so saturation changes no bin j < B.
//  (6) Lookup indices.  J_hi(t) = floor((G_hi / delta)(1 + 2^-50)) >= floor((O+ - t) / delta) and J_lo(t) = floor((G_lo /
//      delta)(1 - 2^-50)) <= (O- - t) / delta for G_lo >= 0; a negative gap means no k-mer (J = -1).  Then
//        sum D+ <= O+ - t  =>  sum q_dn delta <= O+ - t  =>  sum q_dn <= J_hi            (integers)
//        sum q_up <= J_lo  =>  sum D- <= sum q_up delta <= J_lo delta <= O- - t.
//      So  P{sum q_up <= min(J_lo, B - 1)} <= P{fl >= t} <= P{sum q_dn <= J_hi}: the two distributions' cdfs.  J_hi >= B
//      is off the grid (t < t_lo): p_hi = 1.  At t = t_lo, (span / delta)(1 + 2^-50) < B - 1, so J_hi <= B - 2 there.
//  (7) The distribution (hs_pssm_null_conv_host, hs_pssm_null_conv_kernel: the same operations in the same order).
//      pdf_{p+1}[j] = sum over a ascending of bg[a] * pdf_p[j - q[p][a]], from +0.0; mass beyond bin B - 1 is dropped,
//      which no bin below it sees as q >= 0.  cdf[j] = base[j >> 6] + run[j] as the issue defines it.  Every term is
//      >= 0, so the computed value carries a relative error of at most gamma_n, n the roundings on the longest path: per
//      position one product and at most alphabet - 1 sums (the sum onto +0.0 is exact), then 63 sums of a run, at most
//      127 of the bases, and one more: n <= k * alphabet + 191.  Products may underflow: each loses at most 2^-1075
//      absolutely, and at most k * alphabet * B < 2^25 products feed one bin, so the absolute part is below 2^-1050.
//  (8) Margins.  e = (n' + 2) 2^-52 with n' = k (alphabet + 1) + 200 >= n, so e >= 2 gamma_n + 2u; 1 + e and 1 - e are
//      doubles.  p_hi = cdf_dn[J_hi] (1 + e) + 1e-300 and p_lo = max(0, cdf_up[J_lo] (1 - e) - 1e-300): the product and
//      the sum are two more roundings (2u), the relative part of (7) takes (n + 1) u, and 1e-300 / 2 > 2^-1049 takes the
//      absolute part.  No margin comes from a rounding mode.
//  (9) Monotone.  cdf[] ascends (fp64 sums of non-negative terms are monotone, and base[b + 1] = cdf[64 b + 63]), J_hi
//      and J_lo descend in t by (3) and (6), so p_hi and p_lo descend in t.
//
// THE THRESHOLD of a p-value p in (0, 1]:  J* = the largest J in 0 .. B - 1 with cdf_dn[J] (1 + e) + 1e-300 <= p (the
// ladder ascends: a binary search).  None: t_p = +DBL_MAX, flag 2.  J* = B - 1: t_p = t_lo, flag 1 (clipped).  Else t_p
// = the smallest double t with J_hi(t) <= J*, by bisection over hs_pssm_topk.h's ordered keys (J_hi descends in t;
// -0.0 is returned as +0.0, which has the same J_hi), flag 0: p_hi(t_p) <= p and p_hi of the next double below exceeds p.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "hs_pssm_tables.h"
#include "hs_pssm_topk.h"

#define HS_PSSM_NULL_MIN_BINS 64
#define HS_PSSM_NULL_MAX_BINS 8192
#define HS_PSSM_NULL_TINY 1e-300                   /* the absolute margin of step (8) */
#define HS_PSSM_NULL_UP (1.0 + 8.881784197001252e-16)   /* 1 + 2^-50 */
#define HS_PSSM_NULL_DOWN (1.0 - 8.881784197001252e-16) /* 1 - 2^-50 */
#define HS_PSSM_NULL_BIG 3.2451855365842673e32     /* 2^108: above every |score| */

// T- <= S - gamma_k |S| (step 1): the mirror image of hs_pssm_inflate
__host__ __device__ inline double hs_pssm_deflate(double S, double g) {
  if (S == 0.0) return 0.0;
  double e = g * fabs(S);
  if (e < 1e-290) e = 1e-290;
  return S - e;
}

// what a lookup needs of one profile (48 bytes; the device keeps one per profile of the call)
struct hs_pssm_null_prof {
  double so_hi, c_hi;  // the + side: the rounded sum of the offsets and the bound of its error
  double so_lo, c_lo;  // the - side
  double delta;        // width of a bin
  uint32_t dead;       // 1: no k-mer reaches t_lo
  uint32_t pad;
};

// e of step (8)
__host__ __device__ inline double hs_pssm_null_e(uint32_t k, uint32_t alphabet) {
  return (double)(k * (alphabet + 1u) + 202u) * 2.220446049250313e-16;
}

// bg the rule accepts: every entry finite and in 0 .. 1, one positive
__host__ __device__ inline bool hs_pssm_null_bg_ok(const double* bg, uint32_t alphabet) {
  bool pos = false;
  for (uint32_t a = 0; a < alphabet; ++a) {
    if (!(bg[a] >= 0.0 && bg[a] <= 1.0)) return false;
    pos = pos || bg[a] > 0.0;
  }
  return pos;
}
__host__ __device__ inline bool hs_pssm_null_p_ok(double p) { return p > 0.0 && p <= 1.0; }

// one position's offset on either side (side 0: +, 1: -)
__host__ __device__ inline double hs_pssm_null_offset(const double* Srow, uint32_t alphabet, double g, int side) {
  double o = side ? hs_pssm_deflate(Srow[0], g) : hs_pssm_inflate(Srow[0], g);
  for (uint32_t a = 1; a < alphabet; ++a)
    o = fmax(o, side ? hs_pssm_deflate(Srow[a], g) : hs_pssm_inflate(Srow[a], g));
  return o;
}

// steps (3): the gaps.  Neither returns a NaN: beyond +-1e300 (an infinite t) the sign alone is handed on.
__host__ __device__ inline double hs_pssm_null_gap_hi(const hs_pssm_null_prof* pr, double t) {
  const double g0 = (pr->so_hi - t) + pr->c_hi;
  if (!(g0 < 1e300)) return 1e300;
  if (!(g0 > -1e300)) return -1e300;
  return g0 + fabs(g0) * 8.881784197001252e-16;
}
__host__ __device__ inline double hs_pssm_null_gap_lo(const hs_pssm_null_prof* pr, double t) {
  const double g0 = (pr->so_lo - t) - pr->c_lo;
  if (!(g0 < 1e300)) return 1e300;
  if (!(g0 > -1e300)) return -1e300;
  return g0 - fabs(g0) * 8.881784197001252e-16;
}

// step (6).  J_hi in -1 .. B (B: off the grid), J_lo in -1 .. B - 1
__host__ __device__ inline int32_t hs_pssm_null_jhi(const hs_pssm_null_prof* pr, uint32_t B, double t) {
  const double G = hs_pssm_null_gap_hi(pr, t);
  if (G < 0.0) return -1;
  const double x = (G / pr->delta) * HS_PSSM_NULL_UP;
  if (!(x < (double)B)) return (int32_t)B;
  return (int32_t)x;  // (x >= 0: the cast is the floor)
}
__host__ __device__ inline int32_t hs_pssm_null_jlo(const hs_pssm_null_prof* pr, uint32_t B, double t) {
  const double G = hs_pssm_null_gap_lo(pr, t);
  if (G < 0.0) return -1;
  const double x = (G / pr->delta) * HS_PSSM_NULL_DOWN;
  if (!(x < (double)B)) return (int32_t)B - 1;
  return (int32_t)x;
}

// steps (3), (4): the profile's parameters.  S [k][alphabet] checked by the caller, t_lo finite.
__host__ __device__ inline void hs_pssm_null_profile(const double* S, uint32_t k, uint32_t alphabet, double t_lo,
                                                     uint32_t B, hs_pssm_null_prof* out) {
  const double g = hs_pssm_g(k);
  for (int side = 0; side < 2; ++side) {
    double so = 0.0, sabs = 0.0;
    for (uint32_t p = 0; p < k; ++p) {
      const double o = hs_pssm_null_offset(S + (size_t)p * alphabet, alphabet, g, side);
      so += o;
      sabs += fabs(o);
    }
    const double c = g * hs_pssm_up_rel(sabs) + 1e-290;
    if (side) {
      out->so_lo = so;
      out->c_lo = c;
    } else {
      out->so_hi = so;
      out->c_hi = c;
    }
  }
  const double span = hs_pssm_null_gap_hi(out, t_lo < -HS_PSSM_NULL_BIG ? -HS_PSSM_NULL_BIG : t_lo);
  out->pad = 0;
  if (span < 0.0) {
    out->dead = 1;
    out->delta = 1.0;
    return;
  }
  out->dead = 0;
  const double d = (span / (double)(B - 1u)) * (1.0 + 3.552713678800501e-15) /* 1 + 2^-48 */;
  out->delta = d > HS_PSSM_NULL_TINY ? d : HS_PSSM_NULL_TINY;
}

// step (5): one entry's bin shift on either side, 0 .. B.  o: the position's offset of that side.
__host__ __device__ inline uint32_t hs_pssm_null_q(double S, double o, double g, double delta, uint32_t B, int side) {
  const double d = o - (side ? hs_pssm_deflate(S, g) : hs_pssm_inflate(S, g));  // >= 0
  if (!side) {
    const double x = (d / delta) * HS_PSSM_NULL_DOWN;
    if (!(x < (double)B)) return B;
    return (uint32_t)x;  // floor
  }
  const double x = (d / delta) * HS_PSSM_NULL_UP;
  if (!(x <= (double)B)) return B;
  uint32_t q = (uint32_t)x;  // floor; x <= B
  if ((double)q < x) ++q;    // ceil (q <= B still: x <= B)
  if (q == 0 && d > 0.0) q = 1;
  return q;
}

// step (8)
__host__ __device__ inline double hs_pssm_null_ladder_hi(double c, double e) { return c * (1.0 + e) + HS_PSSM_NULL_TINY; }
__host__ __device__ inline double hs_pssm_null_ladder_lo(double c, double e) {
  const double v = c * (1.0 - e) - HS_PSSM_NULL_TINY;
  return v > 0.0 ? v : 0.0;
}

// the lookup of one threshold.  cdf_up and p_lo may be null (the upper side alone).
__host__ __device__ inline void hs_pssm_null_lookup(const hs_pssm_null_prof* pr, uint32_t B, double e,
                                                    const double* cdf_dn, const double* cdf_up, double t, double* p_hi,
                                                    double* p_lo) {
  const int32_t jh = hs_pssm_null_jhi(pr, B, t);
  *p_hi = jh >= (int32_t)B ? 1.0 : jh < 0 ? 0.0 : hs_pssm_null_ladder_hi(cdf_dn[jh], e);
  if (p_lo && cdf_up) {
    const int32_t jl = hs_pssm_null_jlo(pr, B, t);
    *p_lo = jl < 0 ? 0.0 : hs_pssm_null_ladder_lo(cdf_up[jl], e);
  }
}

// THE THRESHOLD.  flag 0: exact on the grid, 1: clipped at t_lo, 2: nothing admissible
__host__ __device__ inline void hs_pssm_null_threshold(const hs_pssm_null_prof* pr, uint32_t B, double e,
                                                       const double* cdf_dn, double t_lo, double p, double* t_p,
                                                       uint32_t* flag) {
  if (!(hs_pssm_null_ladder_hi(cdf_dn[0], e) <= p)) {
    *t_p = 1.7976931348623157e308;
    *flag = 2;
    return;
  }
  uint32_t lo = 0, hi = B;  // ladder(lo) <= p; hi == B or ladder(hi) > p
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (hs_pssm_null_ladder_hi(cdf_dn[mid], e) <= p)
      lo = mid;
    else
      hi = mid;
  }
  if (lo == B - 1) {
    *t_p = t_lo;
    *flag = 1;
    return;
  }
  const int32_t Js = (int32_t)lo;
  // the ordered keys of -DBL_MAX .. +DBL_MAX; J_hi(+DBL_MAX) = -1 <= J*
  uint64_t klo = hs_pssm_order_key(0xffefffffffffffffull), khi = hs_pssm_order_key(0x7fefffffffffffffull);
  while (klo < khi) {  // the smallest key whose double has J_hi <= J*
    const uint64_t mid = klo + (khi - klo) / 2;
    const uint64_t bits = hs_pssm_order_bits(mid);
    double t;
    memcpy(&t, &bits, 8);
    if (hs_pssm_null_jhi(pr, B, t) <= Js)
      khi = mid;
    else
      klo = mid + 1;
  }
  const uint64_t bits = hs_pssm_order_bits(klo);
  double t;
  memcpy(&t, &bits, 8);
  *t_p = t == 0.0 ? 0.0 : t;
  *flag = 0;
}

// ---- host: the exported functions' bodies (hs_capi_pssm.hip defines the symbols) ---------------------------------
// step (7) for one (profile, side): q [k][alphabet], cdf [B]; a, b: scratch of B doubles each
inline void hs_pssm_null_conv_host(const uint16_t* q, const double* bg, uint32_t k, uint32_t alphabet, uint32_t B,
                                   double* a, double* b, double* cdf) {
  double *cur = a, *nxt = b;
  for (uint32_t j = 0; j < B; ++j) cur[j] = 0.0;
  cur[0] = 1.0;
  for (uint32_t p = 0; p < k; ++p) {
    const uint16_t* const qr = q + (size_t)p * alphabet;
    for (uint32_t j = 0; j < B; ++j) {
      double acc = 0.0;
      for (uint32_t r = 0; r < alphabet; ++r)
        if (qr[r] <= j) acc = acc + bg[r] * cur[j - qr[r]];
      nxt[j] = acc;
    }
    double* const s = cur;
    cur = nxt;
    nxt = s;
  }
  double base = 0.0;
  for (uint32_t b0 = 0; b0 < B; b0 += 64) {
    double run = 0.0;
    for (uint32_t j = b0; j < b0 + 64 && j < B; ++j) {
      run = j == b0 ? cur[j] : run + cur[j];
      cdf[j] = base + run;
    }
    base = base + run;  // (the last block's is not used)
  }
}

// the checks every host form shares.  Returns 0 or 1.
inline int hs_pssm_null_args_bad(const double* S, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                 const double* t_lo, uint32_t bins) {
  if (k < 1 || k > HS_PSSM_MAX_K || alphabet < 1 || alphabet > 32 || nm >= (1ull << 27)) return 1;
  if (bins < HS_PSSM_NULL_MIN_BINS || bins > HS_PSSM_NULL_MAX_BINS) return 1;
  if (!nm) return 0;
  if (!S || !bg) return 1;
  const uint64_t ka = (uint64_t)k * alphabet;
  for (uint64_t i = 0; i < nm * ka; ++i)
    if (hs_pssm_bad_value(S[i], HS_PSSM_MAX_ABS)) return 1;
  if (!hs_pssm_null_bg_ok(bg, alphabet)) return 1;
  for (uint64_t m = 0; t_lo && m < nm; ++m)
    if (hs_pssm_bad_value(t_lo[m], 1.7976931348623157e308)) return 1;
  return 0;
}

// one profile's tables into q_dn / q_up [k][alphabet] and cdf_dn / cdf_up [B] (cdf_up may be null: not built)
inline void hs_pssm_null_one_host(const double* Sm, uint32_t k, uint32_t alphabet, const double* bg, double t_lo,
                                  uint32_t B, hs_pssm_null_prof* pr, uint16_t* q_dn, uint16_t* q_up, double* scratch,
                                  double* cdf_dn, double* cdf_up) {
  const double g = hs_pssm_g(k);
  hs_pssm_null_profile(Sm, k, alphabet, t_lo, B, pr);
  for (uint32_t p = 0; p < k; ++p) {
    const double* const row = Sm + (size_t)p * alphabet;
    const double oh = hs_pssm_null_offset(row, alphabet, g, 0), ol = hs_pssm_null_offset(row, alphabet, g, 1);
    for (uint32_t a = 0; a < alphabet; ++a) {
      q_dn[p * alphabet + a] = (uint16_t)hs_pssm_null_q(row[a], oh, g, pr->delta, B, 0);
      q_up[p * alphabet + a] = (uint16_t)hs_pssm_null_q(row[a], ol, g, pr->delta, B, 1);
    }
  }
  hs_pssm_null_conv_host(q_dn, bg, k, alphabet, B, scratch, scratch + B, cdf_dn);
  if (cdf_up) hs_pssm_null_conv_host(q_up, bg, k, alphabet, B, scratch, scratch + B, cdf_up);
}

// Returns 0; 1 for an argument the rule refuses (nothing is written then); 2 when memory ran out.
inline int hs_pssm_null_tables_host(const double* S, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                    const double* t_lo, uint32_t bins, uint16_t* q_dn, uint16_t* q_up, double* delta,
                                    uint8_t* dead, double* cdf_dn, double* cdf_up) {
  if (hs_pssm_null_args_bad(S, nm, k, alphabet, bg, t_lo, bins)) return 1;
  try {
    const size_t ka = (size_t)k * alphabet;
    std::vector<uint16_t> qd(ka), qu(ka);
    std::vector<double> scratch(2 * (size_t)bins), cd(bins), cu(bins);
    for (uint64_t m = 0; m < nm; ++m) {
      hs_pssm_null_prof pr;
      hs_pssm_null_one_host(S + m * ka, k, alphabet, bg, t_lo ? t_lo[m] : 0.0, bins, &pr, qd.data(), qu.data(),
                            scratch.data(), cdf_dn ? cd.data() : scratch.data(), cdf_up ? cu.data() : nullptr);
      if (delta) delta[m] = pr.delta;
      if (dead) dead[m] = (uint8_t)pr.dead;
      for (size_t i = 0; i < ka; ++i) {
        if (q_dn) q_dn[m * ka + i] = qd[i];
        if (q_up) q_up[m * ka + i] = qu[i];
      }
      for (uint32_t j = 0; j < bins; ++j) {
        if (cdf_dn) cdf_dn[m * bins + j] = cd[j];
        if (cdf_up) cdf_up[m * bins + j] = cu[j];
      }
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}

// the p-value bracket of n hits (hit_m, hit_score) in any order; p_lo may be null
inline int hs_pssm_pvalue_host_rule(const double* S, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                    const double* t_lo, uint32_t bins, const uint32_t* hit_m, const double* hit_score,
                                    uint64_t n, double* p_hi, double* p_lo) {
  if (hs_pssm_null_args_bad(S, nm, k, alphabet, bg, t_lo, bins)) return 1;
  if (n && (!hit_m || !hit_score || !p_hi)) return 1;
  for (uint64_t i = 0; i < n; ++i)
    if (hit_m[i] >= nm || hit_score[i] != hit_score[i]) return 1;
  if (!n) return 0;
  try {
    const size_t ka = (size_t)k * alphabet;
    const double e = hs_pssm_null_e(k, alphabet);
    std::vector<uint16_t> qd(ka), qu(ka);
    std::vector<double> scratch(2 * (size_t)bins), cd(bins), cu(bins);
    std::vector<uint8_t> used(nm, 0);
    for (uint64_t i = 0; i < n; ++i) used[hit_m[i]] = 1;
    std::vector<double> hi(n), lo(p_lo ? n : 0);
    for (uint64_t m = 0; m < nm; ++m) {
      if (!used[m]) continue;
      hs_pssm_null_prof pr;
      hs_pssm_null_one_host(S + m * ka, k, alphabet, bg, t_lo ? t_lo[m] : 0.0, bins, &pr, qd.data(), qu.data(),
                            scratch.data(), cd.data(), p_lo ? cu.data() : nullptr);
      for (uint64_t i = 0; i < n; ++i)
        if (hit_m[i] == m)
          hs_pssm_null_lookup(&pr, bins, e, cd.data(), p_lo ? cu.data() : nullptr, hit_score[i], &hi[i],
                              p_lo ? &lo[i] : nullptr);
    }
    for (uint64_t i = 0; i < n; ++i) {
      p_hi[i] = hi[i];
      if (p_lo) p_lo[i] = lo[i];
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}

// the threshold of p [nm] per profile, and the bracket at it; p_lo may be null
inline int hs_pssm_threshold_host_rule(const double* S, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                       const double* t_lo, uint32_t bins, const double* p, double* t_p, double* p_hi,
                                       double* p_lo, uint32_t* flag) {
  if (hs_pssm_null_args_bad(S, nm, k, alphabet, bg, t_lo, bins)) return 1;
  if (nm && (!p || !t_p || !p_hi || !flag)) return 1;
  for (uint64_t m = 0; m < nm; ++m)
    if (!hs_pssm_null_p_ok(p[m])) return 1;
  try {
    const size_t ka = (size_t)k * alphabet;
    const double e = hs_pssm_null_e(k, alphabet);
    std::vector<uint16_t> qd(ka), qu(ka);
    std::vector<double> scratch(2 * (size_t)bins), cd(bins), cu(bins), tp(nm), hi(nm), lo(nm, 0.0);
    std::vector<uint32_t> fl(nm);
    for (uint64_t m = 0; m < nm; ++m) {
      hs_pssm_null_prof pr;
      const double tl = t_lo ? t_lo[m] : 0.0;
      hs_pssm_null_one_host(S + m * ka, k, alphabet, bg, tl, bins, &pr, qd.data(), qu.data(), scratch.data(), cd.data(),
                            p_lo ? cu.data() : nullptr);
      hs_pssm_null_threshold(&pr, bins, e, cd.data(), tl, p[m], &tp[m], &fl[m]);
      hs_pssm_null_lookup(&pr, bins, e, cd.data(), p_lo ? cu.data() : nullptr, tp[m], &hi[m], p_lo ? &lo[m] : nullptr);
    }
    for (uint64_t m = 0; m < nm; ++m) {
      t_p[m] = tp[m];
      p_hi[m] = hi[m];
      if (p_lo) p_lo[m] = lo[m];
      flag[m] = fl[m];
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}
