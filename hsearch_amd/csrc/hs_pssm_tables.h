// hs_pssm_tables.h -- the tables of the PSSM scan's FP6 filter (hs_pssm.hip), as __host__ __device__ routines: the
// device builds them in hs_pssm_prep_kernel, the host exports them (hs_pssm_tables) so that the invariant is tested
// where there is no GPU.  Host-compilable: nothing here needs hipcc.
//
// The contract's score of a k-mer x under a profile S [k][alphabet] is the ROUNDED sum fl(x) = S[0][x_0] + ... +
// S[k-1][x_{k-1}], left to right from +0.0 in fp64; (profile, x) is a hit iff fl(x) >= t.  The filter value is
//     F(x) = sum_p decode(code[p][x_p]),
// a sum of k e2m3 values (multiples of 1/8 within +-7.5), which fp32 accumulates exactly in any order.
//
// THE INVARIANT:  fl(x) >= t  =>  F(x) >= tau,   and   dead = 1 only if no x has fl(x) >= t.
//
// Proof, in the order the code goes (DESIGN.md section 21 has the long form).
//  (1) From the rounded sum to a real one.  Recursive summation of k doubles x_p obeys |fl - sum| <= gamma_{k-1}
//      sum |x_p| (gamma_m = m u / (1 - m u), u = 2^-53; additions have no underflow error, so this holds down to the
//      subnormals).  With T[p][a] >= S[p][a] + gamma_k |S[p][a]|, a hit has  sum_p T[p][x_p] >= t  over the REALS.
//      The slack is per ENTRY, not per profile: a "forbidden residue" of -10^30 inflates only the k-mers that use it.
//      hs_pssm_inflate computes T with g = (k + 2) 2^-52 > 2 gamma_k, which also covers its own two roundings.
//  (2) Offsets.  o[p] = max_a T[p][a], D[p][a] = T[p][a] - o[p] <= 0, gap G = sum_p o[p] - t.  A hit has
//      sum_p D[p][x_p] >= -G; every term is <= 0, so EACH term of a hit is >= -G.  U is an upper bound of G in fp64
//      (the rounding of the sum over o and of the subtraction are added to it).  U < 0: no k-mer hits -- dead.
//  (3) Scale.  lim = min(U, max |D|), s <= 15 / lim (14.5 / lim where lim = U: see the code).  value[p][a] = the
//      smallest e2m3 value v with v - 7.5 >= max(s D, -15).  Either s U <= 15, and a hit's terms s D >= -s G >= -15
//      are not clamped; or s max |D| <= 15 and nothing is clamped at all.  So for a hit F(x) >= s sum_p D + 7.5 k
//      >= 7.5 k - s G >= 7.5 k - s U, and tau is a multiple of 1/8 at or below that.  Every product and sum on the
//      way is moved to the safe side by an explicit margin (up_rel below), never by a rounding mode, and the grid
//      value is found by exact comparisons.
//  (4) Degenerate cases.  max |D| = 0 (a constant profile): s = 1, every value 7.5, F = 7.5 k for every x, and tau <=
//      7.5 k unless the profile is dead.  U = 0 with max |D| > 0 (t at the attainable maximum): lim = max |D|, tau <=
//      7.5 k, and only k-mers whose every entry rounds up to 7.5 pass.  s U beyond 2^20 (a threshold far below every
//      score, or a slack that swallows the range): tau = -infinity, the profile passes everything.  |t| > 2^108 is
//      decided without arithmetic: |fl| <= 75 * 2^100 * (1 + gamma) < 2^108, so such a t is dead or passes everything.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define HS_PSSM_MAX_ABS 1.2676506002282294e30 /* 2^100: the magnitude cap of an entry (keeps every partial sum finite) */
#define HS_PSSM_MAX_K 75                      /* positions of a profile at most (the index's k) */
#define HS_PSSM_STEP 128                      /* depth of one MFMA step */

// e2m3 value of a six-bit code, in eighths (the same map as hs_join6_tables.h)
__host__ __device__ inline int hs_pssm_e2m3_eighths(uint32_t c) {
  const int m = (int)(c & 7u), e = (int)((c >> 3) & 3u);
  const int v = e ? (8 + m) << (e - 1) : m;
  return (c & 32u) ? -v : v;
}
// code of the smallest e2m3 value v with v - 7.5 >= y, for y in [-15, 0].  The 63 grid values minus 7.5 are doubles,
// so every comparison is exact: no rounding stands between y and the grid.  Index i of the ascending grid: the
// negative codes 63 .. 33 (-7.5 .. -0.125), then 0 .. 31 (0 .. 7.5).
__host__ __device__ inline uint32_t hs_pssm_grid_code(int i) { return i < 31 ? (uint32_t)(63 - i) : (uint32_t)(i - 31); }
__host__ __device__ inline uint32_t hs_pssm_e2m3_ceil_m75(double y) {
  int lo = 0, hi = 62;  // the answer lies in [lo, hi]: value(62) - 7.5 = 0 >= y
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (0.125 * (double)hs_pssm_e2m3_eighths(hs_pssm_grid_code(mid)) - 7.5 >= y) hi = mid; else lo = mid + 1;
  }
  return hs_pssm_grid_code(lo);
}

// x moved away from no one: an upper bound of a real number whose fp64 image x carries a few roundings
__host__ __device__ inline double hs_pssm_up_rel(double x) { return x + fabs(x) * 8.881784197001252e-16 /* 2^-50 */; }

// T >= S + gamma_k |S| (step 1 of the proof).  g = (k + 2) 2^-52.
__host__ __device__ inline double hs_pssm_inflate(double S, double g) {
  if (S == 0.0) return 0.0;
  double e = g * fabs(S);
  if (e < 1e-290) e = 1e-290;  // (a product that underflowed: any positive margin is on the safe side)
  return S + e;
}

// per profile: what every entry's code needs
struct hs_pssm_prof {
  double s;      // scale
  double g;      // inflation factor of step 1
  float tau;     // threshold on the 1/8 grid; -inf: passes everything; +inf: dead
  uint32_t dead; // 1: no k-mer can hit
};

// One position of a profile: its offset o = max_a T[a] and the largest |T[a] - o| (both exact selections of doubles
// that every caller computes alike)
__host__ __device__ inline void hs_pssm_position(const double* Srow, uint32_t alphabet, double g, double* o_out,
                                                 double* dmax_out) {
  double o = hs_pssm_inflate(Srow[0], g);
  for (uint32_t a = 1; a < alphabet; ++a) o = fmax(o, hs_pssm_inflate(Srow[a], g));
  double dmax = 0.0;
  for (uint32_t a = 0; a < alphabet; ++a) dmax = fmax(dmax, fabs(hs_pssm_inflate(Srow[a], g) - o));
  *o_out = o;
  *dmax_out = dmax;
}
__host__ __device__ inline double hs_pssm_g(uint32_t k) { return (double)(k + 2u) * 2.220446049250313e-16; }  // (k + 2) 2^-52

// The profile's parameters from its offsets o [k] (summed HERE, left to right: one order on the host and on the
// device), the largest |D| over all entries, and t.  Inputs are finite and |S| <= 2^100 (the callers check).
__host__ __device__ inline void hs_pssm_finish(const double* o, double dmax, double t, uint32_t k, hs_pssm_prof* out) {
  const double g = hs_pssm_g(k);
  out->g = g;
  out->s = 1.0;
  out->dead = 0;
  const double BIG = 3.2451855365842673e32;  // 2^108
  if (t > BIG) {
    out->dead = 1;
    out->tau = INFINITY;
    return;
  }
  if (t < -BIG) {
    out->tau = -INFINITY;
    return;
  }
  double so = 0.0, sabs = 0.0;
  for (uint32_t p = 0; p < k; ++p) {
    so += o[p];
    sabs += fabs(o[p]);
  }
  dmax = hs_pssm_up_rel(dmax);  // >= every real |D|
  // U >= sum_p o[p] - t over the reals: the k - 1 roundings of so are within g * sabs, the subtraction and the
  // addition within up_rel
  const double U = hs_pssm_up_rel((so - t) + (g * hs_pssm_up_rel(sabs) + 1e-290));
  if (U < 0.0) {
    out->dead = 1;
    out->tau = INFINITY;
    return;
  }
  const bool by_gap = U > 0.0 && U < dmax;
  const double lim = by_gap ? U : dmax;
  double s = 1.0;
  if (lim > 0.0) {
    // s * lim <= 15 over the reals; 14.5 where entries clamp, so that ONE clamped entry beside k - 1 perfect ones
    // (7.5 k - 15) stays below tau (7.5 k - 14.5): a forbidden residue rejects, whatever the rest of the k-mer is
    s = ((by_gap ? 14.5 : 15.0) / lim) * (1.0 - 8.881784197001252e-16);
    if (s > 1e250) s = 1e250;  // (a smaller scale is always legal)
  }
  out->s = s;
  const double w = hs_pssm_up_rel(s * U) + 9.094947017729282e-13;  // >= s U; + 2^-40
  if (!(w <= 1048576.0)) {
    out->tau = -INFINITY;
    return;
  }
  // 7.5 k - w carries one rounding of at most 2^-32; 2^-30 below it, then down to the grid
  const double tau8 = floor((7.5 * (double)k - w - 9.313225746154785e-10) * 8.0);
  out->tau = (float)(tau8 * 0.125);  // |tau8| <= 2^24: exact in fp32
}

// the six-bit code of one entry S[p][a] given the profile's parameters and the position's offset o[p]
__host__ __device__ inline uint32_t hs_pssm_entry_code(double S, double o, const hs_pssm_prof* pr) {
  const double d = hs_pssm_inflate(S, pr->g) - o;  // <= 0; one rounding
  double y = pr->s * d;                             // <= 0; a second one
  y = y * (1.0 - 8.881784197001252e-16);            // towards zero by 2^-50: >= s D over the reals
  if (!(y >= -15.0)) y = -15.0;
  if (y > 0.0) y = 0.0;
  return hs_pssm_e2m3_ceil_m75(y);
}
// MFMA depth steps of a profile
__host__ __device__ inline uint32_t hs_pssm_steps(uint32_t k, uint32_t alphabet) {
  return (k * alphabet + HS_PSSM_STEP - 1) / HS_PSSM_STEP;
}

// an entry the contract refuses: NaN, infinite, or beyond 2^100 (thresholds: NaN or infinite only -- max_abs = inf)
__host__ __device__ inline bool hs_pssm_bad_value(double v, double max_abs) { return !(fabs(v) <= max_abs) ; }

// ---- host: the exported function's body (hs_capi_pssm.hip defines the symbol) ---------------------------------------
// code [nm][k][alphabet] six-bit e2m3 codes, tau [nm] (+-infinity as above), dead [nm].  Returns 0, or 1 for an
// argument the contract refuses (nothing is written then).
inline int hs_pssm_tables_host(const double* S, const double* t, uint64_t nm, uint32_t k, uint32_t alphabet,
                               uint8_t* code, double* tau, uint8_t* dead) {
  if (k < 1 || k > 75 || alphabet < 1 || alphabet > 32 || nm >= (1ull << 27)) return 1;
  if (nm && (!S || !t)) return 1;
  const uint64_t ka = (uint64_t)k * alphabet;
  for (uint64_t i = 0; i < nm * ka; ++i)
    if (hs_pssm_bad_value(S[i], HS_PSSM_MAX_ABS)) return 1;
  for (uint64_t m = 0; m < nm; ++m)
    if (hs_pssm_bad_value(t[m], 1.7976931348623157e308)) return 1;
  for (uint64_t m = 0; m < nm; ++m) {
    hs_pssm_prof pr;
    const double* Sm = S + m * ka;
    double o[HS_PSSM_MAX_K], dmax = 0.0;
    for (uint32_t p = 0; p < k; ++p) {
      double d = 0.0;
      hs_pssm_position(Sm + (uint64_t)p * alphabet, alphabet, hs_pssm_g(k), &o[p], &d);
      dmax = fmax(dmax, d);
    }
    hs_pssm_finish(o, dmax, t[m], k, &pr);
    if (tau) tau[m] = (double)pr.tau;
    if (dead) dead[m] = (uint8_t)pr.dead;
    if (code)
      for (uint32_t p = 0; p < k; ++p)
        for (uint32_t a = 0; a < alphabet; ++a)
          code[m * ka + (uint64_t)p * alphabet + a] =
              (pr.dead || pr.tau == -INFINITY) ? (uint8_t)0 : (uint8_t)hs_pssm_entry_code(Sm[p * alphabet + a], o[p], &pr);
  }
  return 0;
}
