// hs_pssm_rank.h -- the rules of hs_pssm_rank (include/hsearch.h) as __host__ __device__ routines and on the host: the
// sample rule (hs_pssm_rank_plan_rule; the C symbol hs_pssm_rank_plan is it), which the driver, the kernels, the numpy
// reference and the tests share, and the order statistic itself over every (profile, k-mer) pair
// (hs_pssm_rank_scores_host; the C symbol hs_pssm_rank_scores).  Host-compilable: nothing here needs hipcc.
// Compile with -ffp-contract=off (the score is a chain of rounded sums; there is no product in it, so no compiler
// contracts anything, but the project's rule is one rule).
//
// THE ORDER is hs_pssm_topk.h's: a score is no NaN, no infinity and no -0.0, so the descending key hs_pssm_desc_key of
// its bits orders the scores, equal scores have equal keys, and the rank-th largest score is the rank-th smallest key.
// That argument needs only the 2^100 cap of an entry and the +0.0 start of the sum: it covers these scores unchanged.
//
// THE SAMPLE RULE, in integers.  n k-mers, a sample of n_s <= n of them, the wanted rank in 1 .. n:
//   q      = ceil(rank * n_s / n)              the rank's image in the sample (rank, n_s < 2^32: the product fits)
//   slack0 = 4 * ceil(sqrt(q)) + 8             four binomial deviations of the sample count, and a floor of 8
//   r_s(j) = q + slack0 * 4^j                  the sample rank of round j = 0, 1, ...
// r_s > n_s means "scan at -DBL_MAX": every k-mer is a hit and the round is final; the plan reports it as n_s + 1.
// n_s == n: the sample is the index, r_s = rank in every round and round 0 is final.
// The constant 8 and the sample's grain (one sample stands for n / n_s k-mers) make small ranks cost several times
// their size in hits: the 64 best and fewer are hs_pssm_topk's business.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "hs_pssm_topk.h"

#define HS_PSSM_RANK_MAX_ABS 1.2676506002282294e30 /* 2^100: hs_pssm_scan's cap of an entry (hs_pssm_tables.h) */

// ceil(sqrt(q)) in integers
__host__ __device__ inline uint64_t hs_pssm_rank_isqrt_up(uint64_t q) {
  uint64_t lo = 0, hi = 1ull << 32;  // lo^2 < q <= hi^2 (q = 0: hi walks down to 0)
  if (!q) return 0;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (mid * mid >= q)
      hi = mid;
    else
      lo = mid;
  }
  return hi;
}

// The sample rank of `round`.  Returns 0 and *sample_rank in 1 .. n_s + 1 (n_s + 1: beyond the sample, every k-mer);
// 1 for rank outside 1 .. n, n_s outside 1 .. n, n >= 2^32 or a null output, with nothing written.
__host__ __device__ inline int hs_pssm_rank_plan_rule(uint64_t rank, uint64_t n, uint64_t n_s, uint32_t round,
                                                 uint64_t* sample_rank) {
  if (!sample_rank || n >= (1ull << 32) || rank < 1 || rank > n || n_s < 1 || n_s > n) return 1;
  if (n_s == n) {
    *sample_rank = rank;
    return 0;
  }
  const uint64_t q = (rank * n_s + n - 1) / n;  // 1 .. n_s
  const uint64_t slack0 = 4 * hs_pssm_rank_isqrt_up(q) + 8;  // < 2^19
  // slack0 * 4^round, saturated: beyond round 16 it exceeds every n_s
  uint64_t r = n_s + 1;
  if (round <= 16) {
    const uint64_t add = slack0 << (2 * round);  // < 2^51
    if (add <= n_s && q + add <= n_s) r = q + add;
  }
  *sample_rank = r;
  return 0;
}

// ---- host: the exported function's body (hs_pssm_rank.hip defines the symbol) -------------------------------------
// Scores every (profile, k-mer) pair under hs_pssm_scan's contract and selects.  codes [n][k], S [nm][k][alphabet],
// rank [nm].  Returns 0; 1 for an argument the contract refuses (nothing is written then); 2 when memory ran out.
inline int hs_pssm_rank_scores_host(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet, const double* S,
                                    uint64_t nm, const uint64_t* rank, double* t_rank, uint64_t* cnt_ge,
                                    uint64_t* cnt_gt) {
  if (!k || !alphabet || alphabet > 32 || n >= (1ull << 32) || nm >= (1ull << 27)) return 1;
  if (n && !codes) return 1;
  if (nm && (!S || !rank || !t_rank || !cnt_ge || !cnt_gt)) return 1;
  const size_t ka = (size_t)k * alphabet;
  for (uint64_t i = 0; i < nm * ka; ++i) {
    const double a = S[i] < 0 ? -S[i] : S[i];
    if (!(a <= HS_PSSM_RANK_MAX_ABS)) return 1;
  }
  for (uint64_t m = 0; m < nm; ++m)
    if (rank[m] < 1 || rank[m] > n) return 1;  // (n == 0 refuses every rank)
  if (nm)
    for (uint64_t i = 0; i < n * k; ++i)
      if (codes[i] >= alphabet) return 1;
  try {
    std::vector<uint64_t> key(n), out_key(nm), ge(nm), gt(nm);
    for (uint64_t m = 0; m < nm; ++m) {
      const double* const Sm = S + m * ka;
      for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* const x = codes + i * k;
        double sc = 0.0;
        for (uint32_t p = 0; p < k; ++p) sc = sc + Sm[(size_t)p * alphabet + x[p]];
        uint64_t bits;
        memcpy(&bits, &sc, 8);
        key[i] = hs_pssm_desc_key(bits);
      }
      std::nth_element(key.begin(), key.begin() + (rank[m] - 1), key.end());
      const uint64_t w = key[rank[m] - 1];
      uint64_t below = 0, equal = 0;
      for (uint64_t i = 0; i < n; ++i) {
        below += key[i] < w;
        equal += key[i] == w;
      }
      out_key[m] = w;
      gt[m] = below;
      ge[m] = below + equal;
    }
    // everything is checked and computed: the outputs
    for (uint64_t m = 0; m < nm; ++m) {
      const uint64_t bits = hs_pssm_desc_bits(out_key[m]);
      memcpy(&t_rank[m], &bits, 8);
      cnt_ge[m] = ge[m];
      cnt_gt[m] = gt[m];
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}
