// hs_pssm_topk.h -- the order of hs_pssm_topk's rows (include/hsearch.h) as __host__ __device__ routines, and the rule
// itself on the host (hs_pssm_topk_hits).  The kernels of hs_pssm_topk.hip and the host rule share the transform.
// Host-compilable: nothing here needs hipcc.
//
// THE ORDER.  Row m holds the best k-mers under (score descending, id ascending).  It is strict and total:
//  (1) A score is never a NaN or an infinity: every entry is within 2^100 (the callers check), so the at most 75 partial
//      sums stay below 2^107.
//  (2) A score is never -0.0: the sum starts at +0.0, and round-to-nearest gives -0.0 only from two -0.0 operands
//      ((+0) + (-0) = +0, x + (-x) = +0).  So equal doubles have equal bits and `==` on the bits is `==` on the scores.
//  (3) For such doubles  u = bits ^ (sign ? ~0 : 1 << 63)  is monotone: positive doubles order like their bits and
//      get the top bit set; negative doubles order against their bits and are complemented below them.  So u orders
//      like the doubles, ~u is the DESCENDING key, and (~u, id) ascending is the row's order.  Ids within a profile
//      are distinct, so no two entries of a row compare equal.
//  (4) ~u = all ones would need u = 0: sign set and all other bits set, a NaN.  No score has it: it is the padding
//      key, above every real one.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <new>
#include <vector>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define HS_PSSM_TOPK_PAD 0xffffffffffffffffull /* the descending key of no score (4) */

// bits of a double that is no NaN and no -0.0 -> u, ordered like the doubles; and back
__host__ __device__ inline uint64_t hs_pssm_order_key(uint64_t bits) {
  return bits ^ ((bits >> 63) ? 0xffffffffffffffffull : 0x8000000000000000ull);
}
__host__ __device__ inline uint64_t hs_pssm_order_bits(uint64_t u) {
  return u ^ ((u >> 63) ? 0x8000000000000000ull : 0xffffffffffffffffull);
}
// the descending key and back
__host__ __device__ inline uint64_t hs_pssm_desc_key(uint64_t bits) { return ~hs_pssm_order_key(bits); }
__host__ __device__ inline uint64_t hs_pssm_desc_bits(uint64_t key) { return hs_pssm_order_bits(~key); }

// ---- host: the exported function's body (hs_pssm_topk.hip defines the symbol) -----------------------------------
// The rule for any list of (m, id, score) tuples.  Returns 0; 1 for an argument the contract refuses (nothing is
// written then); 2 when memory ran out.  -0.0 in a tuple is read as +0.0 (no scan produces it).
inline int hs_pssm_topk_hits_host(const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                  uint64_t nm, uint32_t topk, uint32_t topk_max, uint32_t* top_id, double* top_score,
                                  uint32_t* top_count) {
  if (topk < 1 || topk > topk_max) return 1;
  if (n_tuples && (!m || !id || !score)) return 1;
  if (nm && (!top_id || !top_score || !top_count)) return 1;
  try {
    std::vector<uint64_t> live, key(n_tuples);
    for (uint64_t i = 0; i < n_tuples; ++i) {
      if (id[i] == 0xffffffffu) continue;  // padding of a row fed back in
      if (m[i] >= nm || score[i] != score[i]) return 1;
      const double s = score[i] == 0.0 ? 0.0 : score[i];
      uint64_t bits;
      memcpy(&bits, &s, 8);
      key[i] = hs_pssm_desc_key(bits);
      live.push_back(i);
    }
    // (m, descending score, id): a repeated (m, id) with the same bits lands side by side
    std::sort(live.begin(), live.end(), [&](uint64_t x, uint64_t y) {
      if (m[x] != m[y]) return m[x] < m[y];
      if (id[x] != id[y]) return id[x] < id[y];
      return key[x] < key[y];
    });
    size_t kept = 0;
    for (size_t i = 0; i < live.size(); ++i) {
      if (i && m[live[i]] == m[live[i - 1]] && id[live[i]] == id[live[i - 1]]) {
        if (key[live[i]] != key[live[i - 1]]) return 1;  // two scores for one (m, id)
        continue;
      }
      live[kept++] = live[i];
    }
    live.resize(kept);
    std::sort(live.begin(), live.end(), [&](uint64_t x, uint64_t y) {
      if (m[x] != m[y]) return m[x] < m[y];
      if (key[x] != key[y]) return key[x] < key[y];
      return id[x] < id[y];
    });
    // everything is checked: the rows
    const double ninf = -std::numeric_limits<double>::infinity();
    for (uint64_t i = 0; i < nm * topk; ++i) {
      top_id[i] = 0xffffffffu;
      top_score[i] = ninf;
    }
    for (uint64_t i = 0; i < nm; ++i) top_count[i] = 0u;
    for (size_t i = 0; i < live.size(); ++i) {
      const uint64_t j = live[i], row = m[j];
      if (top_count[row] < topk) {
        const uint64_t at = row * topk + top_count[row]++;
        const uint64_t bits = hs_pssm_desc_bits(key[j]);
        top_id[at] = id[j];
        memcpy(&top_score[at], &bits, 8);
      }
    }
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}
