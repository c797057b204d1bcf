// hs_multiprobe.hip -- query-directed multi-probe LSH (Lv et al., VLDB 2007): the T extra buckets per table
// a query looks in besides its own (hs_set_multiprobe, include/hsearch.h).
//
// 1. hs_mp_hash_kernel: the query's projections in the reference's fp64 order (lsh.hpp:33-49), as
//    hs_hash_kernel evaluates them, keeping v = (dot + b) / W: the bucket int floor(v) AND the fraction
//    x = v - floor(v).  The fractions decide which neighbouring buckets are probed, so they come from this
//    exact pass and never from the int8 projection (whose values carry an error bound).
// 2. hs_mp_probe_sets_kernel: one thread per (query, table).  The 2K boundary distances z(j,-1) = x_j,
//    z(j,+1) = 1 - x_j are ranked by (z, j, delta); perturbation sets are drawn from a min-heap on
//    (score, mask) -- score = sum of z_i^2 over the set in ascending i -- starting at {0}, each pop pushing
//    shift (max element m -> m + 1) and expand (m + 1 added).  Pops that hold both deltas of one function
//    are skipped; generation ends after T sets or 4 (T + 1) pops.  Slots left over are empty probes: their
//    ints repeat the home bucket and their valid flag is 0.
// Both scores and the heap live in private arrays (the heap holds at most 4 T + 5 entries): the kernel
// runs once per query call over nq x L threads, against the probe chain's nq x L x (T + 1) lookups.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "hs_internal.h"

namespace {

// KC functions per thread, strictly i = 0..d-1 per function, product rounded then sum rounded
template <int KC>
__global__ __launch_bounds__(256) void hs_mp_hash_kernel(const double* __restrict__ pts, uint64_t n, int d,
                                                         const double* __restrict__ aT, int F,
                                                         const double* __restrict__ b, double W,
                                                         int32_t* __restrict__ ints, double* __restrict__ frac) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < n;
  const double* x = pts + (valid ? i : 0) * (uint64_t)d;
  for (int fc = (int)blockIdx.y * KC; fc < F; fc += KC * (int)gridDim.y) {
    int fi[KC];
#pragma unroll
    for (int f = 0; f < KC; ++f) fi[f] = min(fc + f, F - 1);  // past the end: a harmless re-read
    double acc[KC];
#pragma unroll
    for (int f = 0; f < KC; ++f) acc[f] = 0.0;
    for (int e = 0; e < d; ++e) {
      const double xe = x[e];
      const double* ar = aT + (size_t)e * F;
#pragma unroll
      for (int f = 0; f < KC; ++f) acc[f] = __dadd_rn(acc[f], __dmul_rn(xe, ar[fi[f]]));
    }
    if (valid) {
#pragma unroll
      for (int f = 0; f < KC; ++f) {
        if (fc + f >= F) break;
        const double v = __ddiv_rn(__dadd_rn(acc[f], b[fc + f]), W);
        const double hb = floor(v);
        ints[i * (uint64_t)F + fc + f] = (int32_t)hb;
        frac[i * (uint64_t)F + fc + f] = __dsub_rn(v, hb);
      }
    }
  }
}

__device__ __forceinline__ bool mp_less(double sa, uint64_t ma, double sb, uint64_t mb) {
  return sa < sb || (sa == sb && ma < mb);
}

// HCAP >= 4 T + 5: the heap never holds more (every pop removes one entry and adds at most two)
template <int HCAP>
__global__ __launch_bounds__(256) void hs_mp_probe_sets_kernel(const int32_t* __restrict__ ints,
                                                               const double* __restrict__ frac, uint64_t n, int K,
                                                               int L, int T, int32_t* __restrict__ out,
                                                               uint8_t* __restrict__ valid_out, uint64_t sq,
                                                               uint32_t sl, uint32_t st) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n * (uint64_t)L) return;
  const uint64_t q = g / (uint32_t)L;
  const uint32_t l = (uint32_t)(g % (uint32_t)L);
  const int32_t* hb = ints + g * K;
  const double* x = frac + g * K;
  const int M = 2 * K;
  // the boundary distances in (z, j, delta) order: element e = 2 j + (delta == +1)
  double zs[2 * HS_MAX_K];
  uint8_t cd[2 * HS_MAX_K];
  for (int e = 0; e < M; ++e) {
    const double ze = (e & 1) ? __dsub_rn(1.0, x[e >> 1]) : x[e >> 1];
    int r = 0;
    for (int f = 0; f < M; ++f) {
      const double zf = (f & 1) ? __dsub_rn(1.0, x[f >> 1]) : x[f >> 1];
      r += (zf < ze || (zf == ze && f < e)) ? 1 : 0;
    }
    zs[r] = ze;
    cd[r] = (uint8_t)e;
  }
  auto score = [&](uint64_t m) {
    double s = 0.0;
    for (uint64_t r = m; r; r &= r - 1) {
      const int i = __builtin_ctzll(r);
      s = __dadd_rn(s, __dmul_rn(zs[i], zs[i]));
    }
    return s;
  };
  auto slot = [&](int t) { return q * sq + (uint64_t)l * sl + (uint64_t)t * st; };
  {
    const uint64_t o = slot(0);
    for (int j = 0; j < K; ++j) out[o * K + j] = hb[j];
    valid_out[o] = 1;
  }
  double hs[HCAP];
  uint64_t hm[HCAP];
  int size = 0;
  auto push = [&](double s, uint64_t m) {
    int c = size++;
    while (c > 0) {
      const int p = (c - 1) >> 1;
      if (!mp_less(s, m, hs[p], hm[p])) break;
      hs[c] = hs[p];
      hm[c] = hm[p];
      c = p;
    }
    hs[c] = s;
    hm[c] = m;
  };
  int emitted = 0, pops = 0;
  if (T > 0) push(score(1ull), 1ull);
  while (emitted < T && pops < 4 * (T + 1) && size > 0) {
    const uint64_t m = hm[0];
    // pop: the last entry sifts down from the root
    const double ls = hs[size - 1];
    const uint64_t lm = hm[size - 1];
    --size;
    int c = 0;
    for (;;) {
      const int a = 2 * c + 1;
      if (a >= size) break;
      const int s2 = (a + 1 < size && mp_less(hs[a + 1], hm[a + 1], hs[a], hm[a])) ? a + 1 : a;
      if (!mp_less(hs[s2], hm[s2], ls, lm)) break;
      hs[c] = hs[s2];
      hm[c] = hm[s2];
      c = s2;
    }
    if (size > 0) {
      hs[c] = ls;
      hm[c] = lm;
    }
    ++pops;
    const int top = 63 - __builtin_clzll(m);
    if (top + 1 < M) {
      const uint64_t shifted = (m & ~(1ull << top)) | (1ull << (top + 1));
      const uint64_t expanded = m | (1ull << (top + 1));
      push(score(shifted), shifted);
      push(score(expanded), expanded);
    }
    uint64_t seen = 0;
    bool ok = true;
    for (uint64_t r = m; r; r &= r - 1) {
      const int j = cd[__builtin_ctzll(r)] >> 1;
      ok = ok && !((seen >> j) & 1ull);
      seen |= 1ull << j;
    }
    if (!ok) continue;
    ++emitted;
    const uint64_t o = slot(emitted);
    for (int j = 0; j < K; ++j) out[o * K + j] = hb[j];
    for (uint64_t r = m; r; r &= r - 1) {
      const int e = cd[__builtin_ctzll(r)];
      out[o * K + (e >> 1)] = hb[e >> 1] + ((e & 1) ? 1 : -1);
    }
    valid_out[o] = 1;
  }
  for (int t = emitted + 1; t <= T; ++t) {
    const uint64_t o = slot(t);
    for (int j = 0; j < K; ++j) out[o * K + j] = hb[j];
    valid_out[o] = 0;
  }
}

// out[r][c] = in[r / P][c]: every query's row once per probe
template <typename E>
__global__ __launch_bounds__(256) void hs_mp_repeat_rows_kernel(const E* __restrict__ in, uint64_t n_out_rows,
                                                                uint32_t row, uint32_t P, E* __restrict__ out) {
  const uint64_t total = n_out_rows * row;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t r = i / row, c = i - r * row;
    out[i] = in[(r / P) * row + c];
  }
}

// a hit of probe row r belongs to query q_base + r / P
__global__ __launch_bounds__(256) void hs_mp_map_q_kernel(uint32_t* __restrict__ q, uint64_t n, uint32_t P,
                                                          uint32_t q_base) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) q[i] = q_base + q[i] / P;
}

// cand[q][l] = sum over t of vcand[q P + t][l]
__global__ __launch_bounds__(256) void hs_mp_cand_kernel(const uint64_t* __restrict__ vcand, uint64_t nq, uint32_t L,
                                                         uint32_t P, uint64_t* __restrict__ cand) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * L) return;
  const uint64_t q = i / L, l = i - q * L;
  uint64_t s = 0;
  for (uint32_t t = 0; t < P; ++t) s += vcand[(q * P + t) * L + l];
  cand[i] = s;
}

inline unsigned mp_blocks(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t hs_launch_mp_hash(const double* d_pts, uint64_t n, int k, const double* d_aT, int F, const double* d_b,
                             double W, int32_t* d_ints, double* d_frac, hipStream_t s) {
  if (!n) return hipSuccess;
  constexpr int KC = 4;
  const unsigned bx = mp_blocks(n);
  // few points (a query batch): the function chunks spread over blockIdx.y so the launch fills the chip
  const unsigned chunks = (unsigned)((F + KC - 1) / KC);
  const unsigned by = std::max(1u, std::min(chunks, (2048u + bx - 1) / bx));
  hs_mp_hash_kernel<KC><<<dim3(bx, by), 256, 0, s>>>(d_pts, n, 8 * k, d_aT, F, d_b, W, d_ints, d_frac);
  return hipGetLastError();
}

hipError_t hs_launch_mp_probe_sets(const int32_t* d_ints, const double* d_frac, uint64_t n, int K, int L, int T,
                                   int32_t* d_out, uint8_t* d_valid, uint64_t sq, uint32_t sl, uint32_t st,
                                   hipStream_t s) {
  if (!n) return hipSuccess;
  if (T < 0 || T > 63 || K < 1 || K > HS_MAX_K) return hipErrorInvalidValue;
  const unsigned blocks = mp_blocks(n * (uint64_t)L);
#define HS_MP_SETS(CAP) \
  hs_mp_probe_sets_kernel<CAP><<<blocks, 256, 0, s>>>(d_ints, d_frac, n, K, L, T, d_out, d_valid, sq, sl, st)
  if (T <= 1) HS_MP_SETS(9);
  else if (T <= 8) HS_MP_SETS(37);
  else if (T <= 16) HS_MP_SETS(69);
  else if (T <= 32) HS_MP_SETS(133);
  else HS_MP_SETS(257);
#undef HS_MP_SETS
  return hipGetLastError();
}

hipError_t hs_launch_mp_repeat_f64(const double* d_in, uint64_t n_out_rows, uint32_t row, uint32_t P, double* d_out,
                                   hipStream_t s) {
  const uint64_t total = n_out_rows * row;
  if (!total) return hipSuccess;
  hs_mp_repeat_rows_kernel<double><<<(unsigned)std::min<uint64_t>(mp_blocks(total), 4096), 256, 0, s>>>(
      d_in, n_out_rows, row, P, d_out);
  return hipGetLastError();
}

hipError_t hs_launch_mp_repeat_u8(const uint8_t* d_in, uint64_t n_out_rows, uint32_t row, uint32_t P, uint8_t* d_out,
                                  hipStream_t s) {
  const uint64_t total = n_out_rows * row;
  if (!total) return hipSuccess;
  hs_mp_repeat_rows_kernel<uint8_t><<<(unsigned)std::min<uint64_t>(mp_blocks(total), 4096), 256, 0, s>>>(
      d_in, n_out_rows, row, P, d_out);
  return hipGetLastError();
}

hipError_t hs_launch_mp_map_q(uint32_t* d_q, uint64_t n, uint32_t P, uint32_t q_base, hipStream_t s) {
  if (!n) return hipSuccess;
  hs_mp_map_q_kernel<<<mp_blocks(n), 256, 0, s>>>(d_q, n, P, q_base);
  return hipGetLastError();
}

hipError_t hs_launch_mp_cand(const uint64_t* d_vcand, uint64_t nq, uint32_t L, uint32_t P, uint64_t* d_cand,
                             hipStream_t s) {
  if (!nq) return hipSuccess;
  hs_mp_cand_kernel<<<mp_blocks(nq * L), 256, 0, s>>>(d_vcand, nq, L, P, d_cand);
  return hipGetLastError();
}
