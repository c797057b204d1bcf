// hs_pssm.hip -- hs_pssm_scan: every indexed k-mer scored against position-specific score matrices.
//
// The score of k-mer x under profile m is sum_p S[m][p][x_p]: as a product, one-hot(x) [n][k * alphabet] times
// S [k * alphabet][nm].  A one-hot operand is exact in any number format, so the FILTER runs on
// v_mfma_f32_16x16x128_f8f6f4 with e2m3 operands: the profile side holds the six-bit codes of hs_pssm_tables.h, whose
// sum over a k-mer's entries is at or above the profile's tau whenever the contract's rounded fp64 score reaches t.
// The accumulators are sums of at most 75 multiples of 1/8 within +-7.5: exact in fp32 in any order, so `acc >= tau`
// is an exact compare.  What passes goes to the exact pass (hs_pssm_exact_kernel), which alone decides.
//
// Depth.  Element e = p * alphabet + a of a row, padded with zeros to steps * 128, steps = ceil(k * alphabet / 128).
// The operand of lane (n = lane & 15, q = lane >> 4) in step s is row / column n, elements 128 s + 32 q .. + 31,
// element i at bit 6 i of the lane's 192 bits; result register i of the lane is member row 4 q + i, profile column n
// (the lane map hs_join6_selftest checks).
//
// Profile side (B): tiles of 16 profiles, written by hs_pssm_prep_tiles_kernel in the order the kernel loads them:
// per (tile, step) 1536 bytes = a plane of 64 x 16 bytes (dwords 0..3 of lane l) and a plane of 64 x 8 bytes (dwords
// 4, 5).  Profiles beyond the batch and dead profiles carry zeros and tau = +infinity: nothing reaches it.
//
// Member side (A): the one-hot rows of 16 members, the code of 1.0 at element p * alphabet + x_p, built from
// packed_all.  Members are resident and profiles stream: a wave owns TM = 4 member tiles, a workgroup of 8 waves 512
// members.  For steps <= 4 (k * alphabet <= 512: k = 25 over the amino acids) a wave builds its TM x steps operands
// ONCE (96 VGPRs at 4 steps) and walks all profile tiles of the batch with them; for deeper rows the same loop builds
// the operand of a step when it comes to it.  Profile tiles are fetched from global memory once per WORKGROUP, a
// stage ahead (4 tiles with resident operands, 1 otherwise), into one of two LDS buffers, and every wave reads its B
// operands from there: 1536 bytes per step serve 8 x 4 MFMAs, and one barrier serves a stage.  The compare runs after the LAST step only.  Survivors are collected by ballot, one
// reservation (hs_reserve_survivors) of at most 256 slots per (member tile, profile tile) that has any.
//
// hs_pssm_exact_kernel: per survivor the contract's sum from `codes` and S -- +0.0, then left to right, every sum
// rounded (-ffp-contract=off, and there is no multiply to fuse) --, kept iff >= t, key = m << 32 | id, value = the
// score's bits.  With the filter off (HS_OPT_PSSM_FILTER = 0) it runs over all pairs of the batch instead.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "hs_internal.h"
#include "hs_pssm_tables.h"

namespace {

typedef int intx6 __attribute__((ext_vector_type(6)));
typedef int intx8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int TM = 4;          // member tiles per wave
constexpr int WAVES = 8;       // waves per workgroup
constexpr int BLOCK = 64 * WAVES;
constexpr int STEP_U4 = 96;    // 16-byte words of a (tile, step) of B: 1536 bytes
constexpr int NS_MAX = 4;      // steps with resident A operands
constexpr int PT_RESIDENT = 4; // ... and the profile tiles they stage in LDS per barrier (2 x 24 KB at 4 steps)
constexpr int STEPS_MAX = 19;  // ceil(75 * 32 / 128)

__device__ __forceinline__ floatx4 tile_mfma6(const intx6 a, const intx8 b8, const floatx4 c) {
  const intx8 a8 = __builtin_shufflevector(a, a, 0, 1, 2, 3, 4, 5, -1, -1);
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, 2, 2, 0, 0, 0, 0);
}

inline unsigned blocks_for(uint64_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }

// ------------------------------------------------------------------------------------ validity
// flag |= 1: an entry that is NaN, infinite or beyond 2^100; |= 2: a threshold that is NaN or infinite
__global__ __launch_bounds__(256) void hs_pssm_check_kernel(const double* __restrict__ S, uint64_t n_entries,
                                                            const double* __restrict__ t, uint64_t nm,
                                                            uint32_t* __restrict__ flag) {
  uint32_t bad = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_entries; i += (uint64_t)gridDim.x * 256)
    if (hs_pssm_bad_value(S[i], HS_PSSM_MAX_ABS)) bad |= 1u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nm; i += (uint64_t)gridDim.x * 256)
    if (hs_pssm_bad_value(t[i], 1.7976931348623157e308)) bad |= 2u;
  if (bad) atomicOr(flag, bad);
}

// ------------------------------------------------------------------------------------ tables
// One WAVE per profile slot of the batch (mb profiles, padded to whole tiles): the lanes take the positions -- offset
// and largest |D| of each --, lane 0 sums the offsets in order (hs_pssm_finish: the host's order) and keeps the
// profile's parameters, its tau and its offsets; the dead profiles are counted.
__global__ __launch_bounds__(256) void hs_pssm_prep_kernel(const double* __restrict__ S, const double* __restrict__ t,
                                                           uint32_t mb, uint32_t mb_pad, uint32_t k, uint32_t alphabet,
                                                           hs_pssm_prof* __restrict__ prof, float* __restrict__ tau,
                                                           double* __restrict__ off, uint32_t* __restrict__ n_dead) {
  __shared__ double o_lds[4][HS_PSSM_MAX_K];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, j = blockIdx.x * 4u + wave;
  const bool real = j < mb;
  double dmax = 0.0;
  if (real)
    for (uint32_t p = lane; p < k; p += 64u) {
      double o, d;
      hs_pssm_position(S + ((uint64_t)j * k + p) * alphabet, alphabet, hs_pssm_g(k), &o, &d);
      o_lds[wave][p] = o;
      off[(uint64_t)j * k + p] = o;
      dmax = fmax(dmax, d);
    }
  for (int sh = 32; sh; sh >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, sh));
  __syncthreads();
  if (lane != 0 || j >= mb_pad) return;
  hs_pssm_prof pr;
  pr.s = 1.0;
  pr.g = 0.0;
  pr.tau = INFINITY;
  pr.dead = 0;
  if (real) {
    hs_pssm_finish(o_lds[wave], dmax, t[j], k, &pr);
    if (pr.dead) atomicAdd(n_dead, 1u);
  }
  prof[j] = pr;
  tau[j] = pr.tau;
}

// One thread per (profile slot, step, lane quarter): the 32 codes of its elements as 6 dwords, at the place the
// filter kernel's lane (slot & 15, quarter) loads them from.
__global__ __launch_bounds__(256) void hs_pssm_prep_tiles_kernel(const double* __restrict__ S, uint32_t mb,
                                                                 uint32_t mb_pad, uint32_t k, uint32_t alphabet,
                                                                 uint32_t steps,
                                                                 const hs_pssm_prof* __restrict__ prof,
                                                                 const double* __restrict__ off,
                                                                 uint32_t* __restrict__ btiles) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (uint64_t)mb_pad * steps * 4u) return;
  const uint32_t q = (uint32_t)(i & 3u), j = (uint32_t)((i >> 2) % mb_pad), s = (uint32_t)((i >> 2) / mb_pad);
  uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  if (j < mb) {
    const hs_pssm_prof pr = prof[j];
    if (!pr.dead && pr.tau != -INFINITY) {
      const double* Sm = S + (uint64_t)j * k * alphabet;
      const uint32_t ka = k * alphabet, e0 = HS_PSSM_STEP * s + 32u * q;
#pragma unroll
      for (int el = 0; el < 32; ++el) {
        const uint32_t e = e0 + (uint32_t)el;
        const uint32_t c = e < ka ? hs_pssm_entry_code(Sm[e], off[(uint64_t)j * k + e / alphabet], &pr) : 0u;
        const int bit = 6 * el, wi = bit >> 5, sh = bit & 31;
        w[wi] |= c << sh;
        if (sh > 26) w[wi + 1] |= c >> (32 - sh);
      }
    }
  }
  const uint32_t lane = q * 16u + (j & 15u);
  uint32_t* const ts = btiles + ((uint64_t)(j >> 4) * steps + s) * (STEP_U4 * 4u);
  *reinterpret_cast<uint4*>(ts + lane * 4u) = make_uint4(w[0], w[1], w[2], w[3]);
  *reinterpret_cast<uint2*>(ts + 256u + lane * 2u) = make_uint2(w[4], w[5]);
}

// ------------------------------------------------------------------------------------ the filter
// residue p of member `row` out of packed_all (5-bit residues, 25 per 16-byte word)
__device__ __forceinline__ uint32_t residue_at(const uint32_t* __restrict__ packed32, int PW, uint32_t row, int p) {
  const int w = p / 25, r = p - 25 * w, bit = 5 * r, wi = bit >> 5, sh = bit & 31;
  const uint32_t* const wd = packed32 + ((uint64_t)row * PW + w) * 4u;
  uint32_t c = wd[wi] >> sh;
  if (sh > 27) c |= wd[wi + 1] << (32 - sh);
  return c & 31u;
}

// the one-hot operand of member `row`, step s, lane quarter q: the code of 1.0 (8) at element p * alphabet + x_p
// for the positions whose element falls into [128 s + 32 q, + 32).  A row beyond n is zero.
__device__ __forceinline__ intx6 build_a(const uint32_t* __restrict__ packed32, uint32_t n, int k, int PW, int alphabet,
                                         uint32_t row, int s, int q) {
  uint32_t a[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  if (row < n) {
    const int base = HS_PSSM_STEP * s + 32 * q;
    const int p_lo = base / alphabet;
    int p_hi = (base + 31) / alphabet;
    if (p_hi > k - 1) p_hi = k - 1;
    for (int p = p_lo; p <= p_hi; ++p) {
      const int e = p * alphabet + (int)residue_at(packed32, PW, row, p) - base;
      if (e >= 0 && e < 32) {
        const int bit = 6 * e, wi = bit >> 5, sh = bit & 31;
        const uint64_t v = (uint64_t)8u << sh;
#pragma unroll
        for (int d = 0; d < 6; ++d) {
          if (wi == d) a[d] |= (uint32_t)v;
          if (wi + 1 == d) a[d] |= (uint32_t)(v >> 32);
        }
      }
    }
  }
  return intx6{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5]};
}

// NS > 0: steps == NS and the A operands are resident; NS == 0: any steps, A built per step.
template <int NS>
__global__ __launch_bounds__(BLOCK) void hs_pssm_filter_kernel(const uint4* __restrict__ packed_all, uint32_t n, int k,
                                                               int PW, int alphabet, int steps,
                                                               const uint4* __restrict__ btiles,
                                                               const float* __restrict__ tau, uint32_t n_ptiles,
                                                               uint32_t* __restrict__ prov_count, uint32_t prov_cap,
                                                               uint2* __restrict__ prov) {
  extern __shared__ uint4 lds[];  // two buffers of PT * steps * STEP_U4 words
  constexpr int PT = NS > 0 ? PT_RESIDENT : 1;  // profile tiles per stage: one barrier serves PT tiles
  // words a thread moves per stage
  constexpr int R = (PT * (NS > 0 ? NS : STEPS_MAX) * STEP_U4 + BLOCK - 1) / BLOCK;
  constexpr int NA = NS > 0 ? NS : 1;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
  const uint32_t* const packed32 = reinterpret_cast<const uint32_t*>(packed_all);
  const uint32_t cnt = (uint32_t)steps * STEP_U4, scnt = PT * cnt, total = n_ptiles * cnt;
  const uint32_t row0 = ((uint32_t)blockIdx.x * WAVES + (uint32_t)wave) * (TM * 16u);  // the wave's first member
  const bool active = row0 < n;

  intx6 A[TM][NA];
  if (NS > 0) {
#pragma unroll
    for (int j = 0; j < TM; ++j)
#pragma unroll
      for (int s = 0; s < NA; ++s) A[j][s] = build_a(packed32, n, k, PW, alphabet, row0 + 16u * j + col, s, q);
  }

  uint4 pre[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t idx = (uint32_t)tid + (uint32_t)BLOCK * r;
    if (idx < scnt && idx < total) lds[idx] = btiles[idx];
  }
  __syncthreads();

  const uint32_t n_stages = (n_ptiles + PT - 1) / PT;
  for (uint32_t stage = 0; stage < n_stages; ++stage) {
    const uint32_t sbuf = (stage & 1u) * scnt;
    const bool more = stage + 1 < n_stages;
    if (more) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t idx = (uint32_t)tid + (uint32_t)BLOCK * r, g = (stage + 1) * scnt + idx;
        if (idx < scnt && g < total) pre[r] = btiles[g];
      }
    }
    for (uint32_t u = 0; u < (uint32_t)PT && active; ++u) {
      const uint32_t pt = stage * PT + u, buf = sbuf + u * cnt;
      if (pt >= n_ptiles) break;
      const float tv = tau[pt * 16u + (uint32_t)col];
      floatx4 acc[TM];
#pragma unroll
      for (int j = 0; j < TM; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (NS > 0) {
#pragma unroll
        for (int s = 0; s < NA; ++s) {
          const uint4 b0 = lds[buf + s * STEP_U4 + lane];
          const uint2 b1 = reinterpret_cast<const uint2*>(lds + buf + s * STEP_U4 + 64)[lane];
          const intx8 b8 = intx8{(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, 0, 0};
#pragma unroll
          for (int j = 0; j < TM; ++j) acc[j] = tile_mfma6(A[j][s], b8, acc[j]);
        }
      } else {
        for (int s = 0; s < steps; ++s) {
          const uint4 b0 = lds[buf + s * STEP_U4 + lane];
          const uint2 b1 = reinterpret_cast<const uint2*>(lds + buf + s * STEP_U4 + 64)[lane];
          const intx8 b8 = intx8{(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, 0, 0};
#pragma unroll
          for (int j = 0; j < TM; ++j)
            acc[j] = tile_mfma6(build_a(packed32, n, k, PW, alphabet, row0 + 16u * j + col, s, q), b8, acc[j]);
        }
      }
      // register i of lane (col, q) of tile j: member row0 + 16 j + 4 q + i against profile 16 pt + col
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const uint32_t r0 = row0 + 16u * j + 4u * q;
        bool pass[4];
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          pass[i] = acc[j][i] >= tv && r0 + (uint32_t)i < n;
          any |= pass[i];
        }
        if (__ballot(any)) {  // (wave-uniform)
          uint64_t bal[4];
          uint32_t total = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            bal[i] = __ballot(pass[i]);
            total += (uint32_t)__popcll(bal[i]);
          }
          uint32_t base = 0;
          if (lane == 0) base = hs_reserve_survivors(prov_count, total);
          base = (uint32_t)__shfl((int)base, 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (pass[i]) {
              const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[i] >> 32),
                                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)bal[i], 0u));
              if (at < prov_cap) prov[at] = make_uint2(pt * 16u + (uint32_t)col, r0 + (uint32_t)i);
            }
            base += (uint32_t)__popcll(bal[i]);
          }
        }
      }
    }
    if (more) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t idx = (uint32_t)tid + (uint32_t)BLOCK * r;
        if (idx < scnt && (stage + 1) * scnt + idx < total) lds[(sbuf ? 0u : scnt) + idx] = pre[r];
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ the exact pass
// S, t: the BATCH's profiles (profile 0 = number m_base of the call).  all_pairs == 0: the survivor list; else every
// (profile, id) pair of the batch, and every hit is counted into the survivor counter as well (the host sizes the
// hit lists from it, as it sizes the survivor list).
__global__ __launch_bounds__(256) void hs_pssm_exact_kernel(const uint8_t* __restrict__ codes,
                                                            const double* __restrict__ S, const double* __restrict__ t,
                                                            int k, int alphabet, uint32_t m_base, uint32_t mb,
                                                            uint32_t n, const uint2* __restrict__ prov,
                                                            uint32_t* __restrict__ counters, uint32_t prov_cap,
                                                            int all_pairs, uint32_t hit_cap,
                                                            uint64_t* __restrict__ hit_key,
                                                            uint64_t* __restrict__ hit_val) {
  const uint64_t total = all_pairs ? (uint64_t)mb * n : (uint64_t)min(counters[0], prov_cap);
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
    uint32_t ml, id;
    if (all_pairs) {
      ml = (uint32_t)(e / n);
      id = (uint32_t)(e - (uint64_t)ml * n);
    } else {
      ml = prov[e].x;
      id = prov[e].y;
    }
    const double* const Sm = S + (uint64_t)ml * k * alphabet;
    const uint8_t* const x = codes + (uint64_t)id * k;
    double sc = 0.0;
    for (int p = 0; p < k; ++p) sc = sc + Sm[p * alphabet + x[p]];
    if (sc >= t[ml]) {
      if (all_pairs) (void)hs_reserve_survivors(counters, 1u);
      const uint32_t idx = atomicAdd(counters + 1, 1u);
      if (idx < hit_cap) {
        hit_key[idx] = ((uint64_t)(m_base + ml) << 32) | id;
        hit_val[idx] = (uint64_t)__double_as_longlong(sc);
      }
    }
  }
}

// a batch's hits into the caller's arrays (write != 0) and into the per-profile counts (cnt may be null)
__global__ __launch_bounds__(256) void hs_pssm_emit_kernel(const uint64_t* __restrict__ key,
                                                           const uint64_t* __restrict__ val, uint32_t nh, int write,
                                                           uint32_t* __restrict__ out_m, uint32_t* __restrict__ out_id,
                                                           double* __restrict__ out_score,
                                                           unsigned long long* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nh) return;
  const uint64_t kk = key[i];
  if (cnt) atomicAdd(cnt + (kk >> 32), 1ull);
  if (write) {
    out_m[i] = (uint32_t)(kk >> 32);
    out_id[i] = (uint32_t)kk;
    out_score[i] = __longlong_as_double((long long)val[i]);
  }
}

}  // namespace

size_t hs_pssm_prof_bytes(uint32_t k) { return sizeof(hs_pssm_prof) + (size_t)k * 8; }
size_t hs_pssm_tile_bytes(uint32_t steps) { return (size_t)steps * STEP_U4 * 16; }

hipError_t hs_launch_pssm_check(const double* d_S, uint64_t n_entries, const double* d_t, uint64_t nm, uint32_t* d_flag,
                                hipStream_t s) {
  if (!n_entries && !nm) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<uint64_t>(4096, (std::max(n_entries, nm) + 255) / 256);
  hs_pssm_check_kernel<<<blocks, 256, 0, s>>>(d_S, n_entries, d_t, nm, d_flag);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_prep(const double* d_S, const double* d_t, uint32_t mb, uint32_t k, uint32_t alphabet,
                               void* d_prof, float* d_tau, void* d_btiles, uint32_t* d_n_dead, hipStream_t s) {
  if (!mb) return hipSuccess;
  const uint32_t mb_pad = (mb + 15u) & ~15u, steps = hs_pssm_steps(k, alphabet);
  // d_prof: the slots' parameters, and behind them their offsets [mb_pad][k]
  double* const d_off = reinterpret_cast<double*>(static_cast<char*>(d_prof) + (size_t)mb_pad * sizeof(hs_pssm_prof));
  hs_pssm_prep_kernel<<<mb_pad / 4, 256, 0, s>>>(d_S, d_t, mb, mb_pad, k, alphabet, (hs_pssm_prof*)d_prof, d_tau, d_off,
                                                 d_n_dead);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hs_pssm_prep_tiles_kernel<<<blocks_for((uint64_t)mb_pad * steps * 4u), 256, 0, s>>>(
      d_S, mb, mb_pad, k, alphabet, steps, (const hs_pssm_prof*)d_prof, d_off, (uint32_t*)d_btiles);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_filter(const uint4* d_packed_all, uint32_t n, int k, int alphabet, const void* d_btiles,
                                 const float* d_tau, uint32_t mb, uint32_t* d_prov_count, uint32_t prov_cap,
                                 uint2* d_prov, hipStream_t s) {
  if (!n || !mb) return hipSuccess;
  const int steps = (int)hs_pssm_steps((uint32_t)k, (uint32_t)alphabet), PW = hs_packed_words(k);
  const uint32_t n_ptiles = (mb + 15u) / 16u;
  const unsigned blocks = blocks_for(n, WAVES * TM * 16);
  const size_t shmem = 2 * (steps <= NS_MAX ? PT_RESIDENT : 1) * hs_pssm_tile_bytes((uint32_t)steps);
  const uint4* const bt = (const uint4*)d_btiles;
#define HS_PSSM_LAUNCH(NS)                                                                                          \
  hs_pssm_filter_kernel<NS><<<blocks, BLOCK, shmem, s>>>(d_packed_all, n, k, PW, alphabet, steps, bt, d_tau, n_ptiles, \
                                                         d_prov_count, prov_cap, d_prov)
  switch (steps <= NS_MAX ? steps : 0) {
    case 1: HS_PSSM_LAUNCH(1); break;
    case 2: HS_PSSM_LAUNCH(2); break;
    case 3: HS_PSSM_LAUNCH(3); break;
    case 4: HS_PSSM_LAUNCH(4); break;
    default: HS_PSSM_LAUNCH(0); break;
  }
#undef HS_PSSM_LAUNCH
  return hipGetLastError();
}

hipError_t hs_launch_pssm_exact(const uint8_t* d_codes, const double* d_S, const double* d_t, int k, int alphabet,
                                uint32_t m_base, uint32_t mb, uint32_t n, const uint2* d_prov, uint32_t* d_counters,
                                uint32_t prov_cap, bool all_pairs, uint32_t hit_cap, uint64_t* d_hit_key,
                                uint64_t* d_hit_val, int n_cu, hipStream_t s) {
  if (!n || !mb) return hipSuccess;
  hs_pssm_exact_kernel<<<n_cu * 8, 256, 0, s>>>(d_codes, d_S, d_t, k, alphabet, m_base, mb, n, d_prov, d_counters,
                                                prov_cap, all_pairs ? 1 : 0, hit_cap, d_hit_key, d_hit_val);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_emit(const uint64_t* d_key, const uint64_t* d_val, uint32_t nh, bool write, uint32_t* d_out_m,
                               uint32_t* d_out_id, double* d_out_score, uint64_t* d_cnt, hipStream_t s) {
  if (!nh || (!write && !d_cnt)) return hipSuccess;
  hs_pssm_emit_kernel<<<blocks_for(nh), 256, 0, s>>>(d_key, d_val, nh, write ? 1 : 0, d_out_m, d_out_id, d_out_score,
                                                     (unsigned long long*)d_cnt);
  return hipGetLastError();
}
