// hs_pssm_null.hip -- hs_pssm_pvalue / hs_pssm_pvalue_threshold (include/hsearch.h): the null-model score
// distribution of every profile, convolved on the device, and the lookups into it.  The rule, its constants and the
// proof of the bracket p_lo <= P <= p_hi: hs_pssm_null.h; every table below is built through that header's routines,
// so the device's bits are the host's (hs_pssm_null_tables).
//
// A batch of mb profiles (hs_capi_pssm.hip pssm_null_core), `sides` = 1 (the upper side alone) or 2:
//   1. hs_pssm_null_prep_kernel   one workgroup per profile: thread 0 computes the profile's parameters (offset sums,
//        their error bounds, delta, the dead flag), then thread p the saturated bin shifts q_dn / q_up of position p.
//   2. hs_pssm_null_conv_kernel   one workgroup of 1024 threads per (profile, side).  Both pdf buffers live in dynamic
//        LDS (2 * B * 8 bytes: 64 KB at B = 4096, 128 KB at 8192, of a CU's 160 KB), so one workgroup is resident per CU
//        and its 16 waves are four per SIMD: one wave per SIMD does not reach the LDS read rate with 8-byte reads, about
//        four do.  Lane j reads old[j - q] for a workgroup-uniform q: consecutive lanes read consecutive doubles, which
//        8-byte LDS reads serve without a bank conflict.  bg is staged once, the q row of position p + 1 while position p
//        runs (two rows, alternating), so a position costs one barrier.  A thread carries its ceil(B / 1024) bins side by
//        side, so one broadcast read of q[a] and bg[a] serves them all.  The sums run over a ascending with __dmul_rn /
//        __dadd_rn, a shift that leaves the buffer adds +0.0 (exact: the accumulator is never negative), mass beyond bin
//        B - 1 is never written.  Then the blocked cumulative sum of the rule: one lane per block of 64 bins, the block
//        bases by one lane, cdf[j] = base[j >> 6] + run[j] stored to global memory.
//        Not done: skipping the bins that cannot hold mass yet (it would change no bit; it was not measured).
//   3. hs_pssm_null_lookup_kernel     one lane per hit of the call whose profile is in the batch: J_hi, J_lo, the two
//        table reads, the margins.
//      hs_pssm_null_threshold_kernel  one lane per profile: the binary search of the ladder for J*, the bisection over
//        the ordered keys of the doubles for t_p, and the lookup at t_p.
// The dynamic-LDS attribute is granted at every launch of step 2: the grant belongs to the current device's copy of the
// kernel, so a flag kept per process would leave every device but the first without it.
// All stores are vector stores.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "hs_internal.h"
#include "hs_pssm_null.h"

namespace {

constexpr int NULL_CONV_THREADS = 1024;

// flag |= 16: bg outside the rule; 32: a p outside (0, 1]; 64: a hit's profile >= nm; 128: a NaN hit score
__global__ __launch_bounds__(256) void hs_pssm_null_check_kernel(const double* __restrict__ bg, uint32_t alphabet,
                                                                 const double* __restrict__ p, uint64_t nm,
                                                                 const uint32_t* __restrict__ hit_m,
                                                                 const double* __restrict__ hit_score, uint64_t n,
                                                                 uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint32_t bad = 0;
  if (i == 0 && bg && !hs_pssm_null_bg_ok(bg, alphabet)) bad |= 16u;
  if (p && i < nm && !hs_pssm_null_p_ok(p[i])) bad |= 32u;
  if (hit_m && i < n) {
    if (hit_m[i] >= nm) bad |= 64u;
    const double s = hit_score[i];
    if (s != s) bad |= 128u;
  }
  if (bad) atomicOr(flag, bad);
}

// 1. parameters and bin shifts; S, t_lo (may be null: 0): the batch's
__global__ __launch_bounds__(128) void hs_pssm_null_prep_kernel(const double* __restrict__ S,
                                                                const double* __restrict__ t_lo, uint32_t k,
                                                                uint32_t alphabet, uint32_t B, int sides,
                                                                hs_pssm_null_prof* __restrict__ prof,
                                                                uint16_t* __restrict__ q_dn,
                                                                uint16_t* __restrict__ q_up) {
  __shared__ double s_delta;
  const uint32_t m = blockIdx.x;
  const size_t ka = (size_t)k * alphabet;
  const double* const Sm = S + m * ka;
  if (threadIdx.x == 0) {
    hs_pssm_null_prof pr;
    hs_pssm_null_profile(Sm, k, alphabet, t_lo ? t_lo[m] : 0.0, B, &pr);
    prof[m] = pr;
    s_delta = pr.delta;
  }
  __syncthreads();
  const uint32_t p = threadIdx.x;
  if (p >= k) return;
  const double g = hs_pssm_g(k), delta = s_delta;
  const double* const row = Sm + (size_t)p * alphabet;
  for (int side = 0; side < sides; ++side) {
    const double o = hs_pssm_null_offset(row, alphabet, g, side);
    uint16_t* const out = (side ? q_up : q_dn) + m * ka + (size_t)p * alphabet;
    for (uint32_t a = 0; a < alphabet; ++a) out[a] = (uint16_t)hs_pssm_null_q(row[a], o, g, delta, B, side);
  }
}

// 2. the convolution and the cumulative sum of one (profile, side); cdf [sides][mb][B]
// NULL_CONV_BINS: the bins a thread carries side by side, ceil(B / 1024) rounded up to 1, 2, 4 or 8
template <int NULL_CONV_BINS>
__global__ __launch_bounds__(NULL_CONV_THREADS) void hs_pssm_null_conv_kernel(const uint16_t* __restrict__ q_dn,
                                                                              const uint16_t* __restrict__ q_up,
                                                                              const double* __restrict__ bg, uint32_t k,
                                                                              uint32_t alphabet, uint32_t B,
                                                                              uint32_t mb, int sides,
                                                                              double* __restrict__ cdf) {
  extern __shared__ double pdf[];  // [2][B]
  __shared__ uint16_t qs[2][32];
  __shared__ double bgs[32];
  __shared__ double base_s[HS_PSSM_NULL_MAX_BINS / 64 + 1];
  const uint32_t m = blockIdx.x / (uint32_t)sides, side = blockIdx.x - m * (uint32_t)sides;
  if (m >= mb) return;  // (the whole workgroup)
  const uint32_t tid = threadIdx.x;
  const uint16_t* const q = (side ? q_up : q_dn) + (size_t)m * k * alphabet;
  for (uint32_t j = tid; j < 2 * B; j += NULL_CONV_THREADS) pdf[j] = j == 0 ? 1.0 : 0.0;
  if (tid < alphabet) {
    bgs[tid] = bg[tid];
    qs[0][tid] = q[tid];
  }
  __syncthreads();
  uint32_t cur = 0;
  for (uint32_t p = 0; p < k; ++p) {
    if (tid < alphabet && p + 1 < k) qs[(p + 1) & 1][tid] = q[(size_t)(p + 1) * alphabet + tid];
    const double* const old = pdf + (size_t)cur * B;
    double* const nxt = pdf + (size_t)(cur ^ 1u) * B;
    const uint16_t* const qr = qs[p & 1];
    // a thread's bins tid, tid + 1024, ... (at most NULL_CONV_BINS) side by side: one read of q and bg serves them all,
    // and every bin still sums over a ascending
    double acc[NULL_CONV_BINS];
#pragma unroll
    for (int i = 0; i < NULL_CONV_BINS; ++i) acc[i] = 0.0;
    for (uint32_t a = 0; a < alphabet; ++a) {
      const uint32_t qa = qr[a];
      const double w = bgs[a];
#pragma unroll
      for (int i = 0; i < NULL_CONV_BINS; ++i) {
        const uint32_t j = tid + (uint32_t)i * NULL_CONV_THREADS;
        const double v = (j < B && qa <= j) ? old[j - qa] : 0.0;  // (the index stays inside 0 .. j)
        acc[i] = __dadd_rn(acc[i], __dmul_rn(w, v));
      }
    }
#pragma unroll
    for (int i = 0; i < NULL_CONV_BINS; ++i) {
      const uint32_t j = tid + (uint32_t)i * NULL_CONV_THREADS;
      if (j < B) nxt[j] = acc[i];
    }
    __syncthreads();
    cur ^= 1u;
  }
  const double* const fin = pdf + (size_t)cur * B;
  double* const run = pdf + (size_t)(cur ^ 1u) * B;
  const uint32_t nblk = (B + 63u) / 64u;
  if (tid < nblk) {
    const uint32_t b0 = tid * 64u, b1 = b0 + 64u < B ? b0 + 64u : B;
    double r = fin[b0];
    run[b0] = r;
    for (uint32_t j = b0 + 1; j < b1; ++j) {
      r = __dadd_rn(r, fin[j]);
      run[j] = r;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double base = 0.0;
    for (uint32_t b = 0; b < nblk; ++b) {
      base_s[b] = base;
      const uint32_t last = b * 64u + 63u;
      if (last < B) base = __dadd_rn(base, run[last]);
    }
  }
  __syncthreads();
  double* const out = cdf + ((size_t)side * mb + m) * B;
  for (uint32_t j = tid; j < B; j += NULL_CONV_THREADS) out[j] = __dadd_rn(base_s[j >> 6], run[j]);
}

// 3. the lookups: hits of the CALL, profiles m0 .. m0 + mb - 1 in the tables
__global__ __launch_bounds__(256) void hs_pssm_null_lookup_kernel(const hs_pssm_null_prof* __restrict__ prof,
                                                                  const double* __restrict__ cdf, uint32_t m0,
                                                                  uint32_t mb, uint32_t B, double e, int sides,
                                                                  const uint32_t* __restrict__ hit_m,
                                                                  const double* __restrict__ hit_score, uint64_t n,
                                                                  double* __restrict__ p_hi, double* __restrict__ p_lo) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = hit_m[i] - m0;  // (unsigned: below the batch wraps above it)
  if (m >= mb) return;
  const hs_pssm_null_prof pr = prof[m];
  double hi = 0.0, lo = 0.0;
  const bool both = sides == 2 && p_lo;
  hs_pssm_null_lookup(&pr, B, e, cdf + (size_t)m * B, both ? cdf + ((size_t)mb + m) * B : nullptr, hit_score[i], &hi,
                      both ? &lo : nullptr);
  p_hi[i] = hi;
  if (both) p_lo[i] = lo;
}

// t_lo, p: the batch's; the outputs: the batch's
__global__ __launch_bounds__(64) void hs_pssm_null_threshold_kernel(const hs_pssm_null_prof* __restrict__ prof,
                                                                    const double* __restrict__ cdf, uint32_t mb,
                                                                    uint32_t B, double e, int sides,
                                                                    const double* __restrict__ t_lo,
                                                                    const double* __restrict__ p,
                                                                    double* __restrict__ t_p, double* __restrict__ p_hi,
                                                                    double* __restrict__ p_lo,
                                                                    uint32_t* __restrict__ flag) {
  const uint32_t m = blockIdx.x * 64u + threadIdx.x;
  if (m >= mb) return;
  const hs_pssm_null_prof pr = prof[m];
  const double* const cd = cdf + (size_t)m * B;
  double t = 0.0, hi = 0.0, lo = 0.0;
  uint32_t f = 0;
  hs_pssm_null_threshold(&pr, B, e, cd, t_lo ? t_lo[m] : 0.0, p[m], &t, &f);
  const bool both = sides == 2 && p_lo;
  hs_pssm_null_lookup(&pr, B, e, cd, both ? cdf + ((size_t)mb + m) * B : nullptr, t, &hi, both ? &lo : nullptr);
  t_p[m] = t;
  p_hi[m] = hi;
  if (both) p_lo[m] = lo;
  flag[m] = f;
}

}  // namespace

size_t hs_pssm_null_prof_bytes(uint32_t mb) { return (size_t)mb * sizeof(hs_pssm_null_prof); }

hipError_t hs_launch_pssm_null_check(const double* d_bg, uint32_t alphabet, const double* d_p, uint64_t nm,
                                     const uint32_t* d_hit_m, const double* d_hit_score, uint64_t n, uint32_t* d_flag,
                                     hipStream_t s) {
  const uint64_t items = std::max<uint64_t>(1, std::max<uint64_t>(d_p ? nm : 0, d_hit_m ? n : 0));
  hs_pssm_null_check_kernel<<<(unsigned)((items + 255u) / 256u), 256, 0, s>>>(d_bg, alphabet, d_p, nm, d_hit_m,
                                                                             d_hit_score, n, d_flag);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_null_tables(const double* d_S, const double* d_bg, const double* d_t_lo, uint32_t mb,
                                      uint32_t k, uint32_t alphabet, uint32_t B, int sides, void* d_prof,
                                      uint16_t* d_q_dn, uint16_t* d_q_up, double* d_cdf, hipStream_t s) {
  if (!mb) return hipSuccess;
  if (k > 128 || alphabet > 32 || B < HS_PSSM_NULL_MIN_BINS || B > HS_PSSM_NULL_MAX_BINS || sides < 1 || sides > 2)
    return hipErrorInvalidValue;
  hs_pssm_null_prep_kernel<<<mb, 128, 0, s>>>(d_S, d_t_lo, k, alphabet, B, sides,
                                             reinterpret_cast<hs_pssm_null_prof*>(d_prof), d_q_dn, d_q_up);
  const size_t shmem = 2 * (size_t)B * 8;
  auto conv = hs_pssm_null_conv_kernel<8>;
  if (B <= 1024) conv = hs_pssm_null_conv_kernel<1>;
  else if (B <= 2048) conv = hs_pssm_null_conv_kernel<2>;
  else if (B <= 4096) conv = hs_pssm_null_conv_kernel<4>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)shmem);
  if (e != hipSuccess) return e;
  conv<<<mb * (uint32_t)sides, NULL_CONV_THREADS, shmem, s>>>(d_q_dn, d_q_up, d_bg, k, alphabet, B, mb, sides, d_cdf);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_null_lookup(const void* d_prof, const double* d_cdf, uint32_t m0, uint32_t mb, uint32_t k,
                                      uint32_t alphabet, uint32_t B, int sides, const uint32_t* d_hit_m,
                                      const double* d_hit_score, uint64_t n, double* d_p_hi, double* d_p_lo,
                                      hipStream_t s) {
  if (!n || !mb) return hipSuccess;
  hs_pssm_null_lookup_kernel<<<(unsigned)((n + 255u) / 256u), 256, 0, s>>>(
      reinterpret_cast<const hs_pssm_null_prof*>(d_prof), d_cdf, m0, mb, B, hs_pssm_null_e(k, alphabet), sides, d_hit_m,
      d_hit_score, n, d_p_hi, d_p_lo);
  return hipGetLastError();
}

hipError_t hs_launch_pssm_null_threshold(const void* d_prof, const double* d_cdf, uint32_t mb, uint32_t k,
                                         uint32_t alphabet, uint32_t B, int sides, const double* d_t_lo,
                                         const double* d_p, double* d_t_p, double* d_p_hi, double* d_p_lo,
                                         uint32_t* d_flag, hipStream_t s) {
  if (!mb) return hipSuccess;
  hs_pssm_null_threshold_kernel<<<(mb + 63u) / 64u, 64, 0, s>>>(reinterpret_cast<const hs_pssm_null_prof*>(d_prof), d_cdf,
                                                               mb, B, hs_pssm_null_e(k, alphabet), sides, d_t_lo, d_p,
                                                               d_t_p, d_p_hi, d_p_lo, d_flag);
  return hipGetLastError();
}
