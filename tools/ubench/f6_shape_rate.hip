// Microbenchmark: the FP6 join's tile loop in the two MFMA shapes, at the same work per tile and the same number of
// other vector instructions.  One tile = 128 members x 32 queries at depth 128 (e2m3 operands, random data), written as
// two accumulator halves; the test of one half sits behind the MFMAs of the other, every instruction pinned where it is
// written.  2 waves per SIMD, as in hs_join6x_kernel, and a threshold nothing passes (the no-survivor path).
//   A60  16 x v_mfma_f32_16x16x128_f8f6f4, the tree of 32 v_max3_f32 + 4 compares, 24 independent filler VALU: the 60
//        other vector instructions per tile that the kernel had before r09
//   A48  the same with 12 fillers
//   B60  8 x v_mfma_f32_32x32x64_f8f6f4 (k-step 0 with C = 0, k-step 1 accumulating, order t0s0 t1s0 t0s1 t1s1),
//        32 v_max3_f32 + 2 compares, 26 fillers
//   B48  the same with 14 fillers
//   A0 / B0  the MFMAs alone
// The fillers are spread evenly over the gaps (16 per tile in A, 8 in B).
// Prints WALL time per tile and SIMD from HIP events (a SIMD runs two waves, so two tiles per iteration): the cycle
// counter that cvt_sign_rate.hip reads does not tick at the shader clock.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
typedef int intx8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

constexpr int NF = 8;  // filler registers, used in turn: neighbouring fillers are independent
__device__ __forceinline__ float max3f(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

// fillers of gap g of GAPS: an even share of NFILL
template <int NFILL, int GAPS>
__device__ __forceinline__ void fillers(int g, uint32_t (&f)[NF], uint32_t salt) {
  if (NFILL <= 0) return;
  const int lo = g * NFILL / GAPS, hi = (g + 1) * NFILL / GAPS;
#pragma unroll
  for (int j = lo; j < hi; ++j) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(f[j % NF]) : "v"(salt));
}

// Step g of 16 of the maximum of 32 values v(0..31) on three-input maxima; the result is w[15].
template <class V>
__device__ __forceinline__ void max_step32(int g, V v, float (&w)[16]) {
  if (g < 10) w[g] = max3f(v(3 * g), v(3 * g + 1), v(3 * g + 2));
  else if (g < 13) w[g] = max3f(w[3 * (g - 10)], w[3 * (g - 10) + 1], w[3 * (g - 10) + 2]);
  else if (g == 13) w[13] = max3f(w[9], v(30), v(31));
  else if (g == 14) w[14] = max3f(w[10], w[11], w[12]);
  else w[15] = max3f(w[13], w[14], v(31));  // (v(31) a second time: a two-input maximum of values the compiler
                                            // cannot trace costs two more instructions)
  asm volatile("" : "+v"(w[g]));
}
// Step g of 16 as hs_join6x_kernel's 16x16 form has it: two trees of 16 values (one per column tile), 8 steps each,
// results in w[7] and w[15]
__device__ __forceinline__ void max_step16(int g, const floatx4 (&acc)[4][2], float (&w)[16]) {
  const int c = g >> 3, s = g & 7, o = 8 * c;
  auto v = [&](int i) { return acc[i >> 2][c][i & 3]; };
  if (s < 5) w[g] = max3f(v(3 * s), v(3 * s + 1), v(3 * s + 2));
  else if (s == 5) w[g] = max3f(w[o], w[o + 1], w[o + 2]);
  else if (s == 6) w[g] = max3f(w[o + 3], w[o + 4], v(15));
  else w[g] = max3f(w[o + 5], w[o + 6], v(15));
  asm volatile("" : "+v"(w[g]));
}

// The wave's ballot of m >= thr: one compare written to a scalar pair
__device__ __forceinline__ uint64_t passed(float m, float thr) {
  uint64_t b;
  asm volatile("v_cmp_ge_f32_e64 %0, %1, %2" : "=s"(b) : "v"(m), "v"(thr));
  return b;
}

__device__ __forceinline__ intx8 rnd6(const uint4* __restrict__ rnd, uint32_t i) {
  const uint4 v = rnd[(2 * i) & 0xfffff], w = rnd[(2 * i + 1) & 0xfffff];
  return intx8{(int)v.x, (int)v.y, (int)v.z, (int)v.w, (int)w.x, (int)w.y, 0, 0};
}

// SHAPE 0: 16x16x128, SHAPE 1: 32x32x64.  NFILL < 0: no test either.
template <int SHAPE, int NFILL>
__global__ __launch_bounds__(256, 2) void k(int iters, const uint4* __restrict__ rnd, int* out, float thr0, float thr1) {
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  constexpr bool TEST = NFILL >= 0;
  uint32_t f[NF];
  for (int i = 0; i < NF; ++i) f[i] = gid + i;
  const uint32_t salt = gid * 2654435761u;
  uint32_t keep = 0;
  asm volatile("" : "+v"(thr0), "+v"(thr1));  // per lane, as the kernel's C is
  if (SHAPE == 0) {
    intx8 A[8], B[2];
    for (int i = 0; i < 8; ++i) A[i] = rnd6(rnd, gid * 8 + i);
    for (int i = 0; i < 2; ++i) B[i] = rnd6(rnd, gid * 2 + i + 77777);
    const floatx4 zero = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    floatx4 X[4][2], Y[4][2];
    for (int t = 0; t < 4; ++t)
      for (int j = 0; j < 2; ++j) X[t][j] = Y[t][j] = zero;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        floatx4 (&W)[4][2] = ph ? Y : X;        // written by this phase's MFMAs
        const floatx4 (&T)[4][2] = ph ? X : Y;  // tested beside them
        float w[16];
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          W[g >> 1][g & 1] =
              __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A[4 * ph + (g >> 1)], B[g & 1], zero, 2, 2, 0, 0, 0, 0);
          if (TEST) {
            max_step16(2 * g, T, w);
            max_step16(2 * g + 1, T, w);
          }
          fillers<NFILL, 16>(8 * ph + g, f, salt);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (TEST && (passed(w[7], thr0) | passed(w[15], thr1))) keep += 1u + (uint32_t)ph;
      }
      B[0][0] ^= (int)(keep & 1u);  // loop-carried, keeps the data moving
    }
    float s = 0.0f;
    for (int t = 0; t < 4; ++t)
      for (int j = 0; j < 2; ++j) s += X[t][j][0] + Y[t][j][1];
    if (s == 12345.678f) keep ^= 1u;
  } else {
    intx8 A[4][2], B[2];  // A[row tile][k-step], B[k-step]
    for (int i = 0; i < 8; ++i) A[i >> 1][i & 1] = rnd6(rnd, gid * 8 + i);
    for (int i = 0; i < 2; ++i) B[i] = rnd6(rnd, gid * 2 + i + 77777);
    floatx16 zero;
    for (int i = 0; i < 16; ++i) zero[i] = 0.0f;
    floatx16 X[2], Y[2];
    for (int t = 0; t < 2; ++t) X[t] = Y[t] = zero;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        floatx16 (&W)[2] = ph ? Y : X;
        const floatx16 (&T)[2] = ph ? X : Y;
        auto v = [&](int i) { return T[i >> 4][i & 15]; };
        float w[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int t = g & 1, s = g >> 1;
          W[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A[2 * ph + t][s], B[s], s ? W[t] : zero, 2, 2, 0, 0, 0,
                                                                  0);
          if (TEST) {
#pragma unroll
            for (int j = 0; j < 4; ++j) max_step32(4 * g + j, v, w);
          }
          fillers<NFILL, 8>(4 * ph + g, f, salt);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (TEST && passed(w[15], thr0)) keep += 1u + (uint32_t)ph;
      }
      B[0][0] ^= (int)(keep & 1u);
    }
    float s = 0.0f;
    for (int t = 0; t < 2; ++t) s += X[t][0] + Y[t][1];
    if (s == 12345.678f) keep ^= 1u;
  }
  uint32_t fx = 0;
  for (int i = 0; i < NF; ++i) fx ^= f[i];
  if (keep == 0xdeadbeefu || fx == 0x12345678u) out[threadIdx.x] = (int)(keep + fx);
}

int main() {
  int* out; uint4* rnd;
  CK(hipMalloc(&out, 4096)); CK(hipMalloc(&rnd, (1 << 20) * 16));
  uint32_t* h = (uint32_t*)malloc((1 << 20) * 16);
  uint64_t x = 88172645463325252ull;
  for (int i = 0; i < (1 << 22); ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; h[i] = (uint32_t)(x >> 16); }
  CK(hipMemcpy(rnd, h, (1 << 20) * 16, hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int iters = 20000;
  const float thr0 = 1.0e9f, thr1 = 2.0e9f;  // (no sum of 128 products of e2m3 values comes near: no test passes)
  const char* name[6] = {"A60", "B60", "A48", "B48", "A0", "B0"};
  const char* what[6] = {"16 x 16x16x128, 32 max3 + 4 cmp + 24 fillers", "8 x 32x32x64, 32 max3 + 2 cmp + 26 fillers",
                         "16 x 16x16x128, 32 max3 + 4 cmp + 12 fillers", "8 x 32x32x64, 32 max3 + 2 cmp + 14 fillers",
                         "16 x 16x16x128 alone", "8 x 32x32x64 alone"};
  printf("512 workgroups of 256, 2 waves per SIMD, %d tiles of 128 x 32 x 128 per wave; wall time from HIP events\n",
         iters);
  for (int rep = -1; rep < 3; ++rep)  // (rep -1: warm-up, not printed)
    for (int form = 0; form < 6; ++form) {
      CK(hipEventRecord(e0));
      switch (form) {
        case 0: k<0, 24><<<512, 256>>>(iters, rnd, out, thr0, thr1); break;
        case 1: k<1, 26><<<512, 256>>>(iters, rnd, out, thr0, thr1); break;
        case 2: k<0, 12><<<512, 256>>>(iters, rnd, out, thr0, thr1); break;
        case 3: k<1, 14><<<512, 256>>>(iters, rnd, out, thr0, thr1); break;
        case 4: k<0, -1><<<512, 256>>>(iters, rnd, out, thr0, thr1); break;
        default: k<1, -1><<<512, 256>>>(iters, rnd, out, thr0, thr1); break;
      }
      CK(hipGetLastError());
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (rep < 0) continue;
      const double ns = (double)ms * 1e6 / ((double)iters * 2.0);
      printf("rep %d  %-4s %-46s %8.3f ms  %7.2f ns per tile and SIMD  (%.0f cycles at 2.4 GHz)\n", rep, name[form],
             what[form], ms, ns, ns * 2.4);
    }
  return 0;
}
