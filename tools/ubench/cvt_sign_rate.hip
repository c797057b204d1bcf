// Microbenchmark: what the group test of hs_join6x_kernel costs beside its MFMAs, in two forms.  One phase = 8
// v_mfma_f32_16x16x128_f8f6f4 (e2m3 operands, random data) into one accumulator half, beside the test of the other
// half's 32 accumulators; two phases per 128 x 32 tile, 2 waves per SIMD as in the kernel.
//   form 0: no test (the MFMAs alone)
//   form 1: the tree of three-input maxima on the floats' bit patterns, two steps behind each MFMA (16 v_max3_i32 +
//           v_cmp), as hs_join6x_kernel tests accumulators that start at C
//   form 2: v_cvt_scalef32_2xpk16_fp6_f32 turns the 32 accumulators into 32 six-bit values that keep their signs
//           (6 registers; a scale that saturates every non-zero value), "some accumulator is non-negative" is then
//           three ANDs of register pairs, the sign masks and a compare
// Prints cycles per phase and wave, and the clock the chip held.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
typedef int intx6 __attribute__((ext_vector_type(6)));
typedef int intx8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

__device__ __forceinline__ void max_step(int g, const floatx4 (&acc)[4][2], int (&w)[16]) {
  auto v = [&](int i) { return __float_as_int(acc[i >> 3][(i >> 2) & 1][i & 3]); };
  if (g < 10) w[g] = max(max(v(3 * g), v(3 * g + 1)), v(3 * g + 2));
  else if (g < 13) w[g] = max(max(w[3 * (g - 10)], w[3 * (g - 10) + 1]), w[3 * (g - 10) + 2]);
  else if (g == 13) w[13] = max(max(w[9], v(30)), v(31));
  else if (g == 14) w[14] = max(max(w[10], w[11]), w[12]);
  else w[15] = max(w[13], w[14]);
  asm volatile("" : "+v"(w[g]));
}

// bits 6 i + 5 of the 192 bits of six registers: the sign of six-bit value i (the pattern repeats every 3 registers)
constexpr uint32_t sign_mask(int r) {
  uint32_t m = 0;
  for (int b = 0; b < 32; ++b)
    if ((32 * r + b) % 6 == 5) m |= 1u << b;
  return m;
}

__device__ __forceinline__ bool cvt_test(const floatx4 (&acc)[4][2]) {
  floatx16 a, b;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[4 * t + i] = acc[t][0][i];
      b[4 * t + i] = acc[t][1][i];
    }
  // scale 2^-126: every value that is not +-0 saturates to +-7.5, the sign survives
  const intx6 p = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, __uint_as_float(0x00800000u));
  const uint32_t u0 = (uint32_t)(p[0] & p[3]), u1 = (uint32_t)(p[1] & p[4]), u2 = (uint32_t)(p[2] & p[5]);
  const uint32_t all = (u0 | ~sign_mask(0)) & (u1 | ~sign_mask(1)) & (u2 | ~sign_mask(2));
  return all != 0xffffffffu;  // some sign bit clear: some accumulator non-negative
}

template <int FORM>
__global__ __launch_bounds__(256, 2) void k(int iters, const uint4* __restrict__ rnd, int* out,
                                            unsigned long long* cyc) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  intx8 A[8], B[2];
  for (int i = 0; i < 8; ++i) {
    const uint4 v = rnd[(gid * 16 + 2 * i) & 0xfffff], w = rnd[(gid * 16 + 2 * i + 1) & 0xfffff];
    A[i] = intx8{(int)v.x, (int)v.y, (int)v.z, (int)v.w, (int)w.x, (int)w.y, 0, 0};
  }
  for (int i = 0; i < 2; ++i) {
    const uint4 v = rnd[(gid * 4 + 2 * i + 77777) & 0xfffff], w = rnd[(gid * 4 + 2 * i + 77778) & 0xfffff];
    B[i] = intx8{(int)v.x, (int)v.y, (int)v.z, (int)v.w, (int)w.x, (int)w.y, 0, 0};
  }
  const float c = -4096.0f;  // (a threshold no pair passes: the test never leaves the no-survivor path)
  const floatx4 C = floatx4{c, c, c, c};
  floatx4 X[4][2], Y[4][2];
  for (int t = 0; t < 4; ++t)
    for (int j = 0; j < 2; ++j) X[t][j] = Y[t][j] = C;
  uint32_t keep = 0;
  const uint64_t t0 = __builtin_readcyclecounter();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      floatx4 (&W)[4][2] = ph ? Y : X;        // written by this phase's MFMAs
      const floatx4 (&T)[4][2] = ph ? X : Y;  // tested beside them
      int w[16];
      bool pass = false;
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        W[g >> 1][g & 1] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A[4 * ph + (g >> 1)], B[g & 1], C, 2, 2, 0, 0,
                                                                           0, 0);
        if (FORM == 1) {
          max_step(2 * g, T, w);
          max_step(2 * g + 1, T, w);
        }
        if (FORM == 2 && g == 3) pass = cvt_test(T);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (FORM == 1) pass = w[15] >= 0;
      if (__ballot(pass)) keep += 1u + (uint32_t)ph;
    }
    B[0][0] ^= (int)(keep & 1u);  // loop-carried, keeps the data moving
  }
  const uint64_t t1 = __builtin_readcyclecounter();
  if (keep == 0xdeadbeef || FORM == 0) {
    float s = 0.0f;
    for (int t = 0; t < 4; ++t)
      for (int j = 0; j < 2; ++j) s += X[t][j][0] + Y[t][j][1];
    if (s == 12345.678f) out[threadIdx.x] = (int)keep;
  }
  if ((threadIdx.x & 63) == 0) atomicAdd(cyc, (unsigned long long)(t1 - t0));
}

int main() {
  int* out; unsigned long long* cyc; uint4* rnd;
  CK(hipMalloc(&out, 4096)); CK(hipMalloc(&cyc, 8)); CK(hipMalloc(&rnd, (1 << 20) * 16));
  uint32_t* h = (uint32_t*)malloc((1 << 20) * 16);
  uint64_t x = 88172645463325252ull;
  for (int i = 0; i < (1 << 22); ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; h[i] = (uint32_t)(x >> 16); }
  CK(hipMemcpy(rnd, h, (1 << 20) * 16, hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int iters = 20000;
  const char* name[3] = {"MFMAs alone", "v_max3_i32 tree", "cvt to fp6 + sign masks"};
  for (int rep = 0; rep < 3; ++rep)
    for (int form = 0; form < 3; ++form) {
      CK(hipMemset(cyc, 0, 8));
      CK(hipEventRecord(e0));
      if (form == 0) k<0><<<512, 256>>>(iters, rnd, out, cyc);
      else if (form == 1) k<1><<<512, 256>>>(iters, rnd, out, cyc);
      else k<2><<<512, 256>>>(iters, rnd, out, cyc);
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      unsigned long long c; CK(hipMemcpy(&c, cyc, 8, hipMemcpyDeviceToHost));
      const double waves = 2048.0;
      printf("%-24s %.3f ms, %.1f cycles per phase of 8 MFMAs per wave, clock %.2f GHz\n", name[form], ms,
             (double)c / waves / iters / 2.0, (double)c / waves / (ms * 1e-3) / 1e9);
    }
  return 0;
}
