// Microbenchmark: what the FP6 join's query-tile stream costs beside its MFMAs, and what sharing a tile buys.
// The tile body is f6_shape_rate.hip's 16x16x128 form (two accumulator halves, the test of one half pinned behind
// the MFMAs of the other, a threshold nothing passes), at hs_join6x_kernel's 53 other vector instructions per tile:
// 32 v_max3_f32 + 4 compares + 13 fillers + the four loads of load_btile6 (arm N: 17 fillers and no load).
//   N  no loads: the floor
//   P  every wave loads its own tiles as the kernel does (dwordx4 + dwordx3 per column tile, three tiles in flight)
//      from per-segment buffers of 640 rows x 128 B, the four waves of a workgroup in the SAME segment at per-wave
//      skewed offsets; the segments together (NSEG x 80 KB = 105 MB) exceed every L2
//   S  the four waves of a workgroup share each tile through LDS: wave w fetches plane w (1 KB, one dwordx4 per lane)
//      of each tile of a group of three a group ahead, stores it with ds_write_b128, and every wave reads its operand
//      back with ds_read_b128 + ds_read_b96 per column tile; two groups of slots, one s_barrier per group
//   D  as S with the plane moved by global_load_lds_dwordx4 (no staging registers, no ds_write)
//   W  barrier-free, 192 members per wave: 24 MFMAs per 4 KB tile, accumulator halves of 6 row tiles, 48 v_max3_f32 +
//      4 compares + 13 fillers + the four loads.  Its line is printed per 16 MFMAs (time per tile x 16 / 24) so that
//      every arm's figure is the time of the same work
// The memory instructions of S and D (6 and 5 per tile) come ON TOP of the 13 fillers: the arm pays for them.
// 512 workgroups of 256, 2 waves per SIMD, fixed trip counts, wall time from HIP events, three repetitions with the
// arms alternating.  Prints ns per tile and SIMD (a SIMD runs two waves: two tiles per iteration).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
typedef int intx3 __attribute__((ext_vector_type(3)));
typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx6 __attribute__((ext_vector_type(6)));
typedef int intx8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

constexpr int NF = 8;            // filler registers, used in turn
constexpr int SEG_TILES = 20;    // 640 rows of 128 B = 20 tiles of 4 KB
constexpr int SEG_GROUPS = 7;    // groups of three tiles a wave walks per segment (the last wraps to tile 0)
constexpr uint32_t SEG_BYTES = SEG_TILES * 4096u;
constexpr uint32_t NSEG = 1280;  // 105 MB of rows
constexpr int GRID = 512;
constexpr int LDS_PAD = 56 * 1024;  // LDS per workgroup, used or not: a CU takes two workgroups, so a SIMD two waves

__device__ __forceinline__ float max3f(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

template <int NFILL, int GAPS>
__device__ __forceinline__ void fillers(int g, uint32_t (&f)[NF], uint32_t salt) {
  const int lo = g * NFILL / GAPS, hi = (g + 1) * NFILL / GAPS;
#pragma unroll
  for (int j = lo; j < hi; ++j) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(f[j % NF]) : "v"(salt));
}

// Step g of 4 HALF of the two maxima (one per column tile) of a half's 16 HALF accumulators on three-input maxima:
// 2 HALF steps per column tile, the results in w[2 HALF - 1] and w[4 HALF - 1].  HALF = 4 is sign_step6.
template <int HALF>
__device__ __forceinline__ void max_step(int g, const floatx4 (&acc)[HALF][2], float (&w)[4 * HALF]) {
  constexpr int S = 2 * HALF;
  const int c = g / S, s = g % S, o = S * c;
  auto v = [&](int i) { return acc[i >> 2][c][i & 3]; };
  if constexpr (HALF == 4) {
    if (s < 5) w[g] = max3f(v(3 * s), v(3 * s + 1), v(3 * s + 2));
    else if (s == 5) w[g] = max3f(w[o], w[o + 1], w[o + 2]);
    else if (s == 6) w[g] = max3f(w[o + 3], w[o + 4], v(15));
    else w[g] = max3f(w[o + 5], w[o + 6], v(15));
  } else {  // 24 values: 8 + 3 + 1
    if (s < 8) w[g] = max3f(v(3 * s), v(3 * s + 1), v(3 * s + 2));
    else if (s < 10) w[g] = max3f(w[o + 3 * (s - 8)], w[o + 3 * (s - 8) + 1], w[o + 3 * (s - 8) + 2]);
    else if (s == 10) w[g] = max3f(w[o + 6], w[o + 7], v(23));
    else w[g] = max3f(w[o + 8], w[o + 9], w[o + 10]);
  }
  asm volatile("" : "+v"(w[g]));
}

__device__ __forceinline__ uint64_t passed(float m, float thr) {
  uint64_t b;
  asm volatile("v_cmp_ge_f32_e64 %0, %1, %2" : "=s"(b) : "v"(m), "v"(thr));
  return b;
}

__device__ __forceinline__ floatx4 mfma6(const intx6 a, const intx8 b, const floatx4 c) {
  const intx8 a8 = __builtin_shufflevector(a, a, 0, 1, 2, 3, 4, 5, -1, -1);
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b, c, 2, 2, 0, 0, 0, 0);
}

// One tile: 2 x 2 HALF MFMAs, the test of the other half behind them, NFILL fillers spread over the gaps
template <int HALF, int NFILL>
__device__ __forceinline__ void tile_body(const intx6 (&A)[2 * HALF], const intx8 (&B)[2], floatx4 (&X)[HALF][2],
                                          floatx4 (&Y)[HALF][2], float thr0, float thr1, uint32_t (&f)[NF],
                                          uint32_t salt, uint32_t& keep) {
  const floatx4 zero = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int ph = 0; ph < 2; ++ph) {
    floatx4 (&W)[HALF][2] = ph ? Y : X;
    const floatx4 (&T)[HALF][2] = ph ? X : Y;
    float w[4 * HALF];
#pragma unroll
    for (int g = 0; g < 2 * HALF; ++g) {
      W[g >> 1][g & 1] = mfma6(A[HALF * ph + (g >> 1)], B[g & 1], zero);
      max_step<HALF>(2 * g, T, w);
      max_step<HALF>(2 * g + 1, T, w);
      // (the first filler of a tile's first two gaps takes the column tile's seventh dword, the kernel's C: the
      // load of that dword stays)
      fillers<NFILL, 4 * HALF>(2 * HALF * ph + g, f, ph == 0 && g < 2 ? (uint32_t)B[g][6] : salt);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (passed(w[2 * HALF - 1], thr0) | passed(w[4 * HALF - 1], thr1)) keep += 1u + (uint32_t)ph;
  }
}

// the kernel's four loads of a tile: lane's pieces of column tile c at 16 lane + 2048 c (+ 1024, three dwords)
__device__ __forceinline__ void load_tile(intx8 (&B)[2], const char* __restrict__ t0, int lane) {
  const char* base = t0 + 16 * lane;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const intx4 hi = *reinterpret_cast<const intx4*>(base + 2048 * c);
    const intx3 lo = *reinterpret_cast<const intx3*>(base + 2048 * c + 1024);
    B[c] = intx8{hi.x, hi.y, hi.z, hi.w, lo.x, lo.y, lo.z, 0};
  }
}
__device__ __forceinline__ void read_tile_lds(intx8 (&B)[2], const char* slot, int lane) {
  const char* base = slot + 16 * lane;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const intx4 hi = *reinterpret_cast<const intx4*>(base + 2048 * c);
    const intx3 lo = *reinterpret_cast<const intx3*>(base + 2048 * c + 1024);
    B[c] = intx8{hi.x, hi.y, hi.z, hi.w, lo.x, lo.y, lo.z, 0};
  }
}

// Tile u of group gg of a walk that starts in segment seg0 at group `first`: a segment per SEG_GROUPS groups
__device__ __forceinline__ const char* tile_addr(const char* __restrict__ rows, uint32_t seg0, uint32_t first,
                                                 uint32_t gg, uint32_t u) {
  const uint32_t pass = gg / SEG_GROUPS, gi = gg % SEG_GROUPS;
  const uint32_t seg = (seg0 + pass * GRID) % NSEG;
  const uint32_t grp = (first + gi) % SEG_GROUPS;
  const uint32_t t = (3u * grp + u) % SEG_TILES;
  return rows + (uint64_t)seg * SEG_BYTES + t * 4096u;
}

enum { ARM_N = 0, ARM_P = 1, ARM_S = 2, ARM_D = 3, ARM_W = 4 };

template <int ARM, int HALF, int NFILL>
__global__ __launch_bounds__(256, 2) void k(uint32_t n_groups, const char* __restrict__ rows,
                                            const uint4* __restrict__ rnd, int* out, float thr0, float thr1) {
  __shared__ __attribute__((aligned(16))) char ring[(ARM == ARM_S || ARM == ARM_D) ? 2 * 3 * 4096 : 16];
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t f[NF];
  for (int i = 0; i < NF; ++i) f[i] = gid + i;
  const uint32_t salt = gid * 2654435761u;
  uint32_t keep = 0;
  asm volatile("" : "+v"(thr0), "+v"(thr1));  // per lane, as the kernel's C is
  intx6 A[2 * HALF];
  for (int i = 0; i < 2 * HALF; ++i) {
    const uint4 v = rnd[(2 * (gid * 16 + i)) & 0xfffff], w = rnd[(2 * (gid * 16 + i) + 1) & 0xfffff];
    A[i] = intx6{(int)v.x, (int)v.y, (int)v.z, (int)v.w, (int)w.x, (int)w.y};
  }
  const floatx4 zero = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
  floatx4 X[HALF][2], Y[HALF][2];
  for (int t = 0; t < HALF; ++t)
    for (int j = 0; j < 2; ++j) X[t][j] = Y[t][j] = zero;
  const uint32_t seg0 = blockIdx.x % NSEG;
  // the kernel's skew, per wave (per workgroup where the waves share their tiles)
  const uint32_t skew_id = (ARM == ARM_S || ARM == ARM_D) ? blockIdx.x * 4u : blockIdx.x * 4u + wave;
  const uint32_t first = (((skew_id * 40503u) & 0xffffu) * SEG_GROUPS) >> 16;

  if (ARM == ARM_N) {
    intx8 B[2];
    for (int i = 0; i < 2; ++i) {
      const uint4 v = rnd[(2 * (gid * 2 + i) + 77777) & 0xfffff], w = rnd[(2 * (gid * 2 + i) + 77778) & 0xfffff];
      B[i] = intx8{(int)v.x, (int)v.y, (int)v.z, (int)v.w, (int)w.x, (int)w.y, (int)w.z, 0};
    }
    for (uint32_t gg = 0; gg < n_groups; ++gg)
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        tile_body<HALF, NFILL>(A, B, X, Y, thr0, thr1, f, salt, keep);
        // loop-carried in BOTH column tiles: with one of them unchanged its 8 products are the same from tile to tile
        // and the compiler computes them once (f6_shape_rate.hip's A arms change B[0] only)
        B[0][0] ^= (int)(keep & 1u);
        B[1][0] ^= (int)((keep >> 1) & 1u);
      }
  } else if (ARM == ARM_P || ARM == ARM_W) {
    intx8 Bq[3][2];
#pragma unroll
    for (int u = 0; u < 3; ++u) load_tile(Bq[u], tile_addr(rows, seg0, first, 0, u), lane);
    for (uint32_t gg = 0; gg < n_groups; ++gg) {
      const uint32_t ng = gg + 1 < n_groups ? gg + 1 : gg;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        tile_body<HALF, NFILL>(A, Bq[u], X, Y, thr0, thr1, f, salt, keep);
        load_tile(Bq[u], tile_addr(rows, seg0, first, ng, u), lane);
      }
    }
  } else {
    // INVARIANT: every wave executes the same number of barriers, n_groups + 1, whatever it computes.
    // Before barrier g every wave has read group g from slots[g & 1] and filled its planes of group g + 1 in
    // slots[(g + 1) & 1]; after it, group g + 2 may overwrite slots[g & 1].
    const uint32_t plane = 1024u * wave + 16u * (uint32_t)lane;
    if (ARM == ARM_S) {
      intx4 R[3];
#pragma unroll
      for (int u = 0; u < 3; ++u)
        *reinterpret_cast<intx4*>(ring + 4096 * u + plane) =
            *reinterpret_cast<const intx4*>(tile_addr(rows, seg0, first, 0, u) + plane);
      {
        const uint32_t g1 = 1 < n_groups ? 1 : 0;
#pragma unroll
        for (int u = 0; u < 3; ++u) R[u] = *reinterpret_cast<const intx4*>(tile_addr(rows, seg0, first, g1, u) + plane);
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      for (uint32_t gg = 0; gg < n_groups; ++gg) {
        char* cur = ring + 12288 * (gg & 1u);
        char* nxt = ring + 12288 * ((gg + 1u) & 1u);
#pragma unroll
        for (int u = 0; u < 3; ++u) *reinterpret_cast<intx4*>(nxt + 4096 * u + plane) = R[u];
        const uint32_t g2 = gg + 2 < n_groups ? gg + 2 : gg;
#pragma unroll
        for (int u = 0; u < 3; ++u) R[u] = *reinterpret_cast<const intx4*>(tile_addr(rows, seg0, first, g2, u) + plane);
        intx8 B[2][2];
        read_tile_lds(B[0], cur, lane);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          if (u < 2) read_tile_lds(B[(u + 1) & 1], cur + 4096 * (u + 1), lane);
          tile_body<HALF, NFILL>(A, B[u & 1], X, Y, thr0, thr1, f, salt, keep);
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
    } else {
      typedef __attribute__((address_space(3))) void* lds_p;
      typedef const __attribute__((address_space(1))) void* glb_p;
#pragma unroll
      for (int u = 0; u < 3; ++u)
        __builtin_amdgcn_global_load_lds((glb_p)(tile_addr(rows, seg0, first, 0, u) + plane),
                                         (lds_p)(ring + 4096 * u + 1024 * wave), 16, 0, 0);
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      for (uint32_t gg = 0; gg < n_groups; ++gg) {
        char* cur = ring + 12288 * (gg & 1u);
        char* nxt = ring + 12288 * ((gg + 1u) & 1u);
        const uint32_t g1 = gg + 1 < n_groups ? gg + 1 : gg;
#pragma unroll
        for (int u = 0; u < 3; ++u)
          __builtin_amdgcn_global_load_lds((glb_p)(tile_addr(rows, seg0, first, g1, u) + plane),
                                           (lds_p)(nxt + 4096 * u + 1024 * wave), 16, 0, 0);
        intx8 B[2][2];
        read_tile_lds(B[0], cur, lane);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          if (u < 2) read_tile_lds(B[(u + 1) & 1], cur + 4096 * (u + 1), lane);
          tile_body<HALF, NFILL>(A, B[u & 1], X, Y, thr0, thr1, f, salt, keep);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
    }
  }
  float s = 0.0f;
  for (int t = 0; t < HALF; ++t)
    for (int j = 0; j < 2; ++j) s += X[t][j][0] + Y[t][j][1];
  if (s == 12345.678f) keep ^= 1u;
  uint32_t fx = 0;
  for (int i = 0; i < NF; ++i) fx ^= f[i];
  if (keep == 0xdeadbeefu || fx == 0x12345678u) out[threadIdx.x] = (int)(keep + fx);
}

int main(int argc, char** argv) {
  const uint32_t n_groups = argc > 1 ? (uint32_t)atoi(argv[1]) : 4900u;  // x 3 tiles per wave
  int* out; uint4* rnd; char* rows;
  const size_t row_bytes = (size_t)NSEG * SEG_BYTES;
  CK(hipMalloc(&out, 4096)); CK(hipMalloc(&rnd, (1 << 20) * 16)); CK(hipMalloc(&rows, row_bytes + 8192));
  uint32_t* h = (uint32_t*)malloc(row_bytes);
  uint64_t x = 88172645463325252ull;
  for (size_t i = 0; i < row_bytes / 4; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; h[i] = (uint32_t)(x >> 16); }
  CK(hipMemcpy(rnd, h, (1 << 20) * 16, hipMemcpyHostToDevice));
  CK(hipMemcpy(rows, h, row_bytes, hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const float thr0 = 1.0e9f, thr1 = 2.0e9f;  // (no sum of 128 products of e2m3 values comes near: no test passes)
  const char* name[5] = {"N", "P", "S", "D", "W"};
  const char* what[5] = {"no loads, 17 fillers", "own tiles, 4 global loads, 13 fillers",
                         "shared through LDS: dwordx4 + ds_write_b128 per plane, 4 ds_reads, 13 fillers",
                         "shared through LDS: global_load_lds_dwordx4 per plane, 4 ds_reads, 13 fillers",
                         "192 members per wave: 24 MFMAs per tile, 4 global loads, 13 fillers; per 16 MFMAs"};
  printf("%d workgroups of 256, 2 waves per SIMD, %u tiles of 32 queries per wave, %u segments of %u B (%.1f MB); "
         "wall time from HIP events\n", GRID, 3 * n_groups, NSEG, SEG_BYTES, (double)row_bytes / 1e6);
  for (int rep = -1; rep < 3; ++rep)  // (rep -1: warm-up, not printed)
    for (int arm = 0; arm < 5; ++arm) {
      CK(hipEventRecord(e0));
      switch (arm) {
        case ARM_N: k<ARM_N, 4, 17><<<GRID, 256, LDS_PAD>>>(n_groups, rows, rnd, out, thr0, thr1); break;
        case ARM_P: k<ARM_P, 4, 13><<<GRID, 256, LDS_PAD>>>(n_groups, rows, rnd, out, thr0, thr1); break;
        case ARM_S: k<ARM_S, 4, 13><<<GRID, 256, LDS_PAD - 24576>>>(n_groups, rows, rnd, out, thr0, thr1); break;
        case ARM_D: k<ARM_D, 4, 13><<<GRID, 256, LDS_PAD - 24576>>>(n_groups, rows, rnd, out, thr0, thr1); break;
        default: k<ARM_W, 6, 13><<<GRID, 256, LDS_PAD>>>(n_groups, rows, rnd, out, thr0, thr1); break;
      }
      CK(hipGetLastError());
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (rep < 0) continue;
      double ns = (double)ms * 1e6 / ((double)(3 * n_groups) * 2.0);
      if (arm == ARM_W) ns *= 16.0 / 24.0;
      printf("rep %d  %-2s %-84s %8.3f ms  %7.2f ns per tile and SIMD\n", rep, name[arm], what[arm], ms, ns);
    }
  return 0;
}
