// hs_join6_tables.h -- the tables and thresholds of the FP6 (e2m3) bucket-join filter (hs_join6.hip), as
// __host__ __device__ routines: the device builds them beside hs_jtables8_kernel, the host exports them
// (hs_join6_tables, hs_join6_thresholds) so that the bound is tested where there is no GPU.
//
// The bound.  x_a = row a of the coordinate table, columns 0..3; s = 7.5 / max |x|; X^[a][j] = the e2m3 value
// nearest to s x_a[j]; S[a][b] = X^[a].X^[b]; E[a][b] = s^2 x_a.x_b - S[a][b].  e[] with e[a] + e[b] >= E[a][b]
// for EVERY residue pair (hs_j6_compute finds a minimal one), r[a] = s^2 |x_a|^2 / 2 - e[a].  Then
//     S[a][b] - r[a] - r[b] >= -(s^2 / 2) |x_a - x_b|^2      for every pair of residues,
// and summed over the k positions of a member x and a query c,
//     F = sum_p S[x_p][c_p] - rho(x) - gamma(c) >= (s^2 / 2) (R^2 - d4^2) >= 0   whenever d^2 <= R^2,
//     rho(x) = sum_p r[x_p],   gamma(c) = sum_p r[c_p] - s^2 R^2 / 2.
// No worst-case rounding term: the error of each of the alphabet^2 residue pairs is in e exactly.
//
// Exactness.  e2m3 values are multiples of 1/8, products of 2^-6; everything below is kept in UNITS of 2^-6
// ("64ths").  rho and gamma are rounded DOWN to 64ths and lowered by one more, so a hit has F >= 2^-6 whatever
// the last bits of the doubles they were summed in.  All sums stay below 2^19 units: exact in fp32.
#pragma once
#include <math.h>
#include <stdint.h>

// what the device kernels read (one block of global memory per handle)
struct hs_j6_dev {
  uint2 pair[1024];   // entry r1 << 5 | r0: the 2 x 24 code bits of both residues (r0 in bits 0..23, r1 in 24..47)
  double r[32];       // r[a] (rows >= alphabet: 0)
  uint32_t bits[32];  // the 4 six-bit codes of residue a, column j at bit 6 j
  double s2_half;     // s^2 / 2
  int32_t rpos64;     // rho is carried relative to rho0 = k * rpos64 (64ths); gamma takes the difference
  int32_t ok;         // 0: the table has no usable scale (all zero, NaN, huge)
};

// rho slots of a member's record, against constant factors on the query side: NC coarse slots (factor 7.5,
// digits multiples of 1/2 within +-7.5: steps of 240 64ths), one medium (factor 1/2, digit a multiple of 1/2
// up to 7: steps of 16) and one fine (factor 1/8, digit a multiple of 1/8 up to 15/8: steps of 1)
#define HS_J6_NC 15
#define HS_J6_QMAX (15 * HS_J6_NC)

// e2m3: sign, 2 exponent bits, 3 mantissa bits; value in eighths
__host__ __device__ inline int hs_e2m3_eighths(uint32_t c) {
  const int m = (int)(c & 7u), e = (int)((c >> 3) & 3u);
  const int v = e ? (8 + m) << (e - 1) : m;
  return (c & 32u) ? -v : v;
}
// code of a value given in eighths that IS on the grid (|v| <= 15; even up to 30; a multiple of 4 up to 60)
__host__ __device__ inline uint32_t hs_e2m3_code(int v8) {
  const uint32_t sg = v8 < 0 ? 32u : 0u;
  const uint32_t a = (uint32_t)(v8 < 0 ? -v8 : v8);
  return sg | (a < 16u ? a : a < 32u ? (a >> 1) + 8u : (a >> 2) + 16u);
}
// code of the grid value nearest to v (|v| beyond 7.5 saturates)
__host__ __device__ inline uint32_t hs_e2m3_nearest(double v) {
  const double a = fabs(v);
  uint32_t best = 0;
  double bd = a;
  for (uint32_t c = 1; c < 32u; ++c) {
    const double d = fabs(a - 0.125 * (double)hs_e2m3_eighths(c));
    if (d < bd) {
      bd = d;
      best = c;
    }
  }
  return best | ((v < 0.0 && best) ? 32u : 0u);
}

// The tables from the coordinate table.  e_out / s_out: optional.
__host__ __device__ inline void hs_j6_compute(const double* coords, int alphabet, hs_j6_dev* T, double* e_out,
                                              double* s_out) {
  double mm = 0.0;
  for (int a = 0; a < alphabet && a < 32; ++a)
    for (int j = 0; j < 4; ++j) mm = fmax(mm, fabs(coords[a * 8 + j]));
  T->ok = (mm > 0.0 && mm < 1e6 && alphabet >= 1 && alphabet <= 32) ? 1 : 0;
  if (!T->ok) mm = 1.0;
  const double s = 7.5 / mm;
  int X8[32][4];
  double e[32];
  for (int a = 0; a < 32; ++a) {
    uint32_t b = 0;
    for (int j = 0; j < 4; ++j) {
      const uint32_t c = (a < alphabet && T->ok) ? hs_e2m3_nearest(s * coords[a * 8 + j]) : 0u;
      X8[a][j] = hs_e2m3_eighths(c);
      b |= c << (6 * j);
    }
    T->bits[a] = b;
    e[a] = 0.0;
    T->r[a] = 0.0;
  }
  auto E = [&](int a, int b) {
    double dot = 0.0;
    int S = 0;
    for (int j = 0; j < 4; ++j) {
      dot += coords[a * 8 + j] * coords[b * 8 + j];
      S += X8[a][j] * X8[b][j];
    }
    return s * s * dot - (double)S / 64.0;
  };
  if (T->ok) {
    for (int a = 0; a < alphabet; ++a) {
      double m = E(a, a);
      for (int b = 0; b < alphabet; ++b) m = fmax(m, E(a, b));
      e[a] = 0.5 * m;
    }
    // lower each e[a] in turn to the least value its constraints allow, until nothing moves (every state on the
    // way satisfies all constraints; the values only fall and are bounded below)
    for (int sweep = 0; sweep < 200; ++sweep) {
      bool moved = false;
      for (int a = 0; a < alphabet; ++a) {
        double need = 0.5 * E(a, a);
        for (int b = 0; b < alphabet; ++b)
          if (b != a) need = fmax(need, E(a, b) - e[b]);
        if (need < e[a]) {
          e[a] = need;
          moved = true;
        }
      }
      if (!moved) break;
    }
    // (E is evaluated in doubles: a hair of room, far below the 2^-6 the thresholds are lowered by)
    for (int a = 0; a < alphabet; ++a) e[a] += 9.094947017729282e-13;  // 2^-40
  }
  double rmin = 0.0, rmax = 0.0;
  for (int a = 0; a < alphabet && a < 32; ++a) {
    double n = 0.0;
    for (int j = 0; j < 4; ++j) n += coords[a * 8 + j] * coords[a * 8 + j];
    T->r[a] = T->ok ? 0.5 * s * s * n - e[a] : 0.0;
    if (a == 0 || T->r[a] < rmin) rmin = T->r[a];
    if (a == 0 || T->r[a] > rmax) rmax = T->r[a];
  }
  // rho0 per position: the middle of r's range, but no further above its minimum than the coarse digits reach
  // DOWN at k = 25 (a rho below its slots' range could only be clamped the forbidden way)
  const int32_t rmin64 = (int32_t)floor(rmin * 64.0), rmax64 = (int32_t)floor(rmax * 64.0);
  int32_t mid = rmin64 + (rmax64 - rmin64) / 2;
  if (mid > rmin64 + 2160) mid = rmin64 + 2160;  // 25 * 2160 = 54000 < 240 * HS_J6_QMAX
  T->rpos64 = mid;
  T->s2_half = 0.5 * s * s;
  for (int i = 0; i < 1024; ++i) {
    const uint64_t v = (uint64_t)T->bits[i & 31] | ((uint64_t)T->bits[i >> 5] << 24);
    T->pair[i].x = (uint32_t)v;
    T->pair[i].y = (uint32_t)(v >> 32);
  }
  if (e_out)
    for (int a = 0; a < 32; ++a) e_out[a] = e[a];
  if (s_out) *s_out = s;
}

// six bits into a 128-bit little-endian word
__host__ __device__ inline void hs_j6_put(uint32_t (&w)[4], int bit, uint32_t c) {
  const int i = bit >> 5, sh = bit & 31;
  w[i] |= c << sh;
  if (sh > 26 && i < 3) w[i + 1] |= c >> (32 - sh);
}

// A member's 16-byte record: bits 0..23 the codes of position 24 (0 if the k-mer has none), then the 17 rho
// slots, 6 bits each.  rho = sum_p r[x_p] as summed by the caller; what the slots stand for comes back in
// 64ths (*enc64): floor(64 rho) - 1, or less where the digits cannot reach it (clamped: more permissive).
__host__ __device__ inline void hs_j6_record(double rho, int k, int32_t rpos64, uint32_t pos24_bits,
                                             uint32_t (&rec)[4], int64_t* enc64) {
  const int64_t v64 = (int64_t)floor(rho * 64.0) - 1, rho0 = (int64_t)k * rpos64;
  const int64_t w = rho0 - v64;  // the slots add up to -(rho - rho0)
  int64_t Q = w >= 0 ? w / 240 : -((-w + 239) / 240);
  int64_t rem = w - 240 * Q;
  if (Q < -HS_J6_QMAX) {  // rho above the digits' range: a lower rho stands for it
    Q = -HS_J6_QMAX;
    rem = 0;
  }
  if (Q > HS_J6_QMAX) {  // (not reachable for k <= 25: rho >= k rmin, and rho0 <= k rmin + 54000 / 64)
    Q = HS_J6_QMAX;
    rem = 239;
  }
  if (enc64) *enc64 = rho0 - (240 * Q + rem);
  rec[0] = pos24_bits & 0xffffffu;
  rec[1] = rec[2] = rec[3] = 0u;
  for (int j = 0; j < HS_J6_NC; ++j) {
    const int take = (int)(Q > 15 ? 15 : Q < -15 ? -15 : Q);
    Q -= take;
    hs_j6_put(rec, 24 + 6 * j, hs_e2m3_code(4 * take));
  }
  hs_j6_put(rec, 24 + 6 * HS_J6_NC, hs_e2m3_code(4 * (int)(rem >> 4)));
  hs_j6_put(rec, 24 + 6 * (HS_J6_NC + 1), hs_e2m3_code((int)(rem & 15)));
}

// The constant factors of the rho slots, as the bits 24.. of the fourth quarter of a query's row (6 dwords):
// 7.5 (code 31) fifteen times, 1/2 (code 4), 1/8 (code 1)
__host__ __device__ inline void hs_j6_query_consts(uint32_t (&w)[6]) {
  for (int i = 0; i < 6; ++i) w[i] = 0u;
  for (int j = 0; j < HS_J6_NC + 2; ++j) {
    const uint32_t c = j < HS_J6_NC ? 31u : j == HS_J6_NC ? 4u : 1u;
    const int bit = 24 + 6 * j, i = bit >> 5, sh = bit & 31;
    w[i] |= c << sh;
    if (sh > 26) w[i + 1] |= c >> (32 - sh);
  }
}

// The query's threshold: C = -(gamma + rho0) in 64ths, gamma = floor(64 (sum_p r[c_p] - s^2 R^2 / 2)) - 1.
// The kernel passes C / 64 as a float: exact while |C| < 2^24 (HS_J6_CMAX keeps every partial sum there too).
#define HS_J6_CMAX (1 << 23)
__host__ __device__ inline int64_t hs_j6_query_c64(double sum_r, double s2_half, double r2, int k, int32_t rpos64) {
  const double g = sum_r - s2_half * r2;
  const int64_t g64 = (int64_t)floor(g * 64.0) - 1;
  return -(g64 + (int64_t)k * rpos64);
}

// The query rows in segment order (hs_gather_c6t_kernel writes them, hs_join6x_kernel reads them).  A row is 8
// pieces of 16 bytes: piece g < 4 = dwords 0..3 of lane quarter g, piece 4 + g = {dwords 4, 5 of quarter g, C, C}.
// Tiles of 32 rows are densely packed, tile t of a segment at 128 bytes x (the segment's first row + 32 t); the
// byte offset of piece g of row j inside a tile of nr rows:
//   full (nr = 32)   four planes of 1 KB in the kernel's lane order: plane 2 c + (g >> 2) holds the piece of row
//                    16 c + n, quarter q = g & 3 at byte 16 (16 q + n) -- lane 16 q + n loads its operand of
//                    column tile c at 16 lane + 1024 (2 c) and + 1024 (2 c + 1), with no address arithmetic
//   ragged (nr < 32) piece-major, piece g of row j at 16 (g nr + j): the last tile of a segment, nr x 128 bytes
#define HS_J6_ROW_BYTES 128
// members per work item of hs_join6w_kernel (12 row tiles of 16; hs_join6x_kernel: 128, hs_join8_members_per_item)
#define HS_J6_WIDE_ITEM 192u
__host__ __device__ inline uint32_t hs_j6_tile_offset(uint32_t nr, uint32_t j, uint32_t g) {
  if (nr == 32u) return ((2u * (j >> 4) + (g >> 2)) << 10) + 16u * (16u * (g & 3u) + (j & 15u));
  return 16u * (g * nr + j);
}
