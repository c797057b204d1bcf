// hs_pssm_compare.hip -- hs_pssm_compare: profile against profile at every offset (the rule, the filter's tables and
// its invariant: hs_pssm_compare.h).
//
// Both operands are dense, so the work is a GEMM per offset: I(x, y, d) = sum over the overlap of q_x * q_y, the int8
// codes of hs_pssm_compare.h on v_mfma_i32_16x16x64_i8.  The accumulators are exact integers, and the pair's largest
// one over the allowed offsets goes through hs_pcmp_pass in fp64.  What passes goes to the exact pass, which alone
// decides.
//
// hs_pcmp_tables_kernel: one wave per profile -- amax and the l1 sum in the header's order (lane l takes the entries
// l, l + 64, ...; the butterfly over the lanes), then the row: `lead` zero bytes, k columns of `stride` bytes (the
// codes of the column's residues, zeros behind them), zeros up to the row's length.  Rows beyond the profiles (the
// tables are padded to whole tiles of 32) are zeros with s = l1 = amax = 0.
//
// hs_pcmp_filter_kernel: a workgroup of four waves takes a tile of 32 X profiles against 32 Y profiles, stages the 32
// X rows (with their zero margins) and the 32 Y rows in LDS once, and every wave owns one 16 x 16 tile of the pairs.
// Lane (n = lane & 15, q = lane >> 4) holds row / column n, bytes 64 s + 16 q .. + 15 of depth step s; result register
// i of the lane is X row 4 q + i, Y column n (the map hs_join8x_kernel runs on).  The Y operand of a step is fixed; the
// X operand of offset d is the same row read (d + k - v) * stride bytes further in, a 16-byte aligned ds_read_b128
// because stride is a multiple of 16.  One MFMA chain per offset leaves I(x, y, d) itself in the accumulators: no
// reduction across lanes; the depth steps that lie wholly outside the offset's overlap are skipped (their Y bytes meet
// zeros only).  The LDS pitch of a row is its length + 16 bytes: 16 rows, read at one column, then fall into 16
// different 16-byte slots of the 256-byte bank row.  After the last offset the pair's largest accumulator is tested;
// survivors are PAIRS {x of the batch, y}, collected by ballot, one reservation (hs_reserve_survivors) per 16 x 16
// tile that has any.  Self mode: pairs with x >= y are masked at emission, tiles with none below the diagonal leave
// at once.
//
// hs_pcmp_exact_kernel: a wave per surviving pair.  Both profiles go to LDS; lane l evaluates the contract's score at
// the offsets number l, l + 64, ... (every column product belongs to exactly one diagonal, so nothing is stored), and
// the wave reduces to the best offset under the tie rule (score descending, then rank 0, -1, +1, -2, ... ascending: a
// total order, so the reduction's shape does not show).  Kept iff best >= t[x]; key = x << 35 | y << 8 | (d + 128),
// which orders like x << 32 | y (one hit per pair) under the 64-bit radix sort and carries the offset; value = the
// score's bits.  With the filter off it runs over all pairs of the batch instead.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "hs_internal.h"
#include "hs_pssm_compare.h"

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));

inline unsigned blocks_for(uint64_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }

// ------------------------------------------------------------------------------------ the tables
__global__ __launch_bounds__(256) void hs_pcmp_tables_kernel(const double* __restrict__ P, uint32_t np, uint32_t np_pad,
                                                             uint32_t k, uint32_t alphabet, uint32_t stride,
                                                             uint32_t lead, uint32_t row, uint32_t* __restrict__ rows,
                                                             hs_pcmp_par* __restrict__ par) {
  const uint32_t lane = threadIdx.x & 63u, idx = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (idx >= np_pad) return;  // (wave-uniform)
  const uint32_t n = k * alphabet;
  const bool live = idx < np;
  const double* const x = P + (size_t)(live ? idx : 0u) * n;
  double amax = 0.0, sum = 0.0;
  if (live)
    for (uint32_t i = lane; i < n; i += 64u) {
      const double a = fabs(x[i]);
      sum = sum + a;
      amax = a > amax ? a : amax;
    }
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    sum = sum + __shfl_xor(sum, w);
    const double o = __shfl_xor(amax, w);
    amax = o > amax ? o : amax;
  }
  const hs_pcmp_par pr = hs_pcmp_par_of(amax, sum);
  if (lane == 0) par[idx] = pr;
  uint32_t* const out = rows + (size_t)idx * (row / 4u);
  const uint32_t body = k * stride;
  for (uint32_t wd = lane; wd < row / 4u; wd += 64u) {
    uint32_t word = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
      const uint32_t b = 4u * wd + j;
      if (live && b >= lead && b - lead < body) {
        const uint32_t p = (b - lead) / stride, r = (b - lead) - p * stride;
        if (r < alphabet) word |= ((uint32_t)hs_pcmp_code(x[p * alphabet + r], pr.s) & 0xffu) << (8u * j);
      }
    }
    out[wd] = word;
  }
}

// ------------------------------------------------------------------------------------ the filter
// xq: the batch's rows [ceil32(mb)][xrow]; yq: the chunk's rows [ceil32(nyc)][yrow]; t, xpar: the batch's; ypar: the
// chunk's.  x_base, y_base: the call's numbers of the batch's and the chunk's first profile.
__global__ __launch_bounds__(256) void hs_pcmp_filter_kernel(const uint4* __restrict__ xq,
                                                             const hs_pcmp_par* __restrict__ xpar,
                                                             const double* __restrict__ t, uint32_t x_base, uint32_t mb,
                                                             const uint4* __restrict__ yq,
                                                             const hs_pcmp_par* __restrict__ ypar, uint32_t y_base,
                                                             uint32_t nyc, uint32_t k, uint32_t alphabet, uint32_t v,
                                                             int self, uint32_t* __restrict__ prov_count,
                                                             uint32_t prov_cap, uint2* __restrict__ prov) {
  extern __shared__ uint4 lds[];
  const hs_pcmp_shape sh = hs_pcmp_shape_of(k, alphabet, v);
  const uint32_t x0 = 32u * blockIdx.y, y0 = 32u * blockIdx.x;
  if (self && x_base + x0 >= y_base + y0 + 31u) return;  // (the whole workgroup: no pair with x < y)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n = lane & 15u, q = lane >> 4;
  const uint32_t xw = sh.xrow / 16u, yw = sh.yrow / 16u, xp = xw + 1u, yp = yw + 1u;
  uint4* const ldsX = lds;
  uint4* const ldsY = lds + 32u * xp;
  for (uint32_t i = tid; i < 32u * xw; i += 256u) {
    const uint32_t r = i / xw, c = i - r * xw;
    ldsX[r * xp + c] = xq[(size_t)(x0 + r) * xw + c];
  }
  for (uint32_t i = tid; i < 32u * yw; i += 256u) {
    const uint32_t r = i / yw, c = i - r * yw;
    ldsY[r * yp + c] = yq[(size_t)(y0 + r) * yw + c];
  }
  __syncthreads();

  const uint32_t xt = wave & 1u, yt = wave >> 1;
  const uint4* const a_row = ldsX + (16u * xt + n) * xp + q;
  const uint4* const b_row = ldsY + (16u * yt + n) * yp + q;
  const uint32_t s16 = sh.stride / 16u;
  intx4 best = intx4{INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
  for (uint32_t o = 0; o < sh.n_off; ++o) {
    uint32_t s_lo, s_hi;
    hs_pcmp_step_range(k, sh.stride, (int)o - (int)(k - v), &s_lo, &s_hi);
    intx4 acc = intx4{0, 0, 0, 0};
    for (uint32_t s = s_lo; s < s_hi; ++s) {
      const uint4 a = a_row[o * s16 + 4u * s], b = b_row[4u * s];
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(intx4{(int)a.x, (int)a.y, (int)a.z, (int)a.w},
                                                  intx4{(int)b.x, (int)b.y, (int)b.z, (int)b.w}, acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) best[i] = acc[i] > best[i] ? acc[i] : best[i];
  }

  // register i of lane (n, q): X profile x0 + 16 xt + 4 q + i of the batch against Y profile y0 + 16 yt + n of the chunk
  const uint32_t yl = y0 + 16u * yt + n, y = y_base + yl;
  const bool y_ok = yl < nyc;
  const hs_pcmp_par py = y_ok ? ypar[yl] : hs_pcmp_par{0.0, 0.0, 0.0};
  const uint32_t xl0 = x0 + 16u * xt + 4u * q;
  bool pass[4];
  bool any = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t xl = xl0 + (uint32_t)i;
    pass[i] = false;
    if (y_ok && xl < mb && !(self && x_base + xl >= y)) {
      const hs_pcmp_par px = xpar[xl];
      pass[i] = hs_pcmp_pass((int64_t)best[i], px.s, px.l1, px.amax, py.s, py.l1, k * alphabet, t[xl]) != 0;
    }
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
        if (at < prov_cap) prov[at] = make_uint2(xl0 + (uint32_t)i, y);
      }
      base += (uint32_t)__popcll(bal[i]);
    }
  }
}

// ------------------------------------------------------------------------------------ the exact pass
// X, t: the BATCH's profiles (profile 0 = number x_base of the call); Y: the call's (self mode: the call's X).
// all_pairs == 0: the survivor list; else every pair of the batch, and every hit is counted into the survivor counter
// as well (the host sizes the hit lists from it).
__global__ __launch_bounds__(64) void hs_pcmp_exact_kernel(const double* __restrict__ X, const double* __restrict__ Y,
                                                           const double* __restrict__ t, uint32_t k, uint32_t alphabet,
                                                           uint32_t v, uint32_t x_base, uint32_t mb, uint32_t ny,
                                                           int self, const uint2* __restrict__ prov,
                                                           uint32_t* __restrict__ counters, uint32_t prov_cap,
                                                           int all_pairs, uint32_t hit_cap,
                                                           uint64_t* __restrict__ hit_key,
                                                           uint64_t* __restrict__ hit_val) {
  extern __shared__ double prof[];  // the pair's X profile, then its Y profile
  const uint32_t n = k * alphabet, lane = threadIdx.x, n_off = 2u * (k - v) + 1u;
  double* const px = prof;
  double* const py = prof + n;
  const uint64_t total = all_pairs ? (uint64_t)mb * ny : (uint64_t)min(counters[0], prov_cap);
  for (uint64_t e = blockIdx.x; e < total; e += gridDim.x) {
    uint32_t xl, y;
    if (all_pairs) {
      xl = (uint32_t)(e / ny);
      y = (uint32_t)(e - (uint64_t)xl * ny);
      if (self && x_base + xl >= y) continue;  // (the whole wave)
    } else {
      xl = prov[e].x;
      y = prov[e].y;
    }
    __syncthreads();
    for (uint32_t i = lane; i < n; i += 64u) {
      px[i] = X[(size_t)xl * n + i];
      py[i] = Y[(size_t)y * n + i];
    }
    __syncthreads();
    double best = -INFINITY;
    int bd = 0;
    uint32_t brank = 0xffffffffu;
    for (uint32_t o = lane; o < n_off; o += 64u) {
      const int d = (int)o - (int)(k - v);
      const double sc = hs_pcmp_score(px, py, k, alphabet, d);
      const uint32_t rank = hs_pcmp_rank(d);
      if (sc > best || (sc == best && rank < brank)) {
        best = sc;
        bd = d;
        brank = rank;
      }
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
      const double os = __shfl_xor(best, w);
      const int od = __shfl_xor(bd, w);
      const uint32_t orank = (uint32_t)__shfl_xor((int)brank, w);
      if (os > best || (os == best && orank < brank)) {
        best = os;
        bd = od;
        brank = orank;
      }
    }
    if (lane == 0 && best >= t[xl]) {
      if (all_pairs) (void)hs_reserve_survivors(counters, 1u);
      const uint32_t idx = atomicAdd(counters + 1, 1u);
      if (idx < hit_cap) {
        hit_key[idx] = ((uint64_t)(x_base + xl) << 35) | ((uint64_t)y << 8) | (uint64_t)(uint32_t)(bd + 128);
        hit_val[idx] = (uint64_t)__double_as_longlong(best);
      }
    }
  }
}

// a batch's hits into the caller's arrays (write != 0) and into the per-profile counts (cnt may be null)
__global__ __launch_bounds__(256) void hs_pcmp_emit_kernel(const uint64_t* __restrict__ key,
                                                           const uint64_t* __restrict__ val, uint32_t nh, int write,
                                                           uint32_t* __restrict__ out_x, uint32_t* __restrict__ out_y,
                                                           int32_t* __restrict__ out_d, double* __restrict__ out_score,
                                                           unsigned long long* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nh) return;
  const uint64_t kk = key[i];
  if (cnt) atomicAdd(cnt + (kk >> 35), 1ull);
  if (write) {
    out_x[i] = (uint32_t)(kk >> 35);
    out_y[i] = (uint32_t)(kk >> 8) & 0x7ffffffu;
    out_d[i] = (int32_t)(kk & 0xffu) - 128;
    out_score[i] = __longlong_as_double((long long)val[i]);
  }
}

}  // namespace

hipError_t hs_launch_pcmp_tables(const double* d_P, uint32_t np, uint32_t k, uint32_t alphabet, uint32_t stride,
                                 uint32_t lead, uint32_t row, void* d_rows, void* d_par, hipStream_t s) {
  if (!np) return hipSuccess;
  const uint32_t np_pad = (np + 31u) & ~31u;
  hs_pcmp_tables_kernel<<<np_pad / 4u, 256, 0, s>>>(d_P, np, np_pad, k, alphabet, stride, lead, row, (uint32_t*)d_rows,
                                                    (hs_pcmp_par*)d_par);
  return hipGetLastError();
}

size_t hs_pcmp_filter_lds(uint32_t k, uint32_t alphabet, uint32_t v) {
  const hs_pcmp_shape sh = hs_pcmp_shape_of(k, alphabet, v);
  return 32u * ((size_t)sh.xrow + 16u) + 32u * ((size_t)sh.yrow + 16u);
}

hipError_t hs_launch_pcmp_filter(const void* d_xq, const void* d_xpar, const double* d_t, uint32_t x_base, uint32_t mb,
                                 const void* d_yq, const void* d_ypar, uint32_t y_base, uint32_t nyc, uint32_t k,
                                 uint32_t alphabet, uint32_t v, bool self, uint32_t* d_prov_count, uint32_t prov_cap,
                                 uint2* d_prov, hipStream_t s) {
  if (!mb || !nyc) return hipSuccess;
  const size_t shmem = hs_pcmp_filter_lds(k, alphabet, v);
  {  // more than the 64 KB a kernel may take without asking
    static int granted = 0;  // largest size asked for so far (one value per process is enough: it only grows)
    if (shmem > 65536u && (int)shmem > granted) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(hs_pcmp_filter_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
      if (e != hipSuccess) return e;
      granted = (int)shmem;
    }
  }
  const dim3 grid((nyc + 31u) / 32u, (mb + 31u) / 32u);
  hs_pcmp_filter_kernel<<<grid, 256, shmem, s>>>((const uint4*)d_xq, (const hs_pcmp_par*)d_xpar, d_t, x_base, mb,
                                                 (const uint4*)d_yq, (const hs_pcmp_par*)d_ypar, y_base, nyc, k,
                                                 alphabet, v, self ? 1 : 0, d_prov_count, prov_cap, d_prov);
  return hipGetLastError();
}

hipError_t hs_launch_pcmp_exact(const double* d_X, const double* d_Y, const double* d_t, uint32_t k, uint32_t alphabet,
                                uint32_t v, uint32_t x_base, uint32_t mb, uint32_t ny, bool self, const uint2* d_prov,
                                uint32_t* d_counters, uint32_t prov_cap, bool all_pairs, uint32_t hit_cap,
                                uint64_t* d_hit_key, uint64_t* d_hit_val, int n_cu, hipStream_t s) {
  if (!mb || !ny) return hipSuccess;
  const size_t shmem = (size_t)2 * k * alphabet * 8;  // at most 2 * 75 * 32 * 8 = 38400 bytes
  hs_pcmp_exact_kernel<<<n_cu * 32, 64, shmem, s>>>(d_X, d_Y, d_t, k, alphabet, v, x_base, mb, ny, self ? 1 : 0, d_prov,
                                                    d_counters, prov_cap, all_pairs ? 1 : 0, hit_cap, d_hit_key,
                                                    d_hit_val);
  return hipGetLastError();
}

hipError_t hs_launch_pcmp_emit(const uint64_t* d_key, const uint64_t* d_val, uint32_t nh, bool write, uint32_t* d_out_x,
                               uint32_t* d_out_y, int32_t* d_out_d, double* d_out_score, uint64_t* d_cnt,
                               hipStream_t s) {
  if (!nh || (!write && !d_cnt)) return hipSuccess;
  hs_pcmp_emit_kernel<<<blocks_for(nh), 256, 0, s>>>(d_key, d_val, nh, write ? 1 : 0, d_out_x, d_out_y, d_out_d,
                                                     d_out_score, (unsigned long long*)d_cnt);
  return hipGetLastError();
}
