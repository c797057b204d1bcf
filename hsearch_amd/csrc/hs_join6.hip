// hs_join6.hip -- the bucket-join filter for queries that are k-mers (k = 21..25, 4-column rows) on FP6 MFMA:
// v_mfma_f32_16x16x128_f8f6f4 with e2m3 operands does the whole depth-128 row of a 16 x 16 tile in ONE
// instruction where hs_join8x_kernel issues two v_mfma_i32_16x16x64_i8.
//
// The bound and its exactness: hs_join6_tables.h.  Here: the row layouts and the kernels.
//
// K layout (128 six-bit elements = 4 lane quarters x 32 elements = 4 x 24 bytes).  The operand of lane
// (n = lane & 15, q = lane >> 4) is row / column n, elements 32 q .. 32 q + 31, element i at bit 6 i of the
// lane's 192 bits (hs_join6_selftest checks this map and the accumulation with exact data).  Element 4 p + j =
// coordinate j of position p: quarter q < 3 holds positions 8 q .. 8 q + 7, quarter 3 position 24 and 28 spare
// slots.  Slots 0..16 of those carry -(rho - rho0): on the member side digits (hs_j6_record: 15 coarse, one
// medium, one fine), on the query side the constant factors 7.5 / 0.5 / 0.125; slots 17..27 are zero.
//
// Member side: quarters 0..2 are built per work item from the packed k-mer through a pair table in LDS
// (entry r1 << 5 | r0 = the 48 bits of two residues: four lookups per member and lane), quarter 3 IS the
// member's 16-byte record (t_rec6, built on the first batch that can use it) + 8 zero bytes.
//
// Query side: a row of 128 bytes = 8 pieces of 16: piece q = dwords 0..3 of quarter q; piece 4 + q = dwords 4, 5
// of quarter q, then the float C = -(gamma + rho0) twice.  The rows are gathered into segment order by
// hs_gather_c6t_kernel, a full tile of 32 rows in the kernel's lane order (hs_j6_tile_offset, hs_join6_tables.h):
// a lane's two pieces of a column tile are two loads at 16 lane + a constant, they land in consecutive registers
// that ARE the MFMA's B operand (the instruction reads the first 6; C rides in the seventh), and nothing is
// computed or copied for them.  C stays OUT of the product: the MFMA's C operand is the constant
// 0, the accumulator's column is the lane's query, and the filter passes a pair iff accumulator >= -C.
// Encoding and range of C: a multiple of 2^-6, |C| <= 2^17 (values beyond are clamped to +-2^17, which changes
// nothing: the other terms stay below 2^13, so such a query passes or fails every member either way; a NaN
// radius gives -2^17).  The accumulators are multiples of 2^-6 below 2^13: exact in fp32, and so is the compare.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "hs_internal.h"
#include "hs_join6_tables.h"

namespace {

typedef int intx3 __attribute__((ext_vector_type(3)));
typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx6 __attribute__((ext_vector_type(6)));
typedef int intx8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr uint32_t JRES = 256;   // survivor slots a wave reserves per counter access (as hs_join8.hip)
constexpr int PIECES = HS_J6_ROW_BYTES / 16;  // 16-byte pieces of a query row

__device__ __forceinline__ void close_reservation(uint2* __restrict__ prov, uint32_t res_base, uint32_t res_used,
                                                  uint32_t prov_cap, int lane) {
  for (uint32_t i = res_used + (uint32_t)lane; i < JRES; i += 64u)
    if (res_base + i < prov_cap) prov[res_base + i] = make_uint2(0xffffffffu, 0u);
}

__device__ __forceinline__ uint4 uniform4(const uint4 v) {
  return make_uint4(__builtin_amdgcn_readfirstlane(v.x), __builtin_amdgcn_readfirstlane(v.y),
                    __builtin_amdgcn_readfirstlane(v.z), __builtin_amdgcn_readfirstlane(v.w));
}

// The tile product of the kernel and of its self-test: D = A (16 x 128, e2m3) x B (128 x 16, e2m3) + C.
// SCALE = 0 in both block-scale operands selects the unscaled v_mfma_f32_16x16x128_f8f6f4 (one instruction).
// (the operands are 6 dwords; the kernel's B comes in the registers it was loaded into, C behind it unread)
template <int SCALE = 0>
__device__ __forceinline__ floatx4 tile_mfma6(const intx6 a, const intx8 b8, const floatx4 c) {
  const intx8 a8 = __builtin_shufflevector(a, a, 0, 1, 2, 3, 4, 5, -1, -1);
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, 2, 2, 0, SCALE, 0, SCALE);
}

// ------------------------------------------------------------------------------------ tables
__global__ void hs_jtables6_kernel(const double* __restrict__ coords, int alphabet, hs_j6_dev* __restrict__ T) {
  if (threadIdx.x == 0 && blockIdx.x == 0) hs_j6_compute(coords, alphabet, T, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------ member records
__global__ __launch_bounds__(256) void hs_gather_rec6_kernel(const uint4* __restrict__ packed_all,
                                                             const uint32_t* __restrict__ ids, uint32_t n, int k,
                                                             const hs_j6_dev* __restrict__ T,
                                                             uint4* __restrict__ out_rec) {
  __shared__ double sR[32];
  __shared__ uint32_t sBits[32];
  if (threadIdx.x < 32) {
    sR[threadIdx.x] = T->r[threadIdx.x];
    sBits[threadIdx.x] = T->bits[threadIdx.x];
  }
  __syncthreads();
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const uint4 pk = packed_all[ids[t]];  // (k <= 25: one packed word)
  const uint32_t w[4] = {pk.x, pk.y, pk.z, pk.w};
  double rho = 0.0;
  uint32_t pos24 = 0;
#pragma unroll
  for (int p = 0; p < 25; ++p) {
    const int bit = 5 * p, wi = bit >> 5, sh = bit & 31;
    uint32_t c = w[wi] >> sh;
    if (sh > 27) c |= w[wi + 1] << (32 - sh);
    c &= 31u;
    if (p < k) {
      rho += sR[c];
      if (p == 24) pos24 = sBits[c];
    }
  }
  uint32_t rec[4];
  hs_j6_record(rho, k, T->rpos64, pos24, rec, nullptr);
  out_rec[t] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
}

// ------------------------------------------------------------------------------------ query rows
// One thread per query: the 96 bytes of codes (quarter 3 with the constant factors of the rho slots) and C.
__global__ __launch_bounds__(256) void hs_qprep6_codes_kernel(const uint8_t* __restrict__ qcodes, uint32_t nq, int k,
                                                              double r2_call, const hs_j6_dev* __restrict__ T,
                                                              uint32_t* __restrict__ out,
                                                              const double* __restrict__ radii) {
  __shared__ double sR[32];
  __shared__ uint32_t sBits[32];
  if (threadIdx.x < 32) {
    sR[threadIdx.x] = T->r[threadIdx.x];
    sBits[threadIdx.x] = T->bits[threadIdx.x];
  }
  __syncthreads();
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const double r2 = hs_r2_of(radii, q, r2_call);
  const uint8_t* code = qcodes + (uint64_t)q * k;
  uint32_t W[4][6];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int i = 0; i < 6; ++i) W[a][i] = 0u;
  hs_j6_query_consts(W[3]);
  double sum_r = 0.0;
#pragma unroll
  for (int p = 0; p < 25; ++p) {
    if (p < k) {
      const uint32_t c = code[p] & 31u;
      sum_r += sR[c];
      const uint32_t b = sBits[c];
      const int qu = p >> 3, bit = 24 * (p & 7), wi = bit >> 5, sh = bit & 31;
      W[qu][wi] |= b << sh;
      if (sh > 8) W[qu][wi + 1] |= b >> (32 - sh);
    }
  }
  int64_t c64 = hs_j6_query_c64(sum_r, T->s2_half, r2, k, T->rpos64);
  c64 = c64 > HS_J6_CMAX ? HS_J6_CMAX : c64 < -HS_J6_CMAX ? -HS_J6_CMAX : c64;
  if (!(r2 == r2)) c64 = -HS_J6_CMAX;  // (a NaN radius: no hit)
  const uint32_t cbits = __float_as_uint((float)c64 * (1.0f / 64.0f));
  uint4* row = reinterpret_cast<uint4*>(out) + (uint64_t)q * PIECES;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    row[a] = make_uint4(W[a][0], W[a][1], W[a][2], W[a][3]);
    row[4 + a] = make_uint4(W[a][4], W[a][5], cbits, cbits);
  }
}

// The rows into segment order, tile by tile in the layout of hs_j6_tile_offset.  EIGHT lanes per probe, one per
// piece (hs_gather_c8t_kernel says why): a load of the wave reads 8 whole rows, and its stores fill 128-byte runs.
__global__ __launch_bounds__(256) void hs_gather_c6t_kernel(const uint4* __restrict__ c6,
                                                            const uint32_t* __restrict__ sorted_ql,
                                                            const uint32_t* __restrict__ seg_qoff,
                                                            const uint32_t* __restrict__ seg_of, uint32_t nql, int L,
                                                            char* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  const uint32_t p = t >> 3, g = t & 7u;
  if (p >= nql) return;
  const uint32_t lo = seg_of[p];
  const uint32_t qoff = seg_qoff[lo], nQ = seg_qoff[lo + 1] - qoff;
  const uint32_t local = p - qoff, tile = local >> 5, j = local & 31u;
  const uint32_t nr = min(32u, nQ - (tile << 5));
  const uint32_t q = sorted_ql[p] / (uint32_t)L;
  char* dst = out + (uint64_t)(qoff + (tile << 5)) * HS_J6_ROW_BYTES + hs_j6_tile_offset(nr, j, g);
  *reinterpret_cast<uint4*>(dst) = c6[(uint64_t)q * PIECES + g];
}

// ------------------------------------------------------------------------------------ join
// Query tile of nr rows at segment-order row row0 (hs_j6_tile_offset): lane (n, q) takes the pieces q and 4 + q
// of row 16 c + n for column tile c, 7 dwords that ARE the B operand with C behind it.  Four loads at the tile's
// (scalar) base + 16 lane + 1024 (2 c + h): no address is computed per load.  What shapes the code:
//   - The piece's last dword is not loaded.  A register nothing reads is handed to the sign test as scratch while
//     its load is still in flight, and the wave then waits for every load at the top of the next tile.
//   - The full-tile loads are issued for EVERY tile, and the ragged last tile of a segment (wave-uniform branch)
//     loads its rows over them: rows past the end repeat the last one (masked when survivors are written).  The
//     4 KB read at a ragged tile stay inside the rows' buffer (hs_capi.hip reserves 64 rows more than there are).
//     As an if / else the two forms leave the compiler a path with neither load, the waits of the loop are then
//     counted as if this tile's loads could be the newest, and every third tile waits for all loads in flight.
__device__ __forceinline__ void load_btile6(intx8 (&B)[2], const char* __restrict__ c6t, uint32_t row0, uint32_t nr,
                                            int lane) {
  const char* t0 = c6t + (uint64_t)row0 * HS_J6_ROW_BYTES;
  const char* base = t0 + 16 * lane;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const intx4 hi = *reinterpret_cast<const intx4*>(base + 2048 * c);
    const intx3 lo = *reinterpret_cast<const intx3*>(base + 2048 * c + 1024);
    B[c] = intx8{hi.x, hi.y, hi.z, hi.w, lo.x, lo.y, lo.z, 0};
  }
  if (__builtin_expect(nr != 32u, 0)) {
    const uint32_t n = (uint32_t)lane & 15u, q = (uint32_t)lane >> 4;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint32_t row = min(16u * (uint32_t)c + n, nr - 1u);
      const intx4 hi = *reinterpret_cast<const intx4*>(t0 + hs_j6_tile_offset(nr, row, q));
      const intx3 lo = *reinterpret_cast<const intx3*>(t0 + hs_j6_tile_offset(nr, row, 4u + q));
      B[c] = intx8{hi.x, hi.y, hi.z, hi.w, lo.x, lo.y, lo.z, 0};
    }
  }
}

// One step of the test of a group's 32 accumulators against their queries' thresholds.  The 16 accumulators a
// lane holds of column tile c belong to ONE query, so their maximum, on a tree of three-input maxima (8 steps per
// column tile, the result in w[8 c + 7]), is compared with -C once: no pair of the group passed iff both fail.
__device__ __forceinline__ float max3f(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
__device__ __forceinline__ void sign_step6(int g, const floatx4 (&acc)[4][2], float (&w)[16]) {
  const int c = g >> 3, s = g & 7, o = 8 * c;
  auto v = [&](int i) { return acc[i >> 2][c][i & 3]; };
  if (s < 5) w[g] = max3f(v(3 * s), v(3 * s + 1), v(3 * s + 2));
  else if (s == 5) w[g] = max3f(w[o], w[o + 1], w[o + 2]);
  else if (s == 6) w[g] = max3f(w[o + 3], w[o + 4], v(15));
  else w[g] = max3f(w[o + 5], w[o + 6], v(15));  // (v(15) a second time: a two-input maximum of values the
                                                 // compiler cannot trace costs two more instructions here)
  asm volatile("" : "+v"(w[g]));
}
// The wave's ballots of the two column tiles' maxima against their thresholds: no pair of the group passed iff
// both are zero.
__device__ __forceinline__ void group_pass6(const float (&w)[16], const float (&C)[2], uint64_t (&pass)[2]) {
  pass[0] = __builtin_amdgcn_ballot_w64(w[7] >= -C[0]);
  pass[1] = __builtin_amdgcn_ballot_w64(w[15] >= -C[1]);
}

// Survivors of one group (row tiles T0 .. T0 + 3) against the 32 queries at segment-relative offset qc.  A few
// per cent of the phases come here, nearly all of them for ONE pair, so the path looks before it computes:
//   - only a column tile whose maximum passed (colpass[c], wave-uniform) is looked at;
//   - one compare per accumulator register, written to a scalar pair, is the wave's ballot for that register,
//     and a register without a survivor costs that compare and a scalar branch;
//   - per-lane masks and indices are formed for the registers that have one, and the list is written by one
//     loop per column tile (bit 4 t + i of the mask = row 16 t + 4 q + i of the group).
__device__ __forceinline__ void emit_survivors6(const floatx4 (&acc)[4][2], int T0, uint32_t qc, uint32_t qoff,
                                                uint32_t q_end, uint32_t wbase, uint32_t M, uint32_t mstart,
                                                const float (&C)[2], const uint64_t (&colpass)[2], int lane,
                                                uint32_t& res_base, uint32_t& res_used,
                                                uint32_t* __restrict__ prov_count, uint32_t prov_cap,
                                                uint2* __restrict__ prov) {
  const uint32_t n = (uint32_t)lane & 15u, q = (uint32_t)lane >> 4;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    if (!colpass[c]) continue;
    const float thr = -C[c];
    uint32_t mask = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool hit = acc[t][c][i] >= thr;
        if (__builtin_amdgcn_ballot_w64(hit)) {
          asm volatile("" : "+v"(mask));  // (keeps the branch: the compiler would else compute every mask bit)
          mask |= (hit ? 1u : 0u) << (4 * t + i);
        }
      }
    const uint32_t col = qc + 16u * (uint32_t)c + n;
    if (!(col < q_end)) mask = 0u;
    const uint32_t ql = HS_PROV_INDIRECT | (qoff + col);
    const uint32_t row0 = wbase + (uint32_t)(16 * T0) + 4u * q;
    while (__ballot(mask != 0)) {
      uint32_t idx = 0;
      bool pass = false;
      if (mask) {
        const uint32_t r = (uint32_t)__ffs((int)mask) - 1u;
        mask &= mask - 1;
        idx = row0 + ((r & 12u) << 2) + (r & 3u);
        pass = idx < M;
      }
      const unsigned long long m = __ballot(pass);
      if (m) {
        const uint32_t cnt = (uint32_t)__popcll(m);
        if (res_used + cnt > JRES) {
          close_reservation(prov, res_base, res_used, prov_cap, lane);
          uint32_t base = 0;
          if (lane == 0) base = hs_reserve_survivors(prov_count, (uint32_t)JRES);
          res_base = __builtin_amdgcn_readfirstlane(base);
          res_used = 0;
        }
        if (pass) {
          const uint32_t o = res_base + res_used + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          if (o < prov_cap) prov[o] = make_uint2(ql, mstart + idx);
        }
        res_used += cnt;
      }
    }
  }
}

// The structure of hs_join8x_kernel: work items owned by one wave, chunks of items from a global counter or from
// per-XCD runs, NB query tiles in flight, the same survivor list.  A phase is 8 MFMAs -- 4 row tiles x 2 column
// tiles -- with two steps of the sign test of the phase before it behind each; a query tile is RT / 4 phases.
// Two instantiations (HS_OPT_JOIN_F6_FORM):
//   hs_join6x_kernel = <8, 3, true>    items of 128 members, three tiles in flight, the next item's members
//                                      prefetched into registers
//   hs_join6w_kernel = <12, 2, false>  items of HS_J6_WIDE_ITEM = 192 members: the 4 KB of a query tile feed 24 MFMAs
//                                      where they feed 16 above -- two thirds of the query bytes a CU pulls per MFMA,
//                                      and the per-tile instructions that are no test spread over half as many MFMAs
//                                      again.  What differs:
//   - An item whose members fill at most 8 row tiles (a bucket's last item, a small bucket) runs the 8-tile body, a
//     wave-uniform choice per item.
//   - The members of the NEXT item are not prefetched (the registers hold four more row tiles' operands): an item
//     loads its members when it starts, behind the first query tiles already in flight.  (Copied into LDS an item
//     ahead instead -- global_load_lds_dwordx4, no register on the way -- the kernel ran 4 % SLOWER: loads return
//     in order, so the next query tiles wait behind twelve copies that miss every cache.)
//   - Two query tiles in flight, not three: a group of tiles must be an even number of phases (below); with four
//     the compiler spills, and the kernel ran 25 % slower.
template <int RT_MAX, int NB, bool PREFETCH>
__device__ __forceinline__ void join6_items(
    const uint4* __restrict__ desc, uint32_t n_items, const uint4* __restrict__ packed_base,
    const uint4* __restrict__ rec_base, const char* __restrict__ c6t, const hs_j6_dev* __restrict__ T,
    uint32_t* __restrict__ prov_count, uint32_t prov_cap, uint2* __restrict__ prov,
    uint32_t* __restrict__ item_counter, uint32_t G, const uint32_t* __restrict__ n_items_dev, uint32_t xcd_run) {
  if (n_items_dev) n_items = min(n_items, __builtin_amdgcn_readfirstlane(*n_items_dev));
  __shared__ uint2 sPair[1024];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, q = lane >> 4;
  for (int e = tid; e < 1024; e += 256) sPair[e] = T->pair[e];
  __syncthreads();  // the only one: the table is read-only from here on
  // (the dealing of chunks: as hs_join8x_kernel, where it is explained)
  const uint32_t xcd_sh = 31u - (uint32_t)__builtin_clz(xcd_run | 1u), xcd_mask = (1u << xcd_sh) - 1u;
  uint32_t victim = __builtin_amdgcn_s_getreg(6164) & 7u;  // hwreg(HW_REG_XCC_ID, 0, 4)
  uint32_t tried = 0;
  const uint32_t first_dynamic = gridDim.x * 4u * G;
  auto chunk_item = [&](uint32_t v) -> uint32_t {
    if (!xcd_run) return first_dynamic + v;
    for (;;) {
      const uint32_t c = ((((v >> xcd_sh) << 3) + victim) << xcd_sh) + (v & xcd_mask);
      const uint64_t it = (uint64_t)c * G;
      if (it < (uint64_t)n_items) return (uint32_t)it;
      if (++tried == 8u) return 0xf0000000u;
      victim = (victim + 1u) & 7u;
      uint32_t j = 0;
      if (lane == 0) j = atomicAdd(item_counter + 8 + victim, 1u);
      v = __builtin_amdgcn_readfirstlane(j);
    }
  };
#define HS_TAKE_CHUNK() (xcd_run ? atomicAdd(item_counter + 8 + victim, 1u) : atomicAdd(item_counter, G))
  uint32_t item = (blockIdx.x * 4u + (uint32_t)wave) * G;
  if (xcd_run) {
    uint32_t first = 0;
    if (lane == 0) first = HS_TAKE_CHUNK();
    item = chunk_item(__builtin_amdgcn_readfirstlane(first));
  }
  if (item >= n_items) return;
  uint32_t res_base = 0, res_used = JRES;
  uint32_t next_chunk_v = 0;
  if (lane == 0) next_chunk_v = HS_TAKE_CHUNK();
  uint32_t pf_item = item, pf_chunk_end = min(item + G, n_items);
#define HS_ADVANCE_PF()                                                                  \
  {                                                                                      \
    ++pf_item;                                                                           \
    if (pf_item == pf_chunk_end) {                                                       \
      pf_item = chunk_item(__builtin_amdgcn_readfirstlane(next_chunk_v));                \
      pf_chunk_end = pf_item < n_items ? min(pf_item + G, n_items) : pf_item + G;        \
      if (lane == 0 && pf_item < n_items) next_chunk_v = HS_TAKE_CHUNK();                \
    }                                                                                    \
  }
  uint4 d0 = uniform4(desc[2 * (uint64_t)item]), d1 = uniform4(desc[2 * (uint64_t)item + 1]);
  HS_ADVANCE_PF()
  uint32_t next_item = pf_item;
  uint4 nd0 = d0, nd1 = d1;
  if (next_item < n_items) {
    nd0 = uniform4(desc[2 * (uint64_t)next_item]);
    nd1 = uniform4(desc[2 * (uint64_t)next_item + 1]);
  }
  static_assert(RT_MAX == 8 || (RT_MAX == 12 && NB % 2 == 0),
                "a group must be an even number of phases, for 2 and for 3 phases per tile");
  constexpr uint32_t JM = 16 * RT_MAX;  // members per work item
  // PREFETCH: lanes of quarters 0..2: packed member 16 t + n of the NEXT item; quarter 3: its record
  uint4 mk_next[PREFETCH ? RT_MAX : 1];
  auto load_members = [&](uint4* mk, int rt, const uint4& D0) {
    const int64_t off = (int64_t)(((uint64_t)D0.y << 32) | (uint64_t)D0.x);
    const uint4* src = (q == 3 ? rec_base : packed_base) + off;
    const uint32_t idx = D0.w * JM + (uint32_t)n;
#pragma unroll
    for (int t = 0; t < RT_MAX; ++t)
      if (t < rt) mk[t] = src[min(idx + 16 * t, D0.z - 1)];
  };
  if (PREFETCH) load_members(mk_next, RT_MAX, d0);
  constexpr uint32_t GQ = 32 * NB;
  intx8 Bq[NB][2];
  const uint32_t skew = ((blockIdx.x * 4u + (uint32_t)wave) * 40503u) & 0xffffu;
#define HS_N_GROUPS(D1) (((D1).z - (D1).y + GQ - 1u) / GQ)
#define HS_FIRST_Q(D1) ((D1).y + GQ * ((skew * HS_N_GROUPS(D1)) >> 16))
  {
    const uint32_t q0 = HS_FIRST_Q(d1);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const uint32_t qu = q0 + 32u * u < d1.z ? q0 + 32u * u : q0;
      load_btile6(Bq[u], c6t, d1.x + qu, min(32u, d1.z - qu), lane);
    }
  }
  // bits 40 q .. 40 q + 39 of the packed word = positions 8 q .. 8 q + 7 of quarter q < 3: dwords (q, q + 1)
  // shifted down by 8 q (quarter 3 computes on its record and discards the result)
  const uint32_t bs = 8u * (uint32_t)min(q, 2);
  while (true) {
    const uint32_t M = d0.z, mt = d0.w;
    const uint32_t qoff = d1.x, q_begin = d1.y, q_end = d1.z, mstart = d1.w;
    const uint32_t wbase = mt * JM;
    const bool has_next = next_item < n_items;
    HS_ADVANCE_PF()  // pf_item = the item after next
    uint4 nnd0 = nd0, nnd1 = nd1;
    if (pf_item < n_items) {
      nnd0 = uniform4(desc[2 * (uint64_t)pf_item]);
      nnd1 = uniform4(desc[2 * (uint64_t)pf_item + 1]);
    }
    auto run_item = [&](auto rt_tag) {
      constexpr int RT = decltype(rt_tag)::value, PH = RT / 4;  // row tiles of 16 members; phases per query tile
      // ---- the item's members (lanes of quarters 0..2: packed member 16 t + n; quarter 3: its record) and
      // their A operands
      intx6 A[RT];
      {
        uint4 mk_here[PREFETCH ? 1 : RT];
        if (!PREFETCH) load_members(mk_here, RT, d0);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          const uint4 m = PREFETCH ? mk_next[t] : mk_here[t];
          const uint32_t a = q == 0 ? m.x : q == 1 ? m.y : m.z, b = q == 0 ? m.y : q == 1 ? m.z : m.w;
          const uint32_t lo = __funnelshift_r(a, b, bs), hi = b >> bs;
          const uint2 e0 = sPair[lo & 1023u], e1 = sPair[(lo >> 10) & 1023u];
          const uint2 e2 = sPair[(lo >> 20) & 1023u], e3 = sPair[__funnelshift_r(lo, hi, 30) & 1023u];
          const intx6 lk = intx6{(int)e0.x, (int)(e0.y | (e1.x << 16)), (int)__funnelshift_r(e1.x, e1.y, 16),
                                 (int)e2.x, (int)(e2.y | (e3.x << 16)), (int)__funnelshift_r(e3.x, e3.y, 16)};
          const intx6 own = intx6{(int)m.x, (int)m.y, (int)m.z, (int)m.w, 0, 0};
          A[t] = q == 3 ? own : lk;
        }
        if (PREFETCH) load_members(mk_next, RT_MAX, nd0);
      }
      // Accumulators: TWO sets of 4 row tiles x 2 column tiles.  A tile is PH = RT / 4 phases; phase p of a group
      // (counted over its tiles) writes set p & 1 from row tiles 4 ph .. 4 ph + 3 and tests the other set -- the
      // phase before it -- in the gaps.  NB PH is even, so a group starts and ends with set 1 pending (written by a
      // tile's last phase, tested in the next tile's first), whichever PH.  Three sets for RT = 12 would cost 32
      // registers more than there are.
      floatx4 acc[2][4][2];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[1][t][c] = __builtin_nondeterministic_value(acc[1][t][c]);
      bool live = false;  // set 1 holds a tile's last phase (not so at the item's first tile)
      float Cp[2] = {0.0f, 0.0f};
      uint32_t prev_qc = q_begin;
      const uint32_t n_groups = HS_N_GROUPS(d1);
      uint32_t qc0 = HS_FIRST_Q(d1);
      auto test_set = [&](const floatx4 (&set)[4][2], const float (&w)[16], int T0, uint32_t qct, const float (&Ct)[2]) {
        uint64_t pp[2];
        group_pass6(w, Ct, pp);
        if (pp[0] | pp[1])
          emit_survivors6(set, T0, qct, qoff, q_end, wbase, M, mstart, Ct, pp, lane, res_base, res_used, prov_count,
                          prov_cap, prov);
      };
      auto do_group = [&](uint32_t gi) {
        uint32_t nrow = qoff, nq0 = qc0 + GQ, nqend = q_end;
        if (nq0 >= q_end) nq0 = q_begin;
        if (gi + 1 == n_groups) {
          nrow = nd1.x;
          nq0 = HS_FIRST_Q(nd1);
          nqend = nd1.z;
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const uint32_t qc = qc0 + 32u * (uint32_t)u;
          intx8 (&B)[2] = Bq[u];
          if (u == 0 || qc < q_end) {
            const floatx4 zero = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
            const float Cx[2] = {__int_as_float(B[0][6]), __int_as_float(B[1][6])};
#pragma unroll
            for (int ph = 0; ph < PH; ++ph) {
              const int ws = (u * PH + ph) & 1, ts = ws ^ 1;
              const bool test = ph > 0 || live;
              float w[16];
#pragma unroll
              for (int g = 0; g < 8; ++g) {
                acc[ws][g >> 1][g & 1] = tile_mfma6(A[4 * ph + (g >> 1)], B[g & 1], zero);
                if (test) {
                  sign_step6(2 * g, acc[ts], w);
                  sign_step6(2 * g + 1, acc[ts], w);
                }
                __builtin_amdgcn_sched_barrier(0);
              }
              if (test) {
                if (ph == 0) test_set(acc[ts], w, 4 * (PH - 1), prev_qc, Cp);
                else test_set(acc[ts], w, 4 * (ph - 1), qc, Cx);
              }
            }
            live = true;
            prev_qc = qc;
            // (the tile's registers are loaded anew below and its last phase is tested a phase later: its C moves
            // out of them here, in so many words -- left to itself the compiler loads every tile elsewhere and
            // copies it)
            asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3"
                         : "=&v"(Cp[0]), "=v"(Cp[1])
                         : "v"(Cx[0]), "v"(Cx[1]));
          } else if (((u * PH - 1) & 1) == 0 && qc - 32u < q_end) {
            // the group's first skipped tile (a segment's ragged last group) and the tile before it left SET 0
            // pending: it moves to set 1, where the next phase expects it (at most once per item's walk)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int c = 0; c < 2; ++c) acc[1][t][c] = acc[0][t][c];
          }
          const uint32_t nb = nq0 + 32u * (uint32_t)u < nqend ? nq0 + 32u * (uint32_t)u : nq0;
          load_btile6(B, c6t, nrow + nb, min(32u, nqend - nb), lane);
        }
        qc0 = nq0;
      };
      do_group(0);
      for (uint32_t gi = 1; gi < n_groups; ++gi) do_group(gi);
      {  // the item's last pending phase
        float w[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) sign_step6(g, acc[1], w);
        test_set(acc[1], w, 4 * (PH - 1), prev_qc, Cp);
      }
    };
    if (RT_MAX > 8 && M - wbase > 128u) run_item(std::integral_constant<int, RT_MAX>{});
    else run_item(std::integral_constant<int, 8>{});
    if (!has_next) break;
    item = next_item;
    next_item = pf_item;
    d0 = nd0;
    d1 = nd1;
    nd0 = nnd0;
    nd1 = nnd1;
  }
#undef HS_ADVANCE_PF
#undef HS_TAKE_CHUNK
#undef HS_N_GROUPS
#undef HS_FIRST_Q
  close_reservation(prov, res_base, res_used, prov_cap, lane);
}

#define HS_JOIN6_PARAMS                                                                                          \
  const uint4 *__restrict__ desc, uint32_t n_items, const uint4 *__restrict__ packed_base,                       \
      const uint4 *__restrict__ rec_base, const char *__restrict__ c6t, const hs_j6_dev *__restrict__ T,         \
      uint32_t *__restrict__ prov_count, uint32_t prov_cap, uint2 *__restrict__ prov,                            \
      uint32_t *__restrict__ item_counter, uint32_t G, const uint32_t *__restrict__ n_items_dev, uint32_t xcd_run
#define HS_JOIN6_ARGS \
  desc, n_items, packed_base, rec_base, c6t, T, prov_count, prov_cap, prov, item_counter, G, n_items_dev, xcd_run
__global__ __launch_bounds__(256, 2) void hs_join6x_kernel(HS_JOIN6_PARAMS) { join6_items<8, 3, true>(HS_JOIN6_ARGS); }
__global__ __launch_bounds__(256, 2) void hs_join6w_kernel(HS_JOIN6_PARAMS) { join6_items<12, 2, false>(HS_JOIN6_ARGS); }
#undef HS_JOIN6_PARAMS
#undef HS_JOIN6_ARGS

// ------------------------------------------------------------------------------------ self-test
// Rows on the e2m3 grid, thresholds on the 2^-6 grid, through tile_mfma6 with the lane map the kernel relies on;
// every accumulator against int64 arithmetic.  One wave per case:
//   0  every element +7.5 on both sides, C = +2^17               (the largest sum, the largest threshold)
//   1  A +7.5, B -7.5, C = -2^17
//   2  A alternating +-7.5 along k, B +7.5, C = 2^17 - 2^-6       (cancellation beside a large threshold)
//   3  A alternating +-7.5 along k and rows, B alternating along k, C = -(2^17 - 2^-6)
//   4+ pseudo-random codes (asymmetric in row, column and k: a wrong lane map cannot pass), C random in +-2^17;
//      odd cases keep position 24 / the slots' shape: elements 117..127 zero
__device__ __forceinline__ uint32_t st_hash(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t st_code(uint32_t cs, uint32_t side, uint32_t row, uint32_t k) {
  const uint32_t MAXP = 31u, MAXN = 63u;  // +7.5, -7.5
  if (cs == 0) return MAXP;
  if (cs == 1) return side ? MAXN : MAXP;
  if (cs == 2) return side ? MAXP : ((k & 1u) ? MAXN : MAXP);
  if (cs == 3) return ((k + (side ? 0u : row)) & 1u) ? MAXN : MAXP;
  if ((cs & 1u) && k >= 117u) return 0u;
  return st_hash(cs * 0x9e3779b9u + side * 0x85ebca6bu + row * 131u + k * 2654435761u) & 63u;
}
__device__ __forceinline__ int32_t st_c64(uint32_t cs, uint32_t col) {
  const int32_t big = 1 << 23;  // 2^17 in 64ths
  if (cs == 0) return big;
  if (cs == 1) return -big;
  if (cs == 2) return big - 1;
  if (cs == 3) return -(big - 1);
  return (int32_t)(st_hash(cs * 977u + col * 0x27d4eb2fu) % (uint32_t)(2 * big + 1)) - big;
}
template <int SCALE>
__global__ __launch_bounds__(64) void hs_join6_selftest_kernel(uint32_t* __restrict__ mismatches,
                                                               uint32_t* __restrict__ first_bad) {
  const uint32_t cs = blockIdx.x, lane = threadIdx.x & 63u, n = lane & 15u, q = lane >> 4;
  uint32_t a[6] = {0, 0, 0, 0, 0, 0}, b[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const uint32_t ca = st_code(cs, 0u, n, 32u * q + (uint32_t)i), cb = st_code(cs, 1u, n, 32u * q + (uint32_t)i);
    const int bit = 6 * i, wi = bit >> 5, sh = bit & 31;
    a[wi] |= ca << sh;
    b[wi] |= cb << sh;
    if (sh > 26) {
      a[wi + 1] |= ca >> (32 - sh);
      b[wi + 1] |= cb >> (32 - sh);
    }
  }
  const float cf = (float)st_c64(cs, n) * (1.0f / 64.0f);
  const floatx4 d = tile_mfma6<SCALE>(intx6{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5]},
                                      intx8{(int)b[0], (int)b[1], (int)b[2], (int)b[3], (int)b[4], (int)b[5],
                                            __float_as_int(cf), __float_as_int(cf)},
                                      floatx4{cf, cf, cf, cf});
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t row = 4u * q + (uint32_t)i;  // result register i of lane (n, q) = row 4 q + i, column n
    long long ref = (long long)st_c64(cs, n);
    for (uint32_t k = 0; k < 128u; ++k)
      ref += (long long)hs_e2m3_eighths(st_code(cs, 0u, row, k)) * (long long)hs_e2m3_eighths(st_code(cs, 1u, n, k));
    const double got = (double)d[i] * 64.0;
    if (!(got == (double)ref)) {
      if (atomicAdd(mismatches, 1u) == 0u) {
        first_bad[0] = cs;
        first_bad[1] = lane * 4u + (uint32_t)i;
        first_bad[2] = __float_as_uint(d[i]);
        first_bad[3] = (uint32_t)(int32_t)ref;
      }
    }
  }
}

inline unsigned blocks_for(uint64_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t hs_launch_jtables6(const double* d_coords, int alphabet, void* d_tab6, hipStream_t s) {
  hs_jtables6_kernel<<<1, 64, 0, s>>>(d_coords, alphabet, (hs_j6_dev*)d_tab6);
  return hipGetLastError();
}

size_t hs_join6_table_bytes() { return sizeof(hs_j6_dev); }
size_t hs_join6_ok_offset() { return offsetof(hs_j6_dev, ok); }
int hs_join6_row_bytes() { return HS_J6_ROW_BYTES; }
uint32_t hs_join6_wide_item() { return HS_J6_WIDE_ITEM; }

hipError_t hs_launch_gather_c6t(const void* d_c6, const uint32_t* d_sorted_ql, const uint32_t* d_seg_qoff,
                                const uint32_t* d_seg_of, uint32_t nql, int L, void* d_out, hipStream_t s) {
  if (!nql) return hipSuccess;
  hs_gather_c6t_kernel<<<blocks_for((uint64_t)nql * PIECES), 256, 0, s>>>((const uint4*)d_c6, d_sorted_ql, d_seg_qoff,
                                                                          d_seg_of, nql, L, (char*)d_out);
  return hipGetLastError();
}

hipError_t hs_launch_gather_rec6(const uint4* d_packed_all, const uint32_t* d_ids_sorted, uint32_t n, int k,
                                 const void* d_tab6, uint4* d_out_rec, hipStream_t s) {
  if (!n) return hipSuccess;
  hs_gather_rec6_kernel<<<blocks_for(n), 256, 0, s>>>(d_packed_all, d_ids_sorted, n, k, (const hs_j6_dev*)d_tab6,
                                                      d_out_rec);
  return hipGetLastError();
}

hipError_t hs_launch_qprep6_codes(const uint8_t* d_qcodes, uint32_t nq, int k, double r2, const void* d_tab6,
                                  void* d_c6, hipStream_t s, const double* d_radii) {
  if (!nq) return hipSuccess;
  hs_qprep6_codes_kernel<<<blocks_for(nq), 256, 0, s>>>(d_qcodes, nq, k, r2, (const hs_j6_dev*)d_tab6,
                                                        (uint32_t*)d_c6, d_radii);
  return hipGetLastError();
}

hipError_t hs_launch_join6x(const uint4* d_desc, uint32_t n_items, const uint4* d_packed_base,
                            const uint4* d_rec_base, const void* d_c6t, const void* d_tab6, uint32_t* d_prov_count,
                            uint32_t prov_cap, uint2* d_prov, uint32_t* d_item_counter, int n_blocks,
                            const uint32_t* d_n_items, uint32_t G, uint32_t xcd_run, hipStream_t s, int wide_items) {
  if (!n_items) return hipSuccess;
  if (wide_items)
    hs_join6w_kernel<<<n_blocks, 256, 0, s>>>(d_desc, n_items, d_packed_base, d_rec_base, (const char*)d_c6t,
                                              (const hs_j6_dev*)d_tab6, d_prov_count, prov_cap, d_prov, d_item_counter,
                                              G, d_n_items, xcd_run);
  else
    hs_join6x_kernel<<<n_blocks, 256, 0, s>>>(d_desc, n_items, d_packed_base, d_rec_base, (const char*)d_c6t,
                                              (const hs_j6_dev*)d_tab6, d_prov_count, prov_cap, d_prov, d_item_counter,
                                              G, d_n_items, xcd_run);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ exported
extern "C" {

// The FP6 filter's tables from a coordinate table ([alphabet][8] doubles), on the host: no GPU needed.
// codes [32][4] six-bit e2m3 codes, e / r [32] doubles, pair [1024][2] dwords (hs_j6_dev::pair); *s the scale.
HS_API hs_status hs_join6_tables(const double* coords, uint32_t alphabet, double* s, uint8_t* codes, double* e,
                                 double* r, uint32_t* pair) {
  if (!coords || alphabet < 1 || alphabet > 32) return HS_ERR_INVALID;
  std::vector<hs_j6_dev> T(1);
  double ee[32], ss = 0.0;
  hs_j6_compute(coords, (int)alphabet, &T[0], ee, &ss);
  if (!T[0].ok) return HS_ERR_INVALID;
  if (s) *s = ss;
  for (int a = 0; a < 32; ++a) {
    if (codes)
      for (int j = 0; j < 4; ++j) codes[a * 4 + j] = (uint8_t)((T[0].bits[a] >> (6 * j)) & 63u);
    if (e) e[a] = ee[a];
    if (r) r[a] = T[0].r[a];
  }
  if (pair) memcpy(pair, T[0].pair, sizeof(T[0].pair));
  return HS_OK;
}

// The thresholds the kernels carry for n k-mers (codes [n][k]) at squared radii r2[n], in units of 2^-6:
// rho64 = what a member's record stands for, c64 = a query's C operand (-(gamma + rho0)), rho0_64 = k * rpos64;
// rec (optional) [n][4] the member records.  The filter value of member x and query c is
// sum_p S[x_p][c_p] - (rho64[x] - rho0_64) / 64 + c64[c] / 64.  Host only.
HS_API hs_status hs_join6_thresholds(const double* coords, uint32_t alphabet, const uint8_t* kmers, uint64_t n,
                                     uint32_t k, const double* r2, int64_t* rho64, int64_t* c64, int64_t* rho0_64,
                                     uint32_t* rec) {
  if (!coords || alphabet < 1 || alphabet > 32 || !kmers || k < 1 || k > 25) return HS_ERR_INVALID;
  std::vector<hs_j6_dev> T(1);
  hs_j6_compute(coords, (int)alphabet, &T[0], nullptr, nullptr);
  if (!T[0].ok) return HS_ERR_INVALID;
  if (rho0_64) *rho0_64 = (int64_t)k * T[0].rpos64;
  for (uint64_t i = 0; i < n; ++i) {
    double sum = 0.0;
    uint32_t pos24 = 0;
    for (uint32_t p = 0; p < k; ++p) {
      const uint32_t c = kmers[i * k + p];
      if (c >= alphabet) return HS_ERR_INVALID;
      sum += T[0].r[c];
      if (p == 24) pos24 = T[0].bits[c];
    }
    uint32_t w[4];
    int64_t enc = 0;
    hs_j6_record(sum, (int)k, T[0].rpos64, pos24, w, &enc);
    if (rho64) rho64[i] = enc;
    if (rec) memcpy(rec + 4 * i, w, 16);
    if (c64) {
      int64_t c = hs_j6_query_c64(sum, T[0].s2_half, r2 ? r2[i] : 0.0, (int)k, T[0].rpos64);
      c64[i] = c > HS_J6_CMAX ? HS_J6_CMAX : c < -HS_J6_CMAX ? -HS_J6_CMAX : c;
    }
  }
  return HS_OK;
}

// The layout the gather writes and the kernel reads (hs_j6_tile_offset), for a test without a GPU
HS_API uint32_t hs_join6_tile_offset(uint32_t nr, uint32_t row, uint32_t piece) {
  if (nr < 1 || nr > 32 || row >= nr || piece >= (uint32_t)PIECES) return 0xffffffffu;
  return hs_j6_tile_offset(nr, row, piece);
}

// GPU: the kernel's tile product against int64 arithmetic on rows at the format's extremes (see the kernel).
// variant 0: the product as hs_join6x_kernel issues it; 1: the same with explicit block scales of 2^0.
// *mismatches = accumulators that differ (0 = exact); first_bad (optional, 4 words): case, lane * 4 + register,
// the float's bits, the expected value in 64ths.
HS_API hs_status hs_join6_selftest(int device, int variant, uint64_t* mismatches, uint32_t* first_bad) {
  if (!mismatches || variant < 0 || variant > 1) return HS_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return HS_ERR_HIP;
  uint32_t* d = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d), 32) != hipSuccess) return HS_ERR_HIP;
  uint32_t host[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipError_t e = hipMemset(d, 0, 32);
  if (e == hipSuccess) {
    constexpr int CASES = 64;
    if (variant == 0) hs_join6_selftest_kernel<0><<<CASES, 64>>>(d, d + 1);
    else hs_join6_selftest_kernel<127><<<CASES, 64>>>(d, d + 1);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(host, d, 32, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return HS_ERR_HIP;
  *mismatches = host[0];
  if (first_bad) memcpy(first_bad, host + 1, 16);
  return HS_OK;
}

}  // extern "C"
