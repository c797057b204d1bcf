// hs_remove.hip -- hs_index_remove: a built index without a set of its k-mers, on the device.
//
// A table is its entries ordered by (fingerprint, id).  Removing entries keeps that order, and the survivors are
// renumbered in their old order, so the table over the remainder is a stream compaction of the bucket-ordered
// arrays plus a compaction of the directory.  Nothing that survives is hashed, sorted or gathered again.
//
// Everything is steered by keep masks: one 64-bit word per 64 positions (bit i = position 64 w + i survives; bits
// at and behind n are 0, and so is one word behind the last), their popcounts, and an exclusive scan of the popcounts
// (one element more than words: the last is the number of survivors).  Then
//     rank(p) = scan[p >> 6] + popcount(mask[p >> 6] & below(p & 63))       (0 <= p <= n)
// is the number of survivors in front of p: the new place of a surviving p, and the difference of two ranks is the
// number of survivors of a range.  The caller (hs_capi.hip, remove_tables) runs:
//   mark        the dead bitmap over ids (64-bit words), from a list of ids (any order, duplicates) or from ranges
//               (may overlap); *flag |= 1 for an id >= n: nothing is written for it
//   masks_ids   id order: mask = ~dead, popcount; <scan>; new_id[i] = rank(i) or 0xffffffff.  codes and packed_all
//               are compacted by new_id
// and per table:
//   masks_tab   table order: one wave per 64 positions, keep = !dead[ids[p]], __ballot, popcount; <scan>
//   dir_flags   one lane per old bucket b: survivors = rank(start[b + 1]) - rank(start[b]); alive = survivors > 0;
//               retuple = alive and the bit at start[b] is clear (the first member went: dir_tuple is the bucket ints
//               of the member with the smallest id, and members share the HashKey string, not always the ints)
//   <scans of alive and retuple: new bucket numbers, and -- in bucket order, so deterministic -- the list of buckets
//    that need a tuple>
//   dir_write   alive b -> bucket scan(alive)[b]: key copied (the fingerprint belongs to the string), count, tuple
//               copied or, for retuple, the OLD id of the new first member (first set bit from start[b] on) and the
//               new bucket number appended to the list at scan(retuple)[b]
//   <the caller gathers the codes of the listed ids, hashes just those with the table's functions; tuples_put
//    writes the K ints to the listed buckets; scan of the counts = dir_start', their maximum = max_bucket>
//   move        lane p with keep writes entry p to rank(p): ids' = new_id[ids[p]], packed (PW 16-byte words), rec8,
//               rho.  Compaction preserves order: a wave's writes are one contiguous run.
// Scratch: 4 n bytes for new_id, n / 8 for the bitmap, 32 bytes per 64 entries for masks, counts and scans (id order
// and one table), and one table's directory.  The shrunken arrays are new allocations which the caller swaps in.
#include "hs_internal.h"

namespace {

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + 255) / 256); }

__device__ __forceinline__ uint64_t below(uint32_t bit) { return ((uint64_t)1 << bit) - 1; }  // bit in 0..63

__device__ __forceinline__ uint32_t rank_of(const uint64_t* __restrict__ mask, const uint32_t* __restrict__ scan,
                                            uint32_t p) {
  return scan[p >> 6] + (uint32_t)__popcll(mask[p >> 6] & below(p & 63));
}

__global__ __launch_bounds__(256) void hs_remove_mark_ids_kernel(const uint32_t* __restrict__ ids, uint64_t m, uint32_t n,
                                                                 unsigned long long* __restrict__ dead,
                                                                 uint32_t* __restrict__ flag) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m) return;
  const uint32_t id = ids[t];
  if (id >= n) {
    atomicOr(flag, 1u);
    return;
  }
  atomicOr(dead + (id >> 6), 1ull << (id & 63));
}

// block (x, y): range y, words of the range dealt to x's threads.  The host has checked first + count <= n.
__global__ __launch_bounds__(256) void hs_remove_mark_ranges_kernel(const uint64_t* __restrict__ first,
                                                                    const uint64_t* __restrict__ count,
                                                                    uint64_t r0, uint64_t n_ranges, uint32_t n,
                                                                    unsigned long long* __restrict__ dead) {
  const uint64_t r = r0 + blockIdx.y;
  if (r >= n_ranges) return;
  const uint64_t lo = first[r], cnt = count[r];
  if (!cnt || lo >= n || cnt > n - lo) return;
  const uint64_t hi = lo + cnt;  // exclusive
  const uint64_t w0 = lo >> 6, w1 = (hi - 1) >> 6;
  for (uint64_t w = w0 + (uint64_t)blockIdx.x * 256 + threadIdx.x; w <= w1; w += (uint64_t)gridDim.x * 256) {
    uint64_t bits = ~(uint64_t)0;
    if (w == w0) bits &= ~below((uint32_t)(lo & 63));
    if (w == w1 && (hi & 63)) bits &= below((uint32_t)(hi & 63));
    atomicOr(dead + w, (unsigned long long)bits);
  }
}

// id order: word w of [0, nw]; the word behind the last is 0
__global__ __launch_bounds__(256) void hs_remove_masks_ids_kernel(const unsigned long long* __restrict__ dead, uint32_t n,
                                                                  uint32_t nw, uint64_t* __restrict__ mask,
                                                                  uint32_t* __restrict__ cnt) {
  const uint32_t w = blockIdx.x * 256 + threadIdx.x;
  if (w > nw) return;
  uint64_t keep = 0;
  if (w < nw) {
    keep = ~(uint64_t)dead[w];
    const uint32_t left = n - w * 64;  // >= 1
    if (left < 64) keep &= below(left);
  }
  mask[w] = keep;
  cnt[w] = (uint32_t)__popcll(keep);
}

__global__ __launch_bounds__(256) void hs_remove_new_id_kernel(const uint64_t* __restrict__ mask,
                                                               const uint32_t* __restrict__ scan, uint32_t n,
                                                               uint32_t* __restrict__ new_id) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool keep = (mask[i >> 6] >> (i & 63)) & 1;
  new_id[i] = keep ? rank_of(mask, scan, i) : 0xffffffffu;
}

// table order: a wave per 64 positions (256 threads = 4 words); the block that holds word nw writes its 0
__global__ __launch_bounds__(256) void hs_remove_masks_tab_kernel(const uint32_t* __restrict__ ids,
                                                                  const unsigned long long* __restrict__ dead,
                                                                  uint32_t n, uint32_t nw, uint64_t* __restrict__ mask,
                                                                  uint32_t* __restrict__ cnt) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  const uint32_t w = p >> 6;  // the same in every lane of a wave
  if (w > nw) return;
  bool keep = false;
  if (p < n) {
    const uint32_t id = ids[p];
    keep = id < n && !((dead[id >> 6] >> (id & 63)) & 1);
  }
  const uint64_t b = __ballot(keep);
  if ((p & 63) == 0) {
    mask[w] = b;
    cnt[w] = (uint32_t)__popcll(b);
  }
}

__global__ __launch_bounds__(256) void hs_remove_dir_flags_kernel(const uint32_t* __restrict__ dir_start, uint32_t nb,
                                                                  const uint64_t* __restrict__ mask,
                                                                  const uint32_t* __restrict__ scan,
                                                                  uint32_t* __restrict__ alive,
                                                                  uint32_t* __restrict__ retuple) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b > nb) return;
  uint32_t a = 0, r = 0;
  if (b < nb) {
    const uint32_t s = dir_start[b], e = dir_start[b + 1];
    a = rank_of(mask, scan, e) != rank_of(mask, scan, s);
    r = a && !((mask[s >> 6] >> (s & 63)) & 1);
  }
  alive[b] = a;  // (b == nb: 0, the scans' last element is the total)
  retuple[b] = r;
}

__global__ __launch_bounds__(256) void hs_remove_dir_write_kernel(
    const uint64_t* __restrict__ dir_key, const uint32_t* __restrict__ dir_start, const int32_t* __restrict__ dir_tuple,
    const uint32_t* __restrict__ ids, uint32_t nb, uint32_t n, uint32_t nw, int K, const uint64_t* __restrict__ mask,
    const uint32_t* __restrict__ scan, const uint32_t* __restrict__ alive, const uint32_t* __restrict__ alive_scan,
    const uint32_t* __restrict__ retuple, const uint32_t* __restrict__ retuple_scan, uint32_t nb_new,
    uint64_t* __restrict__ out_key, int32_t* __restrict__ out_tuple, uint32_t* __restrict__ out_count,
    uint32_t* __restrict__ need_id, uint32_t* __restrict__ need_bucket) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb || !alive[b]) return;
  const uint32_t ob = alive_scan[b];
  if (ob >= nb_new) return;  // (never: no write outside the shrunken directory)
  const uint32_t s = dir_start[b], e = dir_start[b + 1];
  out_key[ob] = dir_key[b];
  out_count[ob] = rank_of(mask, scan, e) - rank_of(mask, scan, s);
  if (!retuple[b]) {
    for (int i = 0; i < K; ++i) out_tuple[(size_t)ob * K + i] = dir_tuple[(size_t)b * K + i];
    return;
  }
  // the new first member: the first set bit from s on (there is one in front of e: the bucket is alive)
  uint32_t w = s >> 6;
  uint64_t bits = mask[w] & ~below(s & 63);
  while (!bits && w < nw) bits = mask[++w];
  const uint32_t p = w * 64 + (uint32_t)__ffsll((unsigned long long)bits) - 1;
  const uint32_t j = retuple_scan[b];
  need_id[j] = p < n ? ids[p] : 0u;
  need_bucket[j] = ob;
}

__global__ __launch_bounds__(256) void hs_remove_tuples_put_kernel(const int32_t* __restrict__ ints,
                                                                   const uint32_t* __restrict__ need_bucket,
                                                                   uint32_t n_need, int K, uint32_t nb_new,
                                                                   int32_t* __restrict__ out_tuple) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_need * (uint32_t)K) return;
  const uint32_t j = t / (uint32_t)K, i = t - j * (uint32_t)K;
  const uint32_t ob = need_bucket[j];
  if (ob < nb_new) out_tuple[(size_t)ob * K + i] = ints[t];
}

template <int PW>
__global__ __launch_bounds__(256) void hs_remove_move_kernel(
    uint32_t n, uint32_t n_dst, const uint64_t* __restrict__ mask, const uint32_t* __restrict__ scan,
    const uint32_t* __restrict__ new_id, const uint32_t* __restrict__ src_ids, const uint4* __restrict__ src_packed,
    const uint4* __restrict__ src_rec, const uint32_t* __restrict__ src_rho, uint32_t* __restrict__ dst_ids,
    uint4* __restrict__ dst_packed, uint4* __restrict__ dst_rec, uint32_t* __restrict__ dst_rho) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint64_t m = mask[p >> 6];  // one word per wave
  if (!((m >> (p & 63)) & 1)) return;
  const uint32_t d = scan[p >> 6] + (uint32_t)__popcll(m & below(p & 63));
  if (d >= n_dst) return;  // (never, for masks and a scan that belong together)
  dst_ids[d] = new_id[src_ids[p]];
#pragma unroll
  for (int w = 0; w < PW; ++w) dst_packed[(size_t)d * PW + w] = src_packed[(size_t)p * PW + w];
  if (dst_rec) dst_rec[d] = src_rec[p];
  if (dst_rho) dst_rho[d] = src_rho[p];
}

// id order: codes [n][k] bytes, one thread per byte; packed_all [n][PW] 16-byte words, one thread per word
__global__ __launch_bounds__(256) void hs_remove_compact_codes_kernel(const uint8_t* __restrict__ src, uint64_t n, int k,
                                                                      const uint32_t* __restrict__ new_id,
                                                                      uint32_t n_dst, uint8_t* __restrict__ dst) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * (uint64_t)k) return;
  const uint64_t i = t / (uint64_t)k;
  const uint32_t d = new_id[i];
  if (d < n_dst) dst[(uint64_t)d * k + (t - i * (uint64_t)k)] = src[t];
}

__global__ __launch_bounds__(256) void hs_remove_compact_packed_kernel(const uint4* __restrict__ src, uint64_t n, int PW,
                                                                       const uint32_t* __restrict__ new_id,
                                                                       uint32_t n_dst, uint4* __restrict__ dst) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * (uint64_t)PW) return;
  const uint64_t i = t / (uint64_t)PW;
  const uint32_t d = new_id[i];
  if (d < n_dst) dst[(uint64_t)d * PW + (t - i * (uint64_t)PW)] = src[t];
}

}  // namespace

hipError_t hs_launch_remove_mark_ids(const uint32_t* d_ids, uint64_t m, uint32_t n, uint64_t* d_dead, uint32_t* d_flag,
                                     hipStream_t s) {
  if (!m) return hipSuccess;
  hs_remove_mark_ids_kernel<<<blocks_for(m), 256, 0, s>>>(d_ids, m, n, (unsigned long long*)d_dead, d_flag);
  return hipGetLastError();
}

hipError_t hs_launch_remove_mark_ranges(const uint64_t* d_first, const uint64_t* d_count, uint64_t n_ranges, uint32_t n,
                                        uint64_t* d_dead, hipStream_t s) {
  const uint64_t words = ((uint64_t)n + 63) / 64;
  const unsigned gx = (unsigned)std::min<uint64_t>(std::max<uint64_t>(1, (words + 255) / 256), 64);
  for (uint64_t r0 = 0; r0 < n_ranges; r0 += 32768) {
    const unsigned gy = (unsigned)std::min<uint64_t>(32768, n_ranges - r0);
    hs_remove_mark_ranges_kernel<<<dim3(gx, gy), 256, 0, s>>>(d_first, d_count, r0, n_ranges, n,
                                                              (unsigned long long*)d_dead);
  }
  return hipGetLastError();
}

hipError_t hs_launch_remove_masks_ids(const uint64_t* d_dead, uint32_t n, uint64_t* d_mask, uint32_t* d_cnt,
                                      hipStream_t s) {
  const uint32_t nw = (uint32_t)(((uint64_t)n + 63) / 64);
  hs_remove_masks_ids_kernel<<<blocks_for((uint64_t)nw + 1), 256, 0, s>>>((const unsigned long long*)d_dead, n, nw,
                                                                        d_mask, d_cnt);
  return hipGetLastError();
}

hipError_t hs_launch_remove_new_id(const uint64_t* d_mask, const uint32_t* d_scan, uint32_t n, uint32_t* d_new_id,
                                   hipStream_t s) {
  if (!n) return hipSuccess;
  hs_remove_new_id_kernel<<<blocks_for(n), 256, 0, s>>>(d_mask, d_scan, n, d_new_id);
  return hipGetLastError();
}

hipError_t hs_launch_remove_masks_tab(const uint32_t* d_ids, const uint64_t* d_dead, uint32_t n, uint64_t* d_mask,
                                      uint32_t* d_cnt, hipStream_t s) {
  const uint32_t nw = (uint32_t)(((uint64_t)n + 63) / 64);
  hs_remove_masks_tab_kernel<<<blocks_for(((uint64_t)nw + 1) * 64), 256, 0, s>>>(
      d_ids, (const unsigned long long*)d_dead, n, nw, d_mask, d_cnt);
  return hipGetLastError();
}

hipError_t hs_launch_remove_dir_flags(const uint32_t* d_dir_start, uint32_t nb, const uint64_t* d_mask,
                                      const uint32_t* d_scan, uint32_t* d_alive, uint32_t* d_retuple, hipStream_t s) {
  hs_remove_dir_flags_kernel<<<blocks_for((uint64_t)nb + 1), 256, 0, s>>>(d_dir_start, nb, d_mask, d_scan, d_alive,
                                                                        d_retuple);
  return hipGetLastError();
}

hipError_t hs_launch_remove_dir_write(const uint64_t* d_dir_key, const uint32_t* d_dir_start, const int32_t* d_dir_tuple,
                                      const uint32_t* d_ids, uint32_t nb, uint32_t n, int K, const uint64_t* d_mask,
                                      const uint32_t* d_scan, const uint32_t* d_alive, const uint32_t* d_alive_scan,
                                      const uint32_t* d_retuple, const uint32_t* d_retuple_scan, uint32_t nb_new,
                                      uint64_t* d_out_key, int32_t* d_out_tuple, uint32_t* d_out_count,
                                      uint32_t* d_need_id, uint32_t* d_need_bucket, hipStream_t s) {
  if (!nb) return hipSuccess;
  const uint32_t nw = (uint32_t)(((uint64_t)n + 63) / 64);
  hs_remove_dir_write_kernel<<<blocks_for(nb), 256, 0, s>>>(d_dir_key, d_dir_start, d_dir_tuple, d_ids, nb, n, nw, K,
                                                            d_mask, d_scan, d_alive, d_alive_scan, d_retuple,
                                                            d_retuple_scan, nb_new, d_out_key, d_out_tuple, d_out_count,
                                                            d_need_id, d_need_bucket);
  return hipGetLastError();
}

hipError_t hs_launch_remove_tuples_put(const int32_t* d_ints, const uint32_t* d_need_bucket, uint32_t n_need, int K,
                                       uint32_t nb_new, int32_t* d_out_tuple, hipStream_t s) {
  if (!n_need) return hipSuccess;
  hs_remove_tuples_put_kernel<<<blocks_for((uint64_t)n_need * K), 256, 0, s>>>(d_ints, d_need_bucket, n_need, K, nb_new,
                                                                             d_out_tuple);
  return hipGetLastError();
}

hipError_t hs_launch_remove_move(uint32_t n, uint32_t n_dst, const uint64_t* d_mask, const uint32_t* d_scan,
                                 const uint32_t* d_new_id, int PW, const uint32_t* d_src_ids, const uint4* d_src_packed,
                                 const uint4* d_src_rec, const uint32_t* d_src_rho, uint32_t* d_dst_ids,
                                 uint4* d_dst_packed, uint4* d_dst_rec, uint32_t* d_dst_rho, hipStream_t s) {
  if (!n || !n_dst) return hipSuccess;
#define HS_MOVE(P)                                                                                                 \
  hs_remove_move_kernel<P><<<blocks_for(n), 256, 0, s>>>(n, n_dst, d_mask, d_scan, d_new_id, d_src_ids, d_src_packed, \
                                                         d_src_rec, d_src_rho, d_dst_ids, d_dst_packed, d_dst_rec,   \
                                                         d_dst_rho)
  switch (PW) {
    case 1: HS_MOVE(1); break;
    case 2: HS_MOVE(2); break;
    case 3: HS_MOVE(3); break;
    default: return hipErrorInvalidValue;
  }
#undef HS_MOVE
  return hipGetLastError();
}

hipError_t hs_launch_remove_compact_ids(const uint8_t* d_codes, const uint4* d_packed_all, uint64_t n, int k, int PW,
                                        const uint32_t* d_new_id, uint32_t n_dst, uint8_t* d_codes_out,
                                        uint4* d_packed_out, hipStream_t s) {
  if (!n || !n_dst) return hipSuccess;
  hs_remove_compact_codes_kernel<<<blocks_for(n * (uint64_t)k), 256, 0, s>>>(d_codes, n, k, d_new_id, n_dst,
                                                                           d_codes_out);
  if (d_packed_out)
    hs_remove_compact_packed_kernel<<<blocks_for(n * (uint64_t)PW), 256, 0, s>>>(d_packed_all, n, PW, d_new_id, n_dst,
                                                                               d_packed_out);
  return hipGetLastError();
}
