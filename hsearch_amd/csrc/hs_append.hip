// hs_append.hip -- hs_index_append: one table of a built index grown by a block of new k-mers, on the device.
//
// A table is its entries ordered by (fingerprint, id), and the ids of an appended block are all larger than the
// index's.  So the grown table is the old one with the block's members placed BEHIND the old members of their
// bucket and the block's new buckets slotted in by fingerprint: a merge of two sorted, duplicate-free directories
// and one streaming move of the bucket-ordered arrays.  Nothing here hashes, sorts or gathers an old k-mer.
//
// The caller (hs_capi.hip, append_tables) has grouped the BLOCK as the build groups a table -- hash, fingerprints
// under the index's seed, sort by (fingerprint, id), exact tuple equality inside each run, run lengths -- into a block
// directory bkey / bstart / btuple of nbB buckets, and then runs, per table:
//   match       one lane per block bucket finds its fingerprint in the old directory (jump table + binary search, as
//               the probe does).  Found: the K ints are compared as HashKey strings with the bucket's dir_tuple,
//               *flag |= 1 where they differ (one fingerprint, two strings: the caller rebuilds from seed 0).  Not
//               found: the insertion rank r (old buckets with a smaller fingerprint), is_new = 1, ++inc[r].
//   <exclusive scans of is_new (over block buckets) and of inc (over old buckets)>
//   dir_old     old bucket b -> merged bucket b + (new buckets in front of it) = b + scan(inc)[b] + inc[b]; its key and
//               its TUPLE go there unchanged (its first member is still its smallest id), its count starts the sum
//   dir_block   block bucket j -> merged bucket (b or r) + scan(is_new)[j]; a new bucket brings key, tuple and count,
//               a matched one adds its count (one block bucket per merged bucket: no atomics)
//   <exclusive scan of the merged counts = dir_start'; their maximum = max_bucket>
//   bases       per old and per block bucket the constant shift of its entries: destination = base + source position
//   move        every entry of a source array (the old table's ids / packed / rec8 / rho, then the block's, which the
//               caller built in block-bucket order with the build's own record kernel) to base[bucket] + position.
//               A wave takes 64 consecutive source positions: one wave-uniform search finds the bucket of its first
//               position, every lane then searches the <= 64 buckets behind it; reads are contiguous, writes are
//               contiguous inside a bucket, all 16-byte accesses except ids and rho.
// Scratch is sized by the block and by one table's directory; the grown arrays are new allocations ([L][n + m]: the
// tables' stride changes with n) which the caller swaps in.  Peak extra HBM is therefore ONE grown copy of the
// bucket-ordered arrays plus that scratch -- never the build's n-sized hash and sort buffers.
#include "hs_internal.h"

namespace {

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + 255) / 256); }

__global__ __launch_bounds__(256) void hs_append_match_kernel(
    const uint64_t* __restrict__ bkey, const int32_t* __restrict__ btuple, uint32_t nbB, int K,
    const uint64_t* __restrict__ dir_key, const int32_t* __restrict__ dir_tuple, const uint32_t* __restrict__ dir_jump,
    uint32_t jump_shift, uint32_t nb, uint32_t* __restrict__ pos, uint32_t* __restrict__ is_new,
    uint32_t* __restrict__ inc, uint32_t* __restrict__ flag) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nbB) return;
  const uint64_t key = bkey[j];
  const uint32_t slot = (uint32_t)(key >> jump_shift);
  uint32_t lo = min(dir_jump[slot], nb), hi = min(dir_jump[slot + 1], nb);
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (dir_key[mid] < key) lo = mid + 1; else hi = mid;
  }
  const bool found = lo < nb && dir_key[lo] == key;
  pos[j] = lo;
  is_new[j] = found ? 0u : 1u;
  if (found) {
    if (!hs_key_equal(btuple + (size_t)j * K, dir_tuple + (size_t)lo * K, K)) atomicOr(flag, 1u);
  } else {
    atomicAdd(inc + lo, 1u);
  }
}

__global__ __launch_bounds__(256) void hs_append_dir_old_kernel(
    const uint64_t* __restrict__ dir_key, const uint32_t* __restrict__ dir_start, const int32_t* __restrict__ dir_tuple,
    uint32_t nb, int K, const uint32_t* __restrict__ inc, const uint32_t* __restrict__ inc_scan,
    uint32_t* __restrict__ map_old, uint64_t* __restrict__ out_key, int32_t* __restrict__ out_tuple,
    uint32_t* __restrict__ out_count) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  const uint32_t mb = b + inc_scan[b] + inc[b];
  map_old[b] = mb;
  out_key[mb] = dir_key[b];
  out_count[mb] = dir_start[b + 1] - dir_start[b];
  for (int i = 0; i < K; ++i) out_tuple[(size_t)mb * K + i] = dir_tuple[(size_t)b * K + i];
}

__global__ __launch_bounds__(256) void hs_append_dir_block_kernel(
    const uint64_t* __restrict__ bkey, const uint32_t* __restrict__ bstart, const int32_t* __restrict__ btuple,
    uint32_t nbB, int K, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ is_new,
    const uint32_t* __restrict__ new_scan, uint32_t* __restrict__ map_blk, uint32_t* __restrict__ old_cnt,
    uint64_t* __restrict__ out_key, int32_t* __restrict__ out_tuple, uint32_t* __restrict__ out_count) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nbB) return;
  const uint32_t mb = pos[j] + new_scan[j], cnt = bstart[j + 1] - bstart[j];
  map_blk[j] = mb;
  if (is_new[j]) {
    old_cnt[j] = 0;
    out_key[mb] = bkey[j];
    out_count[mb] = cnt;
    for (int i = 0; i < K; ++i) out_tuple[(size_t)mb * K + i] = btuple[(size_t)j * K + i];
  } else {
    const uint32_t c = out_count[mb];  // (hs_append_dir_old_kernel's, behind a kernel boundary)
    old_cnt[j] = c;
    out_count[mb] = c + cnt;
  }
}

// base[s] = the merged position of the segment's first entry minus its source position (mod 2^32)
__global__ __launch_bounds__(256) void hs_append_bases_kernel(
    const uint32_t* __restrict__ out_start, const uint32_t* __restrict__ dir_start, const uint32_t* __restrict__ map_old,
    uint32_t nb, const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ map_blk,
    const uint32_t* __restrict__ old_cnt, uint32_t nbB, uint32_t* __restrict__ base_old, uint32_t* __restrict__ base_blk) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t < nb) base_old[t] = out_start[map_old[t]] - dir_start[t];
  if (t < nbB) base_blk[t] = out_start[map_blk[t]] + old_cnt[t] - bstart[t];
}

// largest s in [lo, hi] with seg_start[s] <= p (seg_start[lo] <= p)
__device__ __forceinline__ uint32_t seg_of(const uint32_t* __restrict__ seg_start, uint32_t lo, uint32_t hi, uint32_t p) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (seg_start[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <int PW>
__global__ __launch_bounds__(256) void hs_append_move_kernel(
    uint32_t n_src, const uint32_t* __restrict__ seg_start, uint32_t n_seg, const uint32_t* __restrict__ base,
    uint32_t n_dst, const uint32_t* __restrict__ src_ids, uint32_t id_add, const uint4* __restrict__ src_packed,
    const uint4* __restrict__ src_rec, const uint32_t* __restrict__ src_rho, uint32_t* __restrict__ dst_ids,
    uint4* __restrict__ dst_packed, uint4* __restrict__ dst_rec, uint32_t* __restrict__ dst_rho) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  const uint32_t p0 = p & ~63u;  // the wave's first position: the same in every lane
  if (p0 >= n_src) return;
  const uint32_t s0 = seg_of(seg_start, 0, n_seg - 1, p0);
  if (p >= n_src) return;
  // segments are not empty: the segment of p0 + i lies at most i behind s0
  const uint32_t s = seg_of(seg_start, s0, min(s0 + (p - p0), n_seg - 1), p);
  const uint32_t d = base[s] + p;
  if (d >= n_dst) return;  // (never, for a directory that passed its checks: no write outside the grown arrays)
  dst_ids[d] = src_ids[p] + id_add;
#pragma unroll
  for (int w = 0; w < PW; ++w) dst_packed[(size_t)d * PW + w] = src_packed[(size_t)p * PW + w];
  if (dst_rec) dst_rec[d] = src_rec[p];
  if (dst_rho) dst_rho[d] = src_rho[p];
}

}  // namespace

hipError_t hs_launch_append_match(const uint64_t* d_bkey, const int32_t* d_btuple, uint32_t nbB, int K,
                                  const uint64_t* d_dir_key, const int32_t* d_dir_tuple, const uint32_t* d_dir_jump,
                                  uint32_t jump_shift, uint32_t nb, uint32_t* d_pos, uint32_t* d_is_new,
                                  uint32_t* d_inc, uint32_t* d_flag, hipStream_t s) {
  if (!nbB) return hipSuccess;
  hs_append_match_kernel<<<blocks_for(nbB), 256, 0, s>>>(d_bkey, d_btuple, nbB, K, d_dir_key, d_dir_tuple, d_dir_jump,
                                                         jump_shift, nb, d_pos, d_is_new, d_inc, d_flag);
  return hipGetLastError();
}

hipError_t hs_launch_append_dir(const uint64_t* d_dir_key, const uint32_t* d_dir_start, const int32_t* d_dir_tuple,
                                uint32_t nb, const uint64_t* d_bkey, const uint32_t* d_bstart, const int32_t* d_btuple,
                                uint32_t nbB, int K, const uint32_t* d_pos, const uint32_t* d_is_new,
                                const uint32_t* d_new_scan, const uint32_t* d_inc, const uint32_t* d_inc_scan,
                                uint32_t* d_map_old, uint32_t* d_map_blk, uint32_t* d_old_cnt, uint64_t* d_out_key,
                                int32_t* d_out_tuple, uint32_t* d_out_count, hipStream_t s) {
  if (nb)
    hs_append_dir_old_kernel<<<blocks_for(nb), 256, 0, s>>>(d_dir_key, d_dir_start, d_dir_tuple, nb, K, d_inc,
                                                            d_inc_scan, d_map_old, d_out_key, d_out_tuple, d_out_count);
  if (nbB)
    hs_append_dir_block_kernel<<<blocks_for(nbB), 256, 0, s>>>(d_bkey, d_bstart, d_btuple, nbB, K, d_pos, d_is_new,
                                                               d_new_scan, d_map_blk, d_old_cnt, d_out_key, d_out_tuple,
                                                               d_out_count);
  return hipGetLastError();
}

hipError_t hs_launch_append_bases(const uint32_t* d_out_start, const uint32_t* d_dir_start, const uint32_t* d_map_old,
                                  uint32_t nb, const uint32_t* d_bstart, const uint32_t* d_map_blk,
                                  const uint32_t* d_old_cnt, uint32_t nbB, uint32_t* d_base_old, uint32_t* d_base_blk,
                                  hipStream_t s) {
  const uint32_t most = nb > nbB ? nb : nbB;
  if (!most) return hipSuccess;
  hs_append_bases_kernel<<<blocks_for(most), 256, 0, s>>>(d_out_start, d_dir_start, d_map_old, nb, d_bstart, d_map_blk,
                                                          d_old_cnt, nbB, d_base_old, d_base_blk);
  return hipGetLastError();
}

hipError_t hs_launch_append_move(uint32_t n_src, const uint32_t* d_seg_start, uint32_t n_seg, const uint32_t* d_base,
                                 uint32_t n_dst, int PW, const uint32_t* d_src_ids, uint32_t id_add,
                                 const uint4* d_src_packed, const uint4* d_src_rec, const uint32_t* d_src_rho,
                                 uint32_t* d_dst_ids, uint4* d_dst_packed, uint4* d_dst_rec, uint32_t* d_dst_rho,
                                 hipStream_t s) {
  if (!n_src || !n_seg) return hipSuccess;
#define HS_MOVE(P)                                                                                                    \
  hs_append_move_kernel<P><<<blocks_for(n_src), 256, 0, s>>>(n_src, d_seg_start, n_seg, d_base, n_dst, d_src_ids,     \
                                                             id_add, d_src_packed, d_src_rec, d_src_rho, d_dst_ids,   \
                                                             d_dst_packed, d_dst_rec, d_dst_rho)
  switch (PW) {
    case 1: HS_MOVE(1); break;
    case 2: HS_MOVE(2); break;
    case 3: HS_MOVE(3); break;
    default: return hipErrorInvalidValue;
  }
#undef HS_MOVE
  return hipGetLastError();
}
