/* hsearch.h -- C ABI of the MI355X-native motif-search hot path (libhsearch_amd.so).
 *
 * The reference (acgtun/hsearch) has no FFI or plugin interface: its operator surface is the set of
 * C++ free functions and the LSH class in hclust/src/hclust/ (SURVEY.md 8b).  This header is the
 * boundary a maintainer of the reference would bind instead of those functions; each entry point
 * names the reference interface it replaces.  INTEGRATION.md shows the reference-side call sites.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; every function returns an hs_status and never
 *     throws; hs_last_error() gives the message of the last failure on a handle;
 *   - the caller owns every buffer it passes in; the library owns device memory behind the handle;
 *   - functions WITHOUT a _dev suffix take HOST pointers and copy over PCIe; the _dev variants
 *     take DEVICE pointers (HBM-resident inputs/outputs) and are what bench.py times.  The library
 *     works on streams of its own and returns with them drained: device buffers a caller hands in must
 *     be COMPLETE (whatever the caller has queued on its own streams to fill them: finished) at the
 *     call, and are ready for any stream when it returns;
 *   - output capacity is explicit: when results exceed `cap` the call returns HS_ERR_CAPACITY and
 *     *n_out holds the required capacity (two-call pattern);
 *   - a handle is bound to one GPU and is not thread-safe; use one handle per GPU / process;
 *   - requires a gfx950 device: there is no CPU fallback, calls fail with HS_ERR_NO_DEVICE.
 *
 * Layouts (all row-major, densely packed)
 *   codes   [n][k]      uint8   rows of the coordinate table (0..alphabet-1), see hs_tables.h
 *   points  [n][d]      double  d = 8*k
 *   planes  a[L][K][d], b[L][K] double  (LSH::a, LSH::b of table l -- lsh.hpp:65-66)
 *   buckets [n][L][K]   int32
 */
#ifndef HSEARCH_H
#define HSEARCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HS_API __attribute__((visibility("default")))

typedef enum hs_status {
  HS_OK = 0,
  HS_ERR_INVALID = 1,       /* bad argument */
  HS_ERR_NO_DEVICE = 2,     /* no usable gfx950 device */
  HS_ERR_HIP = 3,           /* a HIP runtime call failed (see hs_last_error) */
  HS_ERR_CAPACITY = 4,      /* output buffer too small; required size reported */
  HS_ERR_STATE = 5,         /* e.g. query before hs_index_build */
  HS_ERR_KEY_COLLISION = 6, /* 64-bit key fingerprints collided for every retry seed */
  HS_ERR_NOMEM = 7,
  HS_ERR_IO = 8,            /* index file missing, truncated, or written for other parameters */
  HS_ERR_PEER = 9           /* hsearch_dist.h: ANOTHER rank of the communicator failed before the exchange;
                               nothing was exchanged (the failed rank returns its own status) */
} hs_status;

/* Replaces the (dimension, hash_K, hash_W) arguments of LSH::LSH (lsh.hpp:10-17) and the
 * (hash_K, hash_L, hash_W) arguments of Search()/Clustering() (motif_both_points.cpp:195-203,
 * hclust2.cpp:86-91).  DIMENSION = AACoordinateSize * KMERLENGTH (motif_both_points.cpp:337-338). */
typedef struct hs_params {
  uint32_t k;      /* residues per k-mer (KMERLENGTH); d = 8*k */
  uint32_t K;      /* hash functions per table (hash_K), 1..32 */
  uint32_t L;      /* hash tables (hash_L), 1..32 */
  double W;        /* bucket width (hash_W) */
  int32_t device;  /* HIP device ordinal */
  uint32_t alphabet; /* rows of the coordinate table, 1..32; 0 means 20 (the amino acids) */
} hs_params;

typedef struct hs_handle hs_handle;

/* Phase timings (HIP events on the library's stream) and counters of the LAST call on a handle. */
typedef struct hs_profile {
  double ms_hash;        /* projection + bucket ints + key fingerprints */
  double ms_sort;        /* build: radix sort + directory */
  double ms_gather;      /* build: bucket-ordered packed-code copies */
  double ms_probe;       /* query: directory lookup */
  double ms_verify;      /* query: candidate scan kernel (the dominant kernel) */
  double ms_finalize;    /* query: dedupe + exact fp64 distance + ordering of hits */
  double ms_total;       /* whole call, device side */
  uint64_t candidates;   /* sum over (q, l) of |B_l(q)| scanned by the last query call */
  uint64_t provisional;  /* candidates that passed the fp32 filter */
  uint64_t hits;
  uint64_t verify_launches;
  uint64_t join_batches;   /* query batches in which the MFMA bucket join ran */
  double ms_join;          /* of ms_verify: the hs_join_kernel part (rest = streaming kernel) */
  uint64_t join_items;     /* (member tile, query group) work items of the join */
  uint64_t join_pairs;     /* (member, query) pairs routed to the join */
  uint64_t join_pairs_issued; /* MFMA rows x columns actually issued for them (padding included) */
  uint64_t join_i8_batches;   /* of join_batches: those run by the int8 form (hs_join8_kernel) */
  uint64_t hash_values;       /* bucket ints produced by the MFMA projection pass (hs_proj_kernel) ... */
  uint64_t hash_flagged;      /* ... of which this many lay within the error bound of a bucket boundary
                                 and were recomputed in the reference's fp64 order (hs_proj_fix_kernel) */
  uint32_t join_row_bytes;    /* int8 join of the last batch: bytes of a row = GEMM depth (128 / 192 / 256; 0:
                                 it did not run) ... */
  uint32_t join_wide;         /* ... and 1 if the rows carried all 8 coordinate columns (short k-mers, large
                                 radii), 0 for the 4 filter columns */
  uint64_t join_items_resident; /* of join_items: those of segments with few probing queries, run by the
                                   query-resident kernel (hs_join8r_kernel) */
  uint64_t join_async_retries; /* batches whose join was launched on a capacity hint that turned out too small
                                  (or illegal) and ran a second time: exclude such a call from kernel timings */
  uint64_t queries_recognised; /* hs_query / hs_query_dev: the call's centres were all k-mers (every 8 doubles a
                                  row of the coordinate table) and ran from their residue codes: this many */
  uint64_t join_f6_batches;    /* of join_i8_batches: those whose query-streaming kernel was the FP6 form
                                  (hs_join6x_kernel: queries that are k-mers, k = 21..25).  join_row_bytes stays
                                  128 for them: the depth of the GEMM, not the bytes of an FP6 row (96) */
  uint64_t join_f6_wide_items; /* of join_items: those of 192 members, run by the FP6 form's 12-row-tile kernel
                                  (hs_join6w_kernel, HS_OPT_JOIN_F6_FORM); 0 for a batch on hs_join6x_kernel */
  uint64_t append_rebuilds;    /* hs_index_append*: 1 if the last append fell back to the full build over the
                                  concatenated codes (a fingerprint shared by two HashKey strings), else 0 */
  uint64_t append_new_buckets; /* hs_index_append*: buckets the block created, summed over the tables */
  uint64_t remove_rebuilds;    /* hs_index_remove*: 1 if the last removal ran the full build loop over the surviving
                                  codes (the index's key_seed was above 0), else 0 */
  uint64_t remove_dead_buckets; /* hs_index_remove*: buckets that lost all their members, summed over the tables */
  uint64_t remove_retupled;    /* hs_index_remove*: buckets whose first member went while others stayed, so that
                                  their tuple was recomputed from the new first member; summed over the tables */
  uint64_t pssm_pairs;         /* hs_pssm_scan*: (profile, k-mer) pairs of the profiles that were not dead: nm_live * n */
  uint64_t pssm_survivors;     /* ... of which this many passed the MFMA filter and went to the exact pass (with
                                  HS_OPT_PSSM_FILTER = 0: all of them) */
  uint64_t pssm_dead;          /* ... profiles skipped because no k-mer can reach their threshold (filter on only) */
  uint64_t pssm_mfma_steps;    /* ... MFMA depth steps per 16 x 16 tile: ceil(k * alphabet / 128) (0: filter off) */
  uint64_t pssm_seq_rows;      /* hs_pssm_seq_scan*: the (profile, sequence) rows the call found (its *n_out) */
  uint64_t pssm_fam_rows;      /* hs_pssm_family_scan*: the (family, sequence, diagonal) rows before the row filters */
  uint64_t pssm_fam_kept;      /* ... of which this many passed min_count and t_group (the call's *n_out) */
  uint64_t pssm_chain_segs;    /* hs_pssm_family_chain*: the (family, sequence) segments before the filters */
  uint64_t pssm_chain_kept;    /* ... of which this many report a chain (the call's *n_out) */
  uint64_t pssm_count_sites;   /* hs_pssm_hit_counts*: the sites counted, the sum of used[] */
  uint64_t pssm_count_items;   /* hs_pssm_hit_counts*: the (profile run, chunk) work items of the counting kernel */
  uint64_t pssm_weight_sites;  /* hs_pssm_weighted_counts*: the sites weighted (pssm_count_sites; 0 after other calls) */
  uint64_t pssm_weight_items;  /* hs_pssm_weighted_counts*: the work items of the weight kernel (pssm_count_items) */
  uint64_t pssm_null_bins;     /* hs_pssm_pvalue*: the bins B of the score grid the call used (HS_OPT_PSSM_NULL_BINS) */
  uint64_t pssm_null_profiles; /* hs_pssm_pvalue*: profiles whose null distribution the call convolved */
  uint64_t summary_weight_rows;  /* hs_cluster_weighted_profile*: the rows weighted (the call's *n_out; 0 after other calls) */
  uint64_t summary_weight_items; /* hs_cluster_weighted_profile*: the work items of the weight kernel, summed over the
                                    row batches */
  uint64_t pssm_cmp_pairs;     /* hs_pssm_compare*: the (x, y) pairs the call examined (self mode: those with x < y) */
  uint64_t pssm_cmp_survivors; /* ... of which this many passed the int8 MFMA filter and went to the exact pass (with
                                  HS_OPT_PSSM_CMP_FILTER = 0, or a shape the filter does not run on: all of them) */
  uint64_t pssm_cmp_steps;     /* ... 64-byte MFMA depth steps per 16 x 16 tile, summed over the offsets (0: no filter) */
  uint64_t pssm_rank_sample;  /* hs_pssm_rank*: the sample size n_s = min(n, HS_OPT_PSSM_RANK_SAMPLE) the call used */
  uint64_t pssm_rank_retries;  /* hs_pssm_rank*: the sum of rounds[]: profiles times the extra rounds they took */
  uint64_t pssm_topk_sample;   /* hs_pssm_topk*: the sample size n_s = min(n, HS_OPT_PSSM_TOPK_SAMPLE) the call used */
  uint64_t pssm_topk_raised;   /* hs_pssm_topk*: profiles scanned at a threshold above their floor (t_used > floor) */
} hs_profile;

typedef struct hs_index_info {
  uint64_t n;               /* DB k-mers */
  uint64_t device_bytes;    /* HBM held by the index */
  uint64_t n_buckets[32];   /* distinct keys of table l (the reference prints this, :217) */
  uint64_t max_bucket[32];  /* population of the largest bucket of table l */
  uint32_t key_seed;        /* fingerprint seed that produced a collision-free directory */
} hs_index_info;

/* ---- lifetime ------------------------------------------------------------------------------- */

/* Replaces L constructions of LSH (lsh.hpp:10-31), except that the planes are an INPUT: the
 * reference draws them from std::random_device (lsh.hpp:19-20), which no caller can reproduce.
 * coords: [alphabet][8] embedding table, or NULL for HS_AA_COORDS (util.hpp:21-42).  A caller whose
 * DB arrives as points (the reference's points files carry the table rounded to 6 significant
 * digits, protein2datapoints.cpp:23-29) passes the distinct 8-tuples it found as the table and the
 * row indices as codes, so both sides hash exactly the same doubles. */
HS_API hs_status hs_create(const hs_params* params, const double* a, const double* b,
                           const double* coords, hs_handle** out);
HS_API void hs_destroy(hs_handle* h);
/* A new hash family (same k, K, L, W) for an existing handle: what constructing the next LSHTable
 * does in Clustering() (hclust2.cpp:104, one fresh family per table).  Drops the index (queries
 * return HS_ERR_STATE until the next build); device buffers are kept. */
HS_API hs_status hs_set_planes(hs_handle* h, const double* a, const double* b);
HS_API const char* hs_last_error(const hs_handle* h);
HS_API hs_status hs_get_profile(const hs_handle* h, hs_profile* out);
/* The parameters the handle was created with (alphabet resolved to the row count in use). */
HS_API hs_status hs_get_params(const hs_handle* h, hs_params* out);
/* Candidate-verification kernel: 0 = auto (bucket join when legal, else streaming), 1 = streaming
 * scan (hs_verify_kernel), 2 = MFMA bucket join wherever it is legal (int8 hs_join8_kernel, else
 * fp16 hs_join_kernel), 3 = the fp16 join only.  All are filters in front of the same exact fp64
 * decision, so results are identical; the environment variable HS_VERIFY_MODE=stream|join|join16
 * sets the default of new handles. */
HS_API hs_status hs_set_verify_mode(hs_handle* h, int mode);
/* How LSH::HashBucketIndex (lsh.hpp:33-49) is evaluated: 0 = auto (the int8 MFMA projection with a
 * proven error bound, values within the bound of a bucket boundary recomputed in the reference's
 * fp64 order -- hs_proj.hip -- unless the bound is so wide that most values would be recomputed,
 * or k > 52), 1 = the exact fp64 vector-ALU kernel only, 2 = the MFMA pass wherever it is compiled
 * (k <= 52).  Bucket integers are bit-identical in every mode.  eps_scale >= 1 inflates the error
 * bound (tests: more values take the recompute path); 1 is the proven bound.  The environment
 * variable HS_HASH_MODE=exact|mfma sets the default of new handles. */
HS_API hs_status hs_set_hash_mode(hs_handle* h, int mode, double eps_scale);
/* Path selection and batch sizing of a handle.  No option changes a result: each forces one of several
 * equivalent paths (the tests run both and compare) or sizes a batch.  Unknown option / value out of range:
 * HS_ERR_INVALID.  Options that shape the index (HS_OPT_BUILD_GROUPING) take effect at the next build. */
typedef enum hs_option {
  HS_OPT_QUERY_BATCH = 1,    /* queries per internal batch of a query call; 0 (default) = by L and free HBM;
                                at most 2^31 / L - 1 (a probe's number carries a flag in bit 31) */
  HS_OPT_SEG_MODE = 2,       /* grouping of the probes by bucket: 0 by the bucket : probe ratio, 1 sort the
                                probes, 2 counting sort over the bucket slots */
  HS_OPT_JOIN_RESIDENT = 3,  /* segments with few probing queries through hs_join8r_kernel: 0 by their share of
                                the previous batches' work items, 1 never, 2 always */
  HS_OPT_RECOGNISE_KMERS = 4,/* 1 (default): centres that are rows of the coordinate table run from their residue
                                codes; 0: always as points */
  HS_OPT_BUILD_GROUPING = 5, /* 0 (default): exact-membership table + radix sort on bucket ranks; 1: radix sort of
                                (fingerprint, id) pairs */
  HS_OPT_WIDE_ROWS = 6,      /* int8 rows over all 8 coordinate columns for k = 21..25: 0 by radius, 1 always,
                                2 never by radius; 3: 4-column rows for k <= 20 as well (drops the index: the
                                member records are built for one form) */
  HS_OPT_REFINE8 = 7,        /* 1 (default): survivors of the 4-column bound pass the 8-column bound first */
  HS_OPT_SELF_CODES = 8,     /* 1 (default): the self-join runs from residue codes; 0: from embedded centres */
  HS_OPT_SORT_HITS = 10,     /* 1: order a batch's hits by a radix sort of the whole list, not per query */
  HS_OPT_SYNC_ITEMS = 11,    /* 1: read the join's work-item count back before launching it */
  HS_OPT_JOIN_MIN_Q = 12,    /* segments with fewer probing queries ... */
  HS_OPT_JOIN_MIN_M = 13,    /* ... or fewer members (and fewer than 512) go to the streaming filter instead of the
                                join (default 1 / 1: none do) */
  HS_OPT_SORT_FROM_BIT = 14, /* HS_OPT_BUILD_GROUPING = 1: lowest fingerprint bit the first sort looks at (0..60) */
  HS_OPT_BUILD_SERIAL = 15,  /* 1: no overlap of a table's hashing with the previous table's grouping */
  HS_OPT_PROBE_RECORDS = 17, /* 1 (default): a probe reads one 64-byte directory record per bucket (fingerprint,
                                boundaries, the bucket ints as int16) where the index has them -- K <= 24 and
                                every bucket int of the table within 16 bits; 0: the directory arrays */
  HS_OPT_JOIN_CHUNK = 18,    /* work items a wave of hs_join8x_kernel takes per access to the item counters (2..64);
                                0 (default): from the previous batch's pairs per item */
  HS_OPT_SUMMARY_CHUNK = 19, /* hs_cluster_profile / hs_cluster_radii: member slots per work item (1 .. 2^20); 0 (default): 512 */
  HS_OPT_SUMMARY_ROWS = 20,  /* hs_cluster_profile: rows per batch; 0 (default): as many as a fixed scratch budget of
                                32 MB of counts holds */
  HS_OPT_MSF_EDGE_BUDGET = 21, /* hs_msf: bytes of HBM a call may spend on keeping the self-join's pairs (16 per
                                unordered pair) for its rounds.  0: never keep them (every pass is a self-join);
                                -1 (default): a quarter of the HBM that is free when the call starts.  The list grows
                                with the pairs, so a call takes what its graph needs, not the budget */
  HS_OPT_JOIN_F6 = 22,       /* 1 (default): batches whose queries are k-mers (codes, recognised centres, the
                                self-join from codes), k = 21..25, 4-column rows, run the query-streaming join on
                                FP6 MFMA (hs_join6x_kernel); 0: never (hs_join8x_kernel) */
  HS_OPT_PSSM_FILTER = 23,   /* hs_pssm_scan: 1 (default): the FP6 MFMA filter in front of the exact pass; 0: no filter,
                                every (profile, k-mer) pair goes to the exact pass */
  HS_OPT_PSSM_TOPK_SAMPLE = 24, /* hs_pssm_topk: k-mers of the index the sample pass scores per profile (>= 1, default
                                262144 = 2^18; the index's size where it is smaller).  Shows in t_used only, never in a row */
  HS_OPT_PSSM_COUNT_CHUNK = 25, /* hs_pssm_hit_counts: sites per work item of the counting kernel (1 .. 2^20); 0 (default):
                                a batch's sites / 4096, within 256 .. 2048.  Never shows in a count */
  HS_OPT_PSSM_RANK_SAMPLE = 26, /* hs_pssm_rank: k-mers of the index the sample pass scores per profile (>= 1, default
                                262144 = 2^18; the index's size where it is smaller).  Shows in t_scan and rounds only */
  HS_OPT_PSSM_NULL_BINS = 27, /* hs_pssm_pvalue, hs_pssm_pvalue_threshold: bins of the score grid the null distribution
                                 is convolved on (64 .. 8192, default 4096): more bins, a tighter p_hi / p_lo */
  HS_OPT_JOIN_F6_FORM = 28,  /* the FP6 join's kernel: 0: hs_join6x_kernel (work items of 128 members); 1:
                                hs_join6w_kernel (items of 192 members: a query tile feeds 24 MFMAs, not 16); -1
                                (default): automatic, which is 1 wherever HS_OPT_JOIN_F6 applies.  Never shows in
                                a result */
  HS_OPT_PSSM_CMP_FILTER = 29, /* hs_pssm_compare: 1 (default): the int8 MFMA filter in front of the exact pass
                                  wherever its shape allows; 0: every pair to the exact pass.  Never shows in a result */
  HS_OPT_JOIN_XCD_RUN = 16 /* hs_join8x_kernel's work items dealt in runs of this many chunks per XCD, each XCD's
                                waves on their own runs (a run's items stream the same query tiles: one L2 fetches
                                them instead of eight).  0: one counter for the chip; -1 (default): by the size
                                of the batch's query-tile array */
} hs_option;
HS_API hs_status hs_set_option(hs_handle* h, int option, int64_t value);

/* ---- the FP6 join filter (HS_OPT_JOIN_F6), as far as a caller can inspect it -------------------- */
/* Its tables from a coordinate table ([alphabet][8] doubles), computed on the host (no GPU): *s = the scale
 * 7.5 / max |x| over columns 0..3, codes [32][4] the six-bit e2m3 codes of s x, e / r [32] the per-residue error
 * share and threshold (e[a] + e[b] >= s^2 x_a.x_b - X^[a].X^[b] for every residue pair; r[a] = s^2 |x_a|^2 / 2
 * - e[a]), pair [1024][2] the kernel's lookup table (entry r1 << 5 | r0: the 2 x 24 code bits of both residues).
 * Any output may be NULL. */
HS_API hs_status hs_join6_tables(const double* coords, uint32_t alphabet, double* s, uint8_t* codes, double* e,
                                 double* r, uint32_t* pair);
/* What the kernels carry for n k-mers (kmers [n][k], k <= 25) at squared radii r2 [n], in units of 2^-6, on the
 * host: rho64 = a member's rho as its 16-byte record encodes it (floor - 1, lower where its digits end), c64 = a
 * query's accumulator start -(gamma + rho0), *rho0_64 = the offset rho is carried against, rec [n][4] the member
 * records.  Filter value of member x and query c, in 64ths: sum_p X^[x_p].X^[c_p] * 64 - (rho64[x] - rho0_64) +
 * c64[c]; a pair within the query's radius has it >= 1. */
HS_API hs_status hs_join6_thresholds(const double* coords, uint32_t alphabet, const uint8_t* kmers, uint64_t n,
                                     uint32_t k, const double* r2, int64_t* rho64, int64_t* c64, int64_t* rho0_64,
                                     uint32_t* rec);
/* Where the gathered query rows of the FP6 join lie, on the host: a row is 8 pieces of 16 bytes (piece g < 4 =
 * dwords 0..3 of the operand's lane quarter g, piece 4 + g = dwords 4, 5 of quarter g and the threshold C twice);
 * the byte offset of piece `piece` of row `row` inside a tile of nr <= 32 rows (a full tile: four 1 KB planes in
 * the kernel's lane order; the ragged last tile of a segment: piece-major).  A bijection onto nr * 128 bytes.
 * 0xffffffff for arguments out of range. */
HS_API uint32_t hs_join6_tile_offset(uint32_t nr, uint32_t row, uint32_t piece);
/* GPU: hs_join6x_kernel's tile product (v_mfma_f32_16x16x128_f8f6f4, e2m3 operands, the kernel's lane map) on
 * rows at the format's extremes -- all-maximum, alternating signs, thresholds of +-2^17, pseudo-random codes --
 * against int64 arithmetic on the device.  variant 0: as the kernel issues it; 1: with explicit block scales of
 * 2^0.  *mismatches = accumulators that differ (0: exact); first_bad (NULL or 4 words): case, lane * 4 +
 * register, the float's bits, the expected value in 64ths. */
HS_API hs_status hs_join6_selftest(int device, int variant, uint64_t* mismatches, uint32_t* first_bad);
/* Bucket partition -- unlike the options above this CHANGES what a query call returns.  With n_parts > 1 the
 * searches of this handle (hs_query*, not the self-joins) probe only the buckets that fall to `part` of
 * `n_parts` (a fixed function of the probe's K bucket ints, the same on every handle; for the few buckets of
 * more than max(4096, n / 1024) members a function of the bucket ints AND of the query's number in the call, so
 * that a giant bucket's queries are shared among the parts instead of the bucket landing on one of them): the
 * loop over tables and buckets of motif_both_points.cpp:224-238 cut by BUCKET.
 * Every (query, table) probe belongs to exactly one part -- provided every part is given the same queries in
 * the same order --, so the union over the parts of the hits is the full call's hits plus
 * later-table sightings of ids an earlier table of another part already had: hs_merge_first_table_dev (per
 * (query, id) the smallest table, order (query, table, id)) of the parts' lists IS the full call's output.  n
 * GPUs with the index replicated and ALL queries on every GPU then share the buckets instead of the queries:
 * each meets 1/n of the probes with all the queries there are per bucket (hs_comm_query_buckets in
 * include/hsearch_dist.h).  n_parts = 1 (part 0): everything, the default. */
HS_API hs_status hs_set_bucket_partition(hs_handle* h, uint32_t part, uint32_t n_parts);
/* Multi-probe LSH (Lv et al., VLDB 2007) -- like the bucket partition this CHANGES what a query call returns.  With
 * extra_probes = T > 0 the searches of this handle (hs_query*, hs_query_dev, hs_query_codes*; NOT hs_self_join*,
 * hs_clustering* or hs_bruteforce*, which ignore the setting) look, in every table, in the query's own bucket and
 * in the T neighbouring buckets it is most likely to have neighbours in:
 *   1. v_j = (dot_j + b_j) / W in the reference's fp64 order (lsh.hpp:33-49), h_j = floor(v_j), x_j = v_j - h_j;
 *   2. the 2K boundary distances z(j,-1) = x_j, z(j,+1) = 1 - x_j, sorted ascending by (z, j, delta);
 *   3. a perturbation set A (sorted indices, a 64-bit mask) scores sum of z_i * z_i over A in ascending i, each
 *      product and sum rounded; it is valid unless it holds both deltas of one j;
 *   4. a min-heap on (score, mask) starts with {0}; a pop with largest element m pushes shift (m -> m + 1) and
 *      expand (m + 1 added) while m + 1 < 2K, and a valid pop is emitted; generation ends after T emitted sets or
 *      4 (T + 1) pops.  Slots left over are empty probes, which find no bucket;
 *   5. probe 0 is the home bucket h, probe t >= 1 is h + delta over the t-th emitted set.
 * A hit is (q, id) with id in any probed bucket and d2 <= R*R, reported with the smallest table l in which some
 * probe of q holds it, in the order (query, table, id); cand[q][l] sums the sizes of table l's probed buckets.
 * With T > 0 the queries' bucket ints come from the exact fp64 pass whatever hs_set_hash_mode says.  0 <= T <= 63
 * and T <= 3^K - 1, else HS_ERR_INVALID.  The setting belongs to the handle: 0 by default, kept across
 * hs_index_build / hs_index_load / hs_set_planes, never written into index files.  T = 0 is the one-probe search. */
HS_API hs_status hs_set_multiprobe(hs_handle* h, uint32_t extra_probes);
/* The probe sequence of nq points (host pointers, centers [nq][d]) under the handle's T (P = 1 + T):
 * buckets[nq][L][P][K] the bucket ints each probe looks up, in probe order; valid[nq][L][P] 0 for the empty slots
 * of rule 4 (their ints repeat the home bucket's).  With T = 0 buckets equals hs_hash_points. */
HS_API hs_status hs_probe_buckets(hs_handle* h, const double* centers, uint64_t nq, int32_t* buckets, uint8_t* valid);
/* The library's work after this call starts only once `hip_event` (a hipEvent_t the caller has recorded on a
 * stream of its own) has completed: the device-side alternative to draining that stream before a _dev call. */
HS_API hs_status hs_wait_event(hs_handle* h, void* hip_event);
HS_API const char* hs_version(void);

/* ---- embedding + hashing (rows a2, a4, a5, a6) ----------------------------------------------- */

/* KmerToCoordinates (hclust2.cpp:49-62) for n k-mers given as codes: out[n][d]. */
HS_API hs_status hs_embed_codes(hs_handle* h, const uint8_t* codes, uint64_t n, double* out);

/* LSH::HashBucketIndex (lsh.hpp:44-49) for every (point, table, function): bit-exact ints,
 * strict left-to-right fp64 with separate multiply and add as lsh.hpp:33-42 evaluates it. */
HS_API hs_status hs_hash_codes(hs_handle* h, const uint8_t* codes, uint64_t n, int32_t* buckets);
HS_API hs_status hs_hash_points(hs_handle* h, const double* points, uint64_t n, int32_t* buckets);

/* LSH::HashKey (lsh.hpp:51-59): decimal strings of K ints concatenated without separator.
 * Host-side helper; returns the length, writes a NUL-terminated string of at most cap-1 chars. */
HS_API uint32_t hs_key_string(const int32_t* buckets, uint32_t K, char* out, uint32_t cap);
/* Diagnostics (host-side, no GPU): the 64-bit fingerprint of that character stream under which the
 * index groups keys, and the exact HashKey string equality of two K-tuples (the index never trusts
 * the fingerprint alone: it re-checks equality at build and at probe time). */
HS_API uint64_t hs_key_fingerprint(const int32_t* buckets, uint32_t K, uint32_t seed);
HS_API int hs_key_strings_equal(const int32_t* x, const int32_t* y, uint32_t K);

/* ---- index build (row a7) --------------------------------------------------------------------- */

/* Replaces the build loop of Search() (motif_both_points.cpp:206-218) / BuildLSHTalbe
 * (hclust2.cpp:74-84): L tables keyed by HashKey string equality, ids ascending inside a bucket.
 * The DB is kept as residue codes (k bytes per k-mer), never as 8k doubles. */
HS_API hs_status hs_index_build(hs_handle* h, const uint8_t* codes, uint64_t n);

/* Index over a SUBSET of a code array that stays the same across calls -- what BuildLSHTalbe does
 * per table inside Clustering() (hclust2.cpp:74-84: the k-mers with merged != 2).  codes_all
 * [n_all][k] crosses PCIe on the first call with this (pointer, n_all) and is kept on the device
 * (the caller must not change it while it keeps calling; a call with another pointer or n_all
 * replaces the copy); every call gathers the rows subset[0 .. n_subset) on the device -- DB id i of
 * the new index = row subset[i]; subset == NULL means all rows in order -- and builds the index. */
HS_API hs_status hs_index_build_subset(hs_handle* h, const uint8_t* codes_all, uint64_t n_all,
                                       const uint32_t* subset, uint64_t n_subset);

/* SURVEY 8(f) row 1 -- k-mer enumeration on the device.  The DB is every length-k window of every
 * sequence of one concatenated residue-code buffer: sequence s occupies residues[seq_start[s] ..
 * seq_start[s+1]), seq_start has n_seq + 1 ascending entries ending at n_residues.  Windows are
 * numbered the way kmer_search.cpp:64-83 walks them (sequence-major, ascending offset; they do not
 * cross sequence boundaries; sequences shorter than k contribute none), and that number is the DB
 * id every other call reports.  *n_windows receives their count; window_pos (optional, one uint32
 * per window -- call once with NULL to learn the count) receives each window's start position in
 * the buffer.  Replaces the host loop of BuildLSHTalbe(prodb, ...) kmer_search.cpp:64-83 together
 * with the build itself; the index is identical to hs_index_build over the materialised windows. */
HS_API hs_status hs_index_build_windows(hs_handle* h, const uint8_t* residues, uint64_t n_residues,
                                        const uint64_t* seq_start, uint64_t n_seq,
                                        uint64_t* n_windows, uint32_t* window_pos);
/* SURVEY 8(e), "Index build" row -- the build loop of Search() (motif_both_points.cpp:212-218) with the
 * evaluation of the hash functions SPREAD OVER RANKS (one handle per rank = GPU).  The index is replicated,
 * so every rank is given all n k-mers; rank r evaluates the L x K functions for its contiguous block of
 * them only (hs_shard_bounds' rule: *block_lo, *block_count), the ranks all-gather 8-byte fingerprints,
 * every rank groups all of them, and the exact HashKey-string membership proof of a k-mer is made by the
 * rank that hashed it, against the bucket's tuple -- the bucket ints of the bucket's first member,
 * contributed by the rank that hashed THAT k-mer.  The caller does the collectives (RCCL, or anything
 * else); every pointer with a d_ prefix is device memory of the handle's GPU.  Per table l = 0 .. L-1:
 *   hs_index_shard_hash_dev(h, l, seed, d_fp_block[block_count])     fingerprints of the rank's block
 *   <all-gather: d_fp_all[n], blocks in rank order>
 *   hs_index_shard_group_dev(h, l, d_fp_all, &nb)                    the table's buckets: nb of them
 *   hs_index_shard_tuples_dev(h, l, d_tuples[nb][K])                 zeros but for the buckets whose first
 *                                                                    member lies in the rank's block
 *   <sum over ranks (all-reduce): d_tuples_all[nb][K]>
 *   hs_index_shard_finish_dev(h, l, d_tuples_all, &collided)         proof of the own block, bucket-ordered copies
 * and after the last table <max over ranks of collided over all tables>: if set (two HashKey strings
 * under one fingerprint), start over from table 0 with seed + 1 (hs_index_build tries seeds 0..3); else
 * hs_index_shard_end(h, seed).  The index equals hs_index_build's bit for bit (same file from
 * hs_index_save).
 * STREAMS: every one of these calls works on the handle's own stream and returns with it drained.  A d_
 * buffer the caller fills between two calls (the gathered fingerprints, the summed tuples: outputs of the
 * caller's collectives on the caller's stream) must be COMPLETE when it is handed over -- drain that stream,
 * or record an event behind the collective and pass it to hs_wait_event(h, event) before the call; buffers
 * the library writes (d_fp_block, d_tuples) are complete when the call returns. */
HS_API hs_status hs_index_shard_begin(hs_handle* h, const uint8_t* codes, uint64_t n, uint32_t rank,
                                      uint32_t world, uint64_t* block_lo, uint64_t* block_count);
HS_API hs_status hs_index_shard_hash_dev(hs_handle* h, uint32_t l, uint32_t seed, uint64_t* d_fp_block);
HS_API hs_status hs_index_shard_group_dev(hs_handle* h, uint32_t l, const uint64_t* d_fp_all, uint32_t* n_buckets);
HS_API hs_status hs_index_shard_tuples_dev(hs_handle* h, uint32_t l, int32_t* d_tuples);
HS_API hs_status hs_index_shard_finish_dev(hs_handle* h, uint32_t l, const int32_t* d_tuples_all,
                                           uint32_t* collided);
HS_API hs_status hs_index_shard_end(hs_handle* h, uint32_t key_seed);

/* SURVEY 8(f) row 2 -- persistent index (no reference analogue: the reference rebuilds its tables
 * on every run, motif_both_points.cpp:206-218).  hs_index_save writes parameters, planes,
 * coordinate table, residue codes and the L tables (ids + bucket directory) of a built handle;
 * hs_index_load restores them into a handle created with the SAME parameters, planes and table
 * (checked bit for bit, HS_ERR_IO otherwise) and re-derives the bucket-ordered copies on the
 * device: queries then give exactly what they give after hs_index_build.
 * The file carries its payload's length and a 64-bit hash; hs_index_load checks them and, before any
 * kernel indexes with a table, the table's content on the device (ids a permutation of 0..n-1,
 * ascending inside a bucket; boundaries strictly ascending from 0 to n; fingerprints strictly
 * ascending and equal to the fingerprint of the bucket's tuple; bucket sizes recomputed): a corrupt,
 * truncated, stale or hand-edited file yields HS_ERR_IO, never an out-of-bounds access.
 * hs_index_file_check runs the same checks on the HOST (no GPU, no handle): HS_OK or HS_ERR_IO with
 * a message in err. */
HS_API hs_status hs_index_save(hs_handle* h, const char* path);
HS_API hs_status hs_index_load(hs_handle* h, const char* path);
HS_API hs_status hs_index_file_check(const char* path, char* err, uint32_t err_cap);

/* SURVEY 8(f) row 2, second half -- a built (or loaded) index GROWS by a block of m further k-mers, on the
 * device.  After hs_index_append(h, B, m) on a handle whose index holds the k-mers A in id order, the handle is
 * indistinguishable from one on which hs_index_build(h, A ++ B, n + m) was called: the new k-mers take the ids
 * n .. n + m - 1; hs_index_info_get gives the same n, n_buckets, max_bucket and key_seed (device_bytes may differ);
 * hs_index_save writes the same file byte for byte; every other entry point gives the same results.  The
 * handle's settings (multi-probe, bucket partition, options) survive, as they survive a build.
 * What it does NOT do again: no old residue code crosses PCIe, no old k-mer is hashed or sorted.  Bucket ints
 * depend on the k-mer alone and a table is its entries ordered by (fingerprint, id), so per table the block is
 * hashed, fingerprinted under the index's key_seed and grouped as a build groups a table, its buckets are looked
 * up in the old directory, the two sorted directories are merged (an old bucket keeps its tuple: its first member
 * is still its smallest id) and the bucket-ordered arrays are moved once, the block's members behind the old
 * members of their bucket (hsearch_amd/csrc/hs_append.hip).
 * MEMORY: the grown arrays are new allocations that replace the old ones, so the peak extra HBM is one grown
 * copy of the index's arrays plus scratch sized by the block and by one table's directory -- never the build's
 * n-sized hash and sort scratch.
 * FINGERPRINT SEED: if a block bucket's fingerprint equals that of an old bucket, or of another block bucket,
 * under a different HashKey string, the call runs the full build loop over the concatenated codes (already on
 * the device) from seed 0 -- which is what hs_index_build over A ++ B ends with (hs_profile.append_rebuilds = 1).
 * m = 0 is a successful no-op; appending to an index of 0 k-mers equals a build.
 * hs_index_append_dev: d_codes in device memory of the handle's GPU, complete when the call is made.
 * hs_index_append_windows: the windows of further sequences, enumerated as hs_index_build_windows enumerates
 * them; *n_windows and window_pos (optional) cover the APPENDED windows only (positions in `residues`).  The
 * result equals hs_index_build_windows over both residue buffers concatenated with their seq_starts joined.
 * ERRORS detected before anything of the handle changes (the old index goes on answering): an unbuilt index is
 * HS_ERR_STATE; n + m >= 2^31, a residue code outside the alphabet in the block (the _dev form finds it on the
 * device, before any table is touched) and a seq_start that does not ascend are HS_ERR_INVALID.  Any LATER
 * failure (a HIP error, no memory, fingerprints that collide for every seed) leaves the handle WITHOUT an index,
 * as after hs_set_planes: calls return HS_ERR_STATE until the next build or load -- never a half-merged table.
 * hs_profile after the call: ms_hash (block hash + fingerprints), ms_sort (block grouping, match, directory
 * merge), ms_gather (block records, the move, pos_of), ms_total, append_rebuilds, append_new_buckets. */
HS_API hs_status hs_index_append(hs_handle* h, const uint8_t* codes, uint64_t m);
HS_API hs_status hs_index_append_dev(hs_handle* h, const uint8_t* d_codes, uint64_t m);
HS_API hs_status hs_index_append_windows(hs_handle* h, const uint8_t* residues, uint64_t n_residues,
                                         const uint64_t* seq_start, uint64_t n_seq,
                                         uint64_t* n_windows, uint32_t* window_pos);

/* The same rule for ONE table on the host (no GPU, no handle): the table's four arrays as hs_index_save writes
 * them (ids [n], dir_key [nb], dir_start [nb + 1], dir_tuple [nb][K]; fingerprint seed `seed`) merged with the
 * bucket ints block_ints [m][K] of m appended k-mers (ids n .. n + m - 1) into out_ids [n + m] and the directory
 * out_dir_key [*nb_out], out_dir_start [*nb_out + 1], out_dir_tuple [*nb_out][K].  The directory follows the
 * two-call capacity pattern: *nb_out <= nb + m is always set; dir_cap < *nb_out gives HS_ERR_CAPACITY with nothing
 * written.  *collided = 1 (HS_OK, nothing written): one fingerprint under two HashKey strings, inside the block or
 * between the block and the table -- the caller rebuilds under another seed.  An input table that breaks the
 * content rules of hs_index_file_check is HS_ERR_INVALID (the collision verdict comes first: a directory key that
 * equals a block fingerprint under another tuple is a collision, whatever else it is). */
HS_API hs_status hs_index_table_append(const uint32_t* ids, const uint64_t* dir_key, const uint32_t* dir_start,
                                       const int32_t* dir_tuple, uint64_t n, uint64_t nb,
                                       const int32_t* block_ints, uint64_t m, uint32_t K, uint32_t seed,
                                       uint32_t* out_ids, uint64_t* out_dir_key, uint32_t* out_dir_start,
                                       int32_t* out_dir_tuple, uint64_t dir_cap, uint64_t* nb_out, uint32_t* collided);

/* The other half of hs_index_append -- a built (or loaded) index SHRINKS by a set D of its ids, on the device.
 * After hs_index_remove(h, D, m, new_id) on a handle whose index holds codes[0..n), the handle is indistinguishable
 * from one on which hs_index_build ran over the surviving rows in their old order: the survivors take the ids
 * 0 .. n' - 1 (n' = n - |D|); hs_index_info_get gives the same n, n_buckets, max_bucket and key_seed (device_bytes
 * may differ); hs_index_save writes the same file byte for byte; every other entry point gives the same results.
 * The handle's settings (multi-probe, bucket partition, options) survive, as they survive an append.  A bucket that
 * loses all its members disappears; removing every k-mer gives what hs_index_build(h, codes, 0) gives.
 * What it does NOT do again: no residue code crosses PCIe, no surviving k-mer is hashed, sorted or gathered.  A
 * table is its entries ordered by (fingerprint, id) and removal keeps that order, so per table the bucket-ordered
 * arrays and the directory are stream-compacted under 64-bit keep masks (hsearch_amd/csrc/hs_remove.hip).
 * TUPLES: a bucket's tuple is the bucket ints of its member with the smallest id, and the members of a bucket share
 * the HashKey string, not always the ints ((1,23) and (12,3)).  Where a bucket's first member goes and others stay,
 * the tuple becomes the bucket ints of the new first member: just those k-mers are hashed again, with that table's
 * functions.  Every other tuple is copied; the fingerprint belongs to the string and never changes.
 * FINGERPRINT SEED: with key_seed 0 the remainder, a subset, cannot collide under seed 0 either, and the result has
 * seed 0.  With key_seed s > 0 the build over the remainder may end at any seed <= s: the call then runs the full
 * build loop from seed 0 over the compacted codes, already on the device (hs_profile.remove_rebuilds = 1).
 * ids: any order, duplicates allowed.  new_id (optional, [n] of the OLD n): each old id's new id, or 0xffffffff for
 * a removed one -- what a caller renumbers its own side tables with, id_start of hs_seq_match included.  m = 0 is a
 * successful no-op, and new_id is then the identity.
 * hs_index_remove_dev: d_ids and d_new_id in device memory of the handle's GPU, d_ids complete when the call is made.
 * hs_index_remove_ranges: the ids [first[r], first[r] + count[r]) of n_ranges ranges (host arrays; ranges may
 * overlap), marked on the device: whole sequences of an index built by hs_index_build_windows go without their ids
 * being written out (hs_window_id_start gives the boundaries).  new_id is host memory.
 * MEMORY: the shrunken arrays are new allocations that replace the old ones, so the peak extra HBM is one shrunken
 * copy of the index's arrays plus scratch: 4 n bytes for new_id, n / 8 bytes for the dead bitmap, 32 bytes per 64
 * entries for masks, counts and scans (id order and one table), and one table's directory -- never the build's
 * n-sized bucket ints, fingerprints and sort buffers (but for the seed fall-back, which is a build).
 * ERRORS detected before anything of the handle changes (the old index goes on answering): an unbuilt index is
 * HS_ERR_STATE; an id >= n (the _dev form finds it on the device, with one read-back) or a range that ends beyond n
 * is HS_ERR_INVALID.  Any LATER failure (a HIP error, no memory) leaves the handle WITHOUT an index, as after a
 * failed append: calls return HS_ERR_STATE until the next build or load -- never a half-compacted table.
 * hs_profile after the call: ms_hash (the re-hash of new first members), ms_sort (masks and the directory),
 * ms_gather (the move, pos_of), ms_total, remove_rebuilds, remove_dead_buckets, remove_retupled. */
HS_API hs_status hs_index_remove(hs_handle* h, const uint32_t* ids, uint64_t m, uint32_t* new_id);
HS_API hs_status hs_index_remove_dev(hs_handle* h, const uint32_t* d_ids, uint64_t m, uint32_t* d_new_id);
HS_API hs_status hs_index_remove_ranges(hs_handle* h, const uint64_t* first, const uint64_t* count, uint64_t n_ranges,
                                        uint32_t* new_id);

/* The same rule for ONE table on the host (no GPU, no handle): the table's four arrays as hs_index_save writes
 * them (fingerprint seed `seed`) without the m ids dead_ids (any order, duplicates allowed), into out_ids [*n_out]
 * (room for n) and the directory out_dir_key [*nb_out], out_dir_start [*nb_out + 1], out_dir_tuple [*nb_out][K].
 * ints [n][K] are bucket ints indexed by OLD id; only the rows of k-mers that become the first member of a bucket
 * are read (null is accepted where there is none).  The directory follows the two-call capacity pattern: *n_out and
 * *nb_out <= nb are always set; dir_cap < *nb_out gives HS_ERR_CAPACITY with nothing written.  An id >= n, or an
 * input table that breaks the content rules of hs_index_file_check, is HS_ERR_INVALID. */
HS_API hs_status hs_index_table_remove(const uint32_t* ids, const uint64_t* dir_key, const uint32_t* dir_start,
                                       const int32_t* dir_tuple, uint64_t n, uint64_t nb, const uint32_t* dead_ids,
                                       uint64_t m, const int32_t* ints, uint32_t K, uint32_t seed, uint32_t* out_ids,
                                       uint64_t* out_dir_key, uint32_t* out_dir_start, int32_t* out_dir_tuple,
                                       uint64_t dir_cap, uint64_t* n_out, uint64_t* nb_out);

/* SURVEY 8(f) row 3 -- Kernel-LSH pre-grouping of whole proteins (pcluster.cpp:11-81).
 * hs_klsh_draw_planes: the planes KLSH::KLSH draws (lsh.cpp:17-38) from its default-seeded
 * std::default_random_engine (lsh.hpp:49) -- per bit t ~ U(-1,1), b ~ U(0, 2 pi), then `feat`
 * normals with standard deviation sigma*sigma (sic, lsh.cpp:22).  Host only; w[bits][feat].
 * hs_klsh_codes: one hash code per sequence of a concatenated buffer of reduced-alphabet classes
 * (0..7 per residue, include/hs_tables.h HS_REDUCED_CLASS): feature vector = counts of the
 * sequence's 3-mers (pcluster.cpp:27-33), bit i = (cos(Dot(p, w_i) + b_i) + t_i >= 0) with Dot
 * strictly left to right in fp64 (KLSH::GetHashValue lsh.cpp:40-49).  Sequences shorter than 3 get
 * HS_KLSH_NONE (the reference skips them, pcluster.cpp:22-24).  uncertain (optional, [n_seq])
 * receives a mask of the bits whose |cos(.) + t| is below 1e-9, i.e. where the device's cos and
 * libm's could disagree on the sign.  Runs on `device`; status only (no handle): err, if given,
 * receives a message. */
#define HS_KLSH_NONE 0xffffffffffffffffull
HS_API hs_status hs_klsh_draw_planes(uint32_t feat, uint32_t bits, double sigma, double* w, double* b,
                                     double* t);
HS_API hs_status hs_klsh_codes(int device, const uint8_t* classes, uint64_t n_residues,
                               const uint64_t* seq_start, uint64_t n_seq, const double* w,
                               const double* b, const double* t, uint32_t bits, uint64_t* codes,
                               uint64_t* uncertain, char* err, uint32_t err_cap);

HS_API hs_status hs_index_info_get(const hs_handle* h, hs_index_info* out);

/* ---- query = probe + dedupe + verify (rows a8, a9, a10) ---------------------------------------- */

/* Replaces the query loop of Search() (motif_both_points.cpp:224-245).  centers[nq][d] are
 * arbitrary points of R^d.  A hit is (query, DB id, table of first sight, sqrt(d2)) with
 * d2 = sum (x_i - c_i)^2 evaluated left to right in fp64 (motif_both_points.cpp:176-183) and
 * d2 <= R*R (:239).  Hits are returned in the reference's output order: query, then table of
 * first sight, then ascending DB id.  cand[nq][L] (may be NULL) receives |B_l(q)|. */
HS_API hs_status hs_query(hs_handle* h, const double* centers, uint64_t nq, double R,
                          uint32_t* hit_q, uint32_t* hit_id, uint32_t* hit_table, double* hit_dist,
                          uint64_t cap, uint64_t* n_hits, uint64_t* cand);
/* Same with every pointer except n_hits in device memory (HBM-resident queries and hits).
 * STREAMS (this and every other _dev entry point): the library works on the handle's own stream.  d_centers
 * must be complete when the call is made (the caller's producer stream drained, or an event recorded behind
 * the producer handed to hs_wait_event(h, event) first); the call returns with the library's stream drained,
 * so the outputs are complete and the inputs may be reused at once, from any stream. */
HS_API hs_status hs_query_dev(hs_handle* h, const double* d_centers, uint64_t nq, double R,
                              uint32_t* d_hit_q, uint32_t* d_hit_id, uint32_t* d_hit_table,
                              double* d_hit_dist, uint64_t cap, uint64_t* n_hits,
                              uint64_t* d_cand);

/* The same search for queries that ARE k-mers -- the usual centres of the reference's own pipeline:
 * hclust2 embeds k-mer strings (KmerToCoordinates, hclust2.cpp:49-62) and `motif_both_points -c`
 * is fed k-mers embedded exactly from the table -- given as residue codes qcodes[nq][k] (rows of the
 * coordinate table, like the DB's): k bytes per query across PCIe instead of 8d = 64 k.  Results are
 * those of hs_query on the embedded codes, bit for bit (hash, filter rows and the exact fp64 distance
 * all read the table rows an embedded centre would hold).  A code outside the alphabet is
 * HS_ERR_INVALID.  hs_query_codes_dev: every pointer except n_hits in device memory. */
HS_API hs_status hs_query_codes(hs_handle* h, const uint8_t* qcodes, uint64_t nq, double R,
                                uint32_t* hit_q, uint32_t* hit_id, uint32_t* hit_table, double* hit_dist,
                                uint64_t cap, uint64_t* n_hits, uint64_t* cand);
HS_API hs_status hs_query_codes_dev(hs_handle* h, const uint8_t* d_qcodes, uint64_t nq, double R,
                                    uint32_t* d_hit_q, uint32_t* d_hit_id, uint32_t* d_hit_table,
                                    double* d_hit_dist, uint64_t cap, uint64_t* n_hits,
                                    uint64_t* d_cand);

/* The merge step of the TABLE-partitioned multi-GPU layout (hsearch_dist.h hs_comm_query_tables): every rank
 * holds some of the L tables over ALL k-mers and answers ALL queries, so a (query, id) pair is reported by
 * every rank whose tables hold the id in the query's bucket, each time with the smallest of that rank's
 * tables (in GLOBAL table numbers).  The reference reports an id in the FIRST table whose probed bucket
 * holds it and never looks at it again (label[], motif_both_points.cpp:232-238); whether it is a hit does not
 * depend on the table.  So of the n gathered tuples the one with the smallest table per (query, id) is the
 * reference's line: this call keeps exactly those, ordered by (query, table, id) -- the reference's file
 * order -- in place in the first *n_out entries of the four device arrays.  q < 2^27, table < 32. */
HS_API hs_status hs_merge_first_table_dev(hs_handle* h, uint32_t* d_q, uint32_t* d_id, uint32_t* d_table,
                                          double* d_dist, uint64_t n, uint64_t* n_out);

/* ---- per-query radii ------------------------------------------------------------------------------ */

/* A search in which every centre has its own radius (the centroids of motif families are not equally tight:
 * hclust.cpp keeps cluster.radius per cluster).  Exactly one of centers [nq][d] / qcodes [nq][k] is non-NULL;
 * radii [nq].
 *
 * Contract: the output is the concatenation, for q = 0 .. nq-1, of what the scalar call (hs_query /
 * hs_query_codes / hs_bruteforce) returns for query q alone at R = radii[q], with hit_q = q; cand[q][l]
 * likewise.  So: the hit test is d2 <= radii[q] * radii[q] in fp64 with the product rounded once (brute force:
 * !(sqrt(d2) > radii[q])), the order is (query, table of first sight, id), distances are bit-identical, a
 * negative radius behaves as it does in the scalar call, the handle's multi-probe setting and bucket partition
 * apply as they do to the scalar call, and recognised k-mer centres and queries given as codes give the same
 * bits as embedded points.  A NaN radius anywhere in the call is HS_ERR_INVALID -- for the _dev form detected on
 * the device -- before any output is written.  Capacity follows the two-call pattern of hs_query.
 *
 * One call joins every bucket's members against ALL the queries that probe it, whatever their radii: the join
 * kernels never see a radius (it lives in each query row's gamma, in the refinement's |c|^2 - R^2 slot and in
 * the fp16 row's last column); the streaming / brute-force filters and the exact decision read radii[q].  What
 * is decided per CALL -- 8-column rows (HS_OPT_WIDE_ROWS), the join's legality, the digit bound of -gamma -- is
 * decided from the largest |radii[q]|, the conservative side of each rule.  The scalar entry points run as
 * before, launch for launch. */
HS_API hs_status hs_query_radii(hs_handle* h, const double* centers, const uint8_t* qcodes, uint64_t nq,
                                const double* radii, uint32_t* hit_q, uint32_t* hit_id, uint32_t* hit_table,
                                double* hit_dist, uint64_t cap, uint64_t* n_hits, uint64_t* cand);
/* ... all pointers device pointers (n_hits: host); one small reduction over d_radii and one read-back per call */
HS_API hs_status hs_query_radii_dev(hs_handle* h, const double* d_centers, const uint8_t* d_qcodes, uint64_t nq,
                                    const double* d_radii, uint32_t* d_hit_q, uint32_t* d_hit_id,
                                    uint32_t* d_hit_table, double* d_hit_dist, uint64_t cap, uint64_t* n_hits,
                                    uint64_t* d_cand);
/* hs_bruteforce with radii [nq] */
HS_API hs_status hs_bruteforce_radii(hs_handle* h, const double* centers, uint64_t nq, const double* radii,
                                     uint32_t* hit_q, uint32_t* hit_id, double* hit_dist, uint64_t cap,
                                     uint64_t* n_hits);

/* ---- nearest centre of every DB k-mer (annotation) ------------------------------------------------- */

/* Which centre does every DB k-mer belong to: what kmer_search.cpp's Search() accumulates in `matches`
 * (:90, :113-121), reduced on the device instead of from the hit list.  Exactly one of centers [nq][d] /
 * qcodes [nq][k] is non-NULL; radii == NULL: every query is searched at R; else radii [nq] and R is ignored.
 *
 * Contract: let H be the hit list hs_query / hs_query_codes (radii == NULL) or hs_query_radii returns for the same
 * arguments on the same handle -- so the handle's multi-probe setting and bucket partition apply as they do there,
 * and recognised k-mer centres and queries given as codes give the same bits as embedded points.  The output has one
 * row per distinct id of H: the hit of H with that id that is smallest under (dist, table, q), dist compared as
 * doubles, table and q as integers -- tables ascending, centres ascending within a table, replaced only by a
 * strictly smaller distance.  Rows are in ascending id; out_dist is bit-identical to that hit's hit_dist.
 * A NaN radius, a query code outside the alphabet, an unbuilt index and nq >= 2^27 are errors exactly as in the
 * underlying call, reported before any output is written.  Capacity follows the two-call pattern, and
 * *n_out <= n (the index's k-mers) always: buffers sized once at n hold every call's result.
 *
 * The hit list is never materialised across the call's batches nor ordered per query: every batch's exact hits are
 * reduced where they lie, into state of the handle that is sized by the index (16 bytes per DB k-mer plus the list of
 * the ids touched), and the call's cost beyond the search grows with the hits and the touched ids, never with n.
 * hs_query* calls run as before, launch for launch. */
HS_API hs_status hs_annotate(hs_handle* h, const double* centers, const uint8_t* qcodes, uint64_t nq, double R,
                             const double* radii, uint32_t* out_id, uint32_t* out_q, uint32_t* out_table,
                             double* out_dist, uint64_t cap, uint64_t* n_out);
/* ... every pointer but n_out in device memory (streams: as hs_query_dev); with radii one small reduction over
 * them and one read-back per call, as in hs_query_radii_dev */
HS_API hs_status hs_annotate_dev(hs_handle* h, const double* d_centers, const uint8_t* d_qcodes, uint64_t nq, double R,
                                 const double* d_radii, uint32_t* d_out_id, uint32_t* d_out_q, uint32_t* d_out_table,
                                 double* d_out_dist, uint64_t cap, uint64_t* n_out);
/* The same rule on the host (no GPU, no handle) for ANY concatenation of n tuples in any order -- a raw hit list,
 * several ranks' annotations of their query blocks (query numbers made global first), the parts of a bucket
 * partition: per distinct id the tuple smallest under (dist, table, q), rows in ascending id.  The result does not
 * depend on the order of the input; merging annotations gives the annotation of the union of the hit lists.
 * Capacity as above (*n_out = distinct ids).  The outputs must not overlap the inputs. */
HS_API hs_status hs_merge_best(const uint32_t* id, const uint32_t* q, const uint32_t* table, const double* dist,
                               uint64_t n, uint32_t* out_id, uint32_t* out_q, uint32_t* out_table, double* out_dist,
                               uint64_t cap, uint64_t* n_out);

/* ---- brute force (row a11) ---------------------------------------------------------------------- */

/* Replaces Search() of motif_both_points_noLSH.cpp:36-56: every (q, j) with !(sqrt(d2) > R),
 * query-major, ascending j (the order of the reference's hits file). */
HS_API hs_status hs_bruteforce(hs_handle* h, const double* centers, uint64_t nq, double R,
                               uint32_t* hit_q, uint32_t* hit_id, double* hit_dist, uint64_t cap,
                               uint64_t* n_hits);
/* Exact k nearest DB k-mers per query (ground truth of recall@k; ties by lower id).
 * nn_id[nq][topk], nn_dist2[nq][topk] (squared, fp64 left-to-right). */
HS_API hs_status hs_bruteforce_topk(hs_handle* h, const double* centers, uint64_t nq,
                                    uint32_t topk, uint32_t* nn_id, double* nn_dist2);

/* ---- all-vs-all near-neighbour graph + greedy clustering (row a12) ------------------------------- */

/* Every ordered pair (i, j), i != j, of indexed k-mers that share a bucket in some table and lie
 * within R of each other; edge_table = the first table in which they share a bucket.  Sorted by
 * (i, table, j).  sqrt_test != 0 selects hclust2's test sqrt(d2) <= R (hclust2.cpp:64-71,119-120)
 * instead of Search()'s d2 <= R*R.  This is the bucket-local member x center distance work of
 * Clustering() (hclust2.cpp:107-132) done as one join per table. */
HS_API hs_status hs_self_join(hs_handle* h, double R, int sqrt_test, uint32_t* edge_i,
                              uint32_t* edge_j, uint32_t* edge_table, double* edge_dist,
                              uint64_t cap, uint64_t* n_edges);

/* The same for the indexed k-mers [first, first + count) only (as the `i` side): the shard of one
 * rank when the join of a table is spread over GPUs. */
HS_API hs_status hs_self_join_range(hs_handle* h, uint64_t first, uint64_t count, double R,
                                    int sqrt_test, uint32_t* edge_i, uint32_t* edge_j,
                                    uint32_t* edge_table, double* edge_dist, uint64_t cap,
                                    uint64_t* n_edges);

/* ---- connected components of the near-neighbour graph (single linkage at radius R) ------------------ */

/* The families of the graph the self-join returns, reduced on the device instead of from the edge list (the
 * clustering pcluster's UnionFind was meant for: its clustering step is an empty stub).
 *
 * Contract: let G be the undirected graph on the indexed k-mers 0 .. n-1 whose edges are exactly the pairs
 * hs_self_join(h, R, sqrt_test, ...) returns on the same handle -- the same bucket rule over all L tables, the same
 * exact fp64 test (sqrt_test selects sqrt(d2) <= R or d2 <= R*R), self pairs dropped; the handle's multi-probe
 * setting and bucket partition are ignored, as the self-joins ignore them.  label[i] is the smallest id in i's
 * component of G: label[i] <= i, and label[i] == i for exactly one k-mer per component; *n_components is the number
 * of such i; *n_edges (may be NULL) is what hs_self_join* puts into *n_edges for the same arguments (ORDERED pairs).
 * The result is a pure function of the index, R and sqrt_test: batch sizes, filter paths, options and the order in
 * which the device happens to unite the pairs do not show in it.
 * hs_components_range: the labels, over all n vertices, of the subgraph whose edges are those
 * hs_self_join_range(first, count) returns; a k-mer without such an edge labels itself.  It is one rank's share
 * when the i side is cut in blocks, and hs_components_merge joins the shares.
 * Errors as in hs_self_join_range: an unbuilt index is HS_ERR_STATE, a range outside the index HS_ERR_INVALID.
 * There is no capacity protocol: the output is always n labels.
 *
 * The edge list is never materialised, ordered per query or copied to the host: every batch's exact pairs are
 * united where they lie, in a union-find forest of the handle that takes 4 bytes per indexed k-mer and nothing
 * per edge (allocated by the first such call, kept with the handle).  n labels cross PCIe (none for the _dev
 * forms).  hs_self_join*, hs_query*, hs_annotate* and hs_clustering* run as before, launch for launch. */
HS_API hs_status hs_components(hs_handle* h, double R, int sqrt_test, uint32_t* label, uint64_t* n_components,
                               uint64_t* n_edges);
HS_API hs_status hs_components_range(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test,
                                     uint32_t* label, uint64_t* n_components, uint64_t* n_edges);
/* ... d_label [n] in device memory, the counts on the host (streams: as hs_query_dev) */
HS_API hs_status hs_components_dev(hs_handle* h, double R, int sqrt_test, uint32_t* d_label, uint64_t* n_components,
                                   uint64_t* n_edges);
HS_API hs_status hs_components_range_dev(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test,
                                         uint32_t* d_label, uint64_t* n_components, uint64_t* n_edges);
/* The merge of such shares on the host (no GPU, no handle).  labels [m][n]: m label arrays over the same n
 * vertices, each a forest given by its labels; out_label [n]: the labels (smallest id per component) of the union
 * of the m forests.  Merging the shares of any partition of 0 .. n-1 into ranges gives hs_components' labels.
 * The result does not depend on the order of the m arrays; the merge is idempotent and m = 1 returns its input
 * (m = 0: every vertex labels itself).  An input with label[i] > i or label[label[i]] != label[i] is
 * HS_ERR_INVALID, reported before anything is written.  out_label may be one of the inputs. */
HS_API hs_status hs_components_merge(const uint32_t* labels, uint64_t m, uint64_t n, uint32_t* out_label,
                                     uint64_t* n_components);

/* ---- density clusters of the near-neighbour graph (DBSCAN at radius R) ------------------------------- */

/* Single linkage chains: one stray k-mer within R of two families fuses them.  DBSCAN lets only k-mers with at
 * least min_pts neighbours join clusters together; sparse k-mers attach to a cluster or are noise.
 *
 * Contract: let G be the graph of hs_self_join(h, R, sqrt_test, ...) on the same handle, as in hs_components -- the
 * same bucket rule over all L tables, the same exact fp64 test, self pairs dropped; the handle's multi-probe setting
 * and bucket partition are ignored, as the self-joins ignore them.
 *   degree[i]  the number of distinct j != i adjacent to i: the density of i at radius R, what one looks at to
 *              choose min_pts and R.  The degrees sum to the self-join's *n_edges (ORDERED pairs).
 *   core       i is core iff degree[i] + 1 >= min_pts (the point counts itself, as in Ester et al. 1996).
 *              min_pts >= 1; 0 is HS_ERR_INVALID.
 *   cluster    a connected component of the subgraph induced on the core vertices; its label is its smallest core
 *              id, so label[i] <= i for a core i.
 *   border     a non-core vertex with at least one core neighbour.  It takes the label of its core neighbour with
 *              the SMALLEST ID.  Classical DBSCAN leaves this choice to the visiting order; this rule does not
 *              depend on any order and costs one 32-bit atomic min per pair.  ("The smallest adjacent cluster
 *              label" would need a third pass over the edges -- a third more time for a choice as arbitrary.)
 *   noise      every other vertex: label[i] = HS_NOISE.
 * The result is a pure function of the index, R, sqrt_test and min_pts.  min_pts = 1 gives exactly hs_components'
 * labels; min_pts = 2 gives them with the singletons turned into noise.
 *
 * hs_degrees_range: degree [n], non-zero only for i in [first, first + count) -- the `i` side of
 * hs_self_join_range; the shares of a partition add up to hs_degrees.  *n_edges (may be NULL) as in hs_components.
 * hs_dbscan: label [n], degree [n] (may be NULL), *out the counts: n_core + n_border + n_noise = n, and n_edges is
 * the self-join's.  Errors as in hs_components: an unbuilt index is HS_ERR_STATE; a NaN R, a
 * range outside the index and min_pts = 0 are HS_ERR_INVALID; the counts are zeroed first.  There is no capacity
 * protocol: the outputs are always n words.
 *
 * Nothing per edge is kept or copied: hs_degrees is one self-join whose batches' pairs are counted where they lie,
 * hs_dbscan a second one with the same arguments that unites the cores and finds the anchors, in state of the
 * handle that takes 12 bytes per indexed k-mer (allocated by the first such call, kept with the handle).
 * hs_self_join*, hs_components*, hs_query* and hs_annotate* run as before, launch for launch. */
#define HS_NOISE 0xffffffffu
typedef struct hs_dbscan_counts {
  uint64_t n_clusters, n_core, n_border, n_noise, n_edges;
} hs_dbscan_counts;
HS_API hs_status hs_degrees(hs_handle* h, double R, int sqrt_test, uint32_t* degree, uint64_t* n_edges);
HS_API hs_status hs_degrees_range(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test,
                                  uint32_t* degree, uint64_t* n_edges);
HS_API hs_status hs_dbscan(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* label, uint32_t* degree,
                           hs_dbscan_counts* out);
/* ... d_degree / d_label [n] in device memory, the counts on the host (streams: as hs_query_dev) */
HS_API hs_status hs_degrees_dev(hs_handle* h, double R, int sqrt_test, uint32_t* d_degree, uint64_t* n_edges);
HS_API hs_status hs_degrees_range_dev(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test,
                                      uint32_t* d_degree, uint64_t* n_edges);
HS_API hs_status hs_dbscan_dev(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* d_label,
                               uint32_t* d_degree, hs_dbscan_counts* out);
/* The same rule on the host (no GPU, no handle) for ANY list of n_edges pairs (ei[t], ej[t]) over the vertices
 * 0 .. n-1: a pair may appear in either or both directions, repeated, and in any order; self pairs are ignored.  The
 * graph is the set of unordered pairs, the degree counts distinct neighbours, and out->n_edges is the sum of the
 * degrees (twice the distinct unordered pairs).  An id >= n is HS_ERR_INVALID, reported before anything is written;
 * so are min_pts = 0 and a NULL label (n > 0) or out.  This is the multi-GPU route: gather the ranks'
 * hs_self_join_range edges, then call it. */
HS_API hs_status hs_dbscan_edges(const uint32_t* ei, const uint32_t* ej, uint64_t n_edges, uint64_t n,
                                 uint32_t min_pts, uint32_t* label, uint32_t* degree, hs_dbscan_counts* out);

/* ---- single-linkage tree: the minimum spanning forest of the near-neighbour graph ---------------------------- */

/* hs_components answers at ONE radius.  The minimum spanning forest (MSF) of the graph at radius R is the single-
 * linkage dendrogram up to R: at most n - 1 edges, and cutting it at any r <= R gives the components at r, so one call
 * replaces a ladder of hs_components calls and says at which distance two families merge.
 *
 * Contract: let G be the graph of hs_self_join(h, R, sqrt_test, ...) on the same handle, as in hs_components -- the
 * same bucket rule over all L tables, the same exact fp64 test, self pairs dropped; the handle's multi-probe setting
 * and bucket partition are ignored.  The WEIGHT of {a, b} is the edge_dist the self-join reports for the pair.  It is
 * the same bits in both directions: every term (x_t - c_t)^2 is symmetric in IEEE arithmetic and the summation order
 * over t is the same.  Edges are totally ordered by (dist as a double, lo, hi) with lo < hi; under a strict total
 * order the MSF is unique, so the result is a pure function of the index, R and sqrt_test: batch sizes, filter paths,
 * options and the device's scheduling do not show in it.
 *
 * hs_msf: the n - n_components tree edges in ascending (dist, lo, hi), edge_lo[t] < edge_hi[t]: the merge order of
 * single linkage, the distances the merge heights.  Cutting into c clusters (n_components <= c <= n) is taking the
 * first n - c edges of the list; it needs no function.  Capacity follows the two-call pattern: HS_ERR_CAPACITY with
 * out->n_tree_edges (and the rest of *out) set and nothing else written -- neither the edge arrays nor label, in
 * the _dev form either; the count is at most n - 1, so buffers sized once at n hold every result.  label [n] (may be NULL) is bit for bit what hs_components(h, R, sqrt_test) writes.
 * out->n_graph_edges is hs_self_join's *n_edges (ORDERED pairs); out->rounds the Boruvka rounds that united something
 * (the call makes rounds + 1 passes over the pairs that look for crossing edges; a graph without edges: 0 rounds,
 * one pass); out->resident 1 if the pairs were kept in HBM, 0 if every pass was a self-join.  Errors as in
 * hs_components: an unbuilt index is HS_ERR_STATE, a NaN R HS_ERR_INVALID; *out is zeroed first.
 *
 * The two paths (an option selects a path, never a result).  Re-join: every pass is a self-join whose batches' pairs
 * are reduced where they lie -- no memory per edge, 2 rounds + 1 self-joins.  Resident (the default when it fits):
 * the first self-join also appends every pair once (lo < hi) with its distance bits to a list in HBM, 16 bytes per
 * unordered pair, and all later passes read that list -- one self-join.  HS_OPT_MSF_EDGE_BUDGET bounds the list; a
 * graph that outgrows it drops the list and continues on the re-join path, which the caller sees in out->resident
 * alone.  State of the handle: 56 bytes per indexed k-mer (components, forest, two 64-bit slots per component, the
 * edge list and its sorted copy; allocated by the first such call, kept with the handle).  THE KEPT LIST STAYS WITH
 * THE HANDLE TOO after a resident call returns -- 16 bytes per unordered pair of the last graph, rounded up by the
 * doubling (275 MB for 17 M pairs), at most the budget -- so that the next call grows nothing; it is freed by the
 * next hs_msf that does not end resident (HS_OPT_MSF_EDGE_BUDGET = 0 followed by a call is the way to give it back)
 * and by hs_destroy.
 * Every existing entry point runs as before, launch for launch.
 *
 * hs_msf_edges (host only, no GPU, no handle): the same rule for ANY list of n_edges weighted pairs (ei[t], ej[t],
 * dist[t]) over the vertices 0 .. n-1: a pair may appear in either or both directions, repeated, and in any order;
 * self pairs are ignored.  An id >= n, a NaN or negative distance, and two occurrences of one unordered pair with
 * different distance bits are HS_ERR_INVALID, reported before any output is written.  out->n_graph_edges is twice
 * the distinct unordered pairs; rounds and resident are 0.  This is the multi-GPU route: over the gathered
 * hs_self_join_range edges of the ranks (as with hs_dbscan_edges), or as the MERGE of several ranks' forests --
 * the MSF of a union of MSFs of edge subsets is the MSF of the whole (an edge that is not in the MSF of its subset
 * is the largest of a cycle there, hence of a cycle in the whole, hence in no MSF of the whole under a strict order).
 *
 * hs_msf_cut (host only): label [n] = the smallest id per component of the forest made of the given tree edges with
 * dist <= r.  With sqrt_test != 0 and r <= R the labels of hs_msf's tree cut at r equal hs_components(h, r, 1)
 * exactly: sqrt(d2) <= r is the edge test of both.  With sqrt_test == 0 the equality is only guaranteed for the
 * full forest against hs_components(h, R, 0): d2 <= r*r and sqrt(d2) <= r may differ in the last bit.  An input
 * that is not a forest over 0 .. n-1 (an id >= n, a self pair, a NaN distance, an edge that closes a cycle) or a NaN
 * r is HS_ERR_INVALID. */
typedef struct hs_msf_info {
  uint64_t n_tree_edges, n_components, n_graph_edges; /* n_graph_edges: ordered pairs, = hs_self_join's *n_edges */
  uint32_t rounds, resident;                          /* resident 1: the pairs were kept in HBM, 0: re-joined per pass */
} hs_msf_info;
HS_API hs_status hs_msf(hs_handle* h, double R, int sqrt_test, uint32_t* edge_lo, uint32_t* edge_hi, double* edge_dist,
                        uint64_t cap, uint32_t* label, hs_msf_info* out);
/* ... the arrays in device memory, *out on the host (streams: as hs_query_dev) */
HS_API hs_status hs_msf_dev(hs_handle* h, double R, int sqrt_test, uint32_t* d_edge_lo, uint32_t* d_edge_hi,
                            double* d_edge_dist, uint64_t cap, uint32_t* d_label, hs_msf_info* out);
HS_API hs_status hs_msf_edges(const uint32_t* ei, const uint32_t* ej, const double* dist, uint64_t n_edges, uint64_t n,
                              uint32_t* out_lo, uint32_t* out_hi, double* out_dist, uint64_t cap, uint32_t* label,
                              hs_msf_info* out);
HS_API hs_status hs_msf_cut(const uint32_t* lo, const uint32_t* hi, const double* dist, uint64_t m, uint64_t n,
                            double r, uint32_t* label, uint64_t* n_components);

/* ---- density tree: DBSCAN at every radius up to R (the DBSCAN* hierarchy) ----------------------------------- */

/* hs_dbscan answers at ONE (R, min_pts); choosing R from the degrees is a ladder of hs_dbscan calls at two self-joins
 * each.  The minimum spanning forest under the mutual-reachability distance (Campello, Moulavi, Sander 2013: the tree
 * HDBSCAN is built on) holds the density clusters of every radius r <= R at one min_pts, as hs_msf holds the
 * components of every radius.
 *
 * Contract: let G be the graph of hs_self_join(h, R, sqrt_test, ...) on the same handle, exactly as in hs_components,
 * hs_dbscan and hs_msf -- the same bucket rule over all L tables, the same exact fp64 test, self pairs dropped; the
 * handle's multi-probe setting and bucket partition are ignored.  d{a,b} is the edge_dist the self-join reports, the
 * same bits in both directions (see hs_msf).
 *   core distance     core[i], for min_pts >= 1 (0 is HS_ERR_INVALID).  min_pts == 1: +0.0.  Otherwise the
 *                     (min_pts - 1)-th smallest value of the multiset { d{i,j} : j adjacent to i }, counted WITH
 *                     multiplicity (three neighbours at distance 0 count three times); +infinity if degree[i] <
 *                     min_pts - 1.  So core[i] <= r exactly when i is a core point of hs_dbscan(h, r, 1, min_pts), for
 *                     every r <= R.
 *   mutual reach.     w{a,b} = max(core[a], core[b], d{a,b}), compared as doubles.  A pair with an infinite end is not
 *                     an edge.
 *   density tree      the minimum spanning forest of G under the strict total order (w, lo, hi), lo < hi.  It is
 *                     unique, hence a pure function of the index, R, sqrt_test and min_pts.  It has n_core - n_clusters
 *                     edges (n_core: the k-mers with a finite core distance), returned in ascending (w, lo, hi): the
 *                     merge order, w the merge height.
 *   label [n]         (may be NULL) for a k-mer with a finite core distance the smallest id of its component: bit for
 *                     bit hs_dbscan(h, R, sqrt_test, min_pts)'s label on the core k-mers.  For every other k-mer
 *                     HS_NOISE.  This is DBSCAN*: BORDER K-MERS ARE NOISE.  The border rule of hs_dbscan ("the core
 *                     neighbour with the smallest id") is a choice made per radius -- which neighbours are core, and
 *                     which are within reach, changes with r -- and a tree of merges between core k-mers cannot carry
 *                     it; a caller who wants borders at one r runs hs_dbscan there.
 *   core [n]          (may be NULL) the core distances.
 * min_pts == 1 gives hs_msf's edges, distances and labels bit for bit.
 *
 * hs_core_distance: core [n], *n_core (the finite ones), *n_edges (may be NULL) = hs_self_join's: one self-join.
 * hs_density_tree: capacity follows the two-call pattern exactly as hs_msf -- HS_ERR_CAPACITY with *out set and
 * nothing else written (neither edges nor label nor core, in the _dev form either); buffers sized once at n hold every
 * result.  Errors as in hs_dbscan / hs_msf: an unbuilt index is HS_ERR_STATE, a NaN R or min_pts == 0 HS_ERR_INVALID;
 * *out is zeroed first.  out->rounds as in hs_msf; out->self_joins the passes that ran the join.
 *
 * The passes.  core[b] of a later batch is unknown while an earlier one is reduced, so the core distances take a
 * self-join of their own; then hs_msf's rounds run on w.  Resident (the default when it fits): that first self-join
 * also keeps every pair once with its RAW distance, 16 bytes per unordered pair, and every later pass reads the list:
 * 1 self-join.  Re-join: 1 + 1 + 2 rounds self-joins (the core pass, the first look for crossing pairs, two per
 * round).  HS_OPT_MSF_EDGE_BUDGET governs the list as it does for hs_msf, and a list that outgrows it falls back to
 * re-joining, visible in out->resident and out->self_joins alone.  An option selects a path, never a result.
 * State of the handle: hs_msf's 56 bytes per indexed k-mer and 28 more (core distance, threshold and round minimum as
 * 64-bit words, a 32-bit count), allocated by the first such call and kept with the handle; the kept list as hs_msf.
 * Every existing entry point runs as before, launch for launch.
 *
 * hs_density_tree_edges (host only, no GPU, no handle): the same rule for ANY list of weighted pairs over the vertices
 * 0 .. n-1.  It accepts what hs_msf_edges accepts -- either or both directions of a pair, repeats, any order, self
 * pairs ignored -- and rejects what it rejects: an id >= n, a NaN or negative distance, two occurrences of one
 * unordered pair with different bits, and min_pts == 0 are HS_ERR_INVALID, reported before anything is written.
 * A distance of -0.0 is read as +0.0 (so -0.0 and +0.0 for one pair do not conflict, and no output carries a sign bit).
 * out->n_graph_edges is twice the distinct unordered pairs; rounds, resident and self_joins are 0.  This is the
 * multi-GPU route, over the gathered hs_self_join_range edges of the ranks.  (Unlike hs_msf_edges it is NOT a merge
 * of forests: core distances need all edges of a vertex.)
 *
 * hs_density_tree_cut (host only): a k-mer with core[i] > r is HS_NOISE (and one without a core distance, +infinity,
 * at every r, r = +infinity included); the rest are labelled with the smallest id
 * per component of the tree edges with w <= r; *n_clusters counts those components.  With sqrt_test != 0 and r <= R
 * the labels of hs_density_tree's tree cut at r equal hs_dbscan(h, r, 1, min_pts)'s on the k-mers that are core at r
 * exactly: sqrt(d2) <= r is the edge test of both.  With sqrt_test == 0 the equality is only guaranteed for the full
 * forest against hs_dbscan(h, R, 0, min_pts): d2 <= r*r and sqrt(d2) <= r may differ in the last bit.  An input that is
 * not a forest over 0 .. n-1 (an id >= n, a self pair, a NaN weight, an edge that closes a cycle), a NaN r, a core
 * entry that is NaN or negative, and a tree edge with w smaller than either end's core distance are HS_ERR_INVALID;
 * label is not written then. */
typedef struct hs_density_info {
  uint64_t n_tree_edges, n_clusters, n_core, n_graph_edges; /* n_graph_edges = hs_self_join's *n_edges */
  uint32_t rounds, resident, self_joins;                     /* self_joins: passes that ran the join */
} hs_density_info;
HS_API hs_status hs_core_distance(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, double* core,
                                  uint64_t* n_core, uint64_t* n_edges);
HS_API hs_status hs_core_distance_dev(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, double* d_core,
                                      uint64_t* n_core, uint64_t* n_edges);
HS_API hs_status hs_density_tree(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* edge_lo,
                                 uint32_t* edge_hi, double* edge_w, uint64_t cap, uint32_t* label, double* core,
                                 hs_density_info* out);
/* ... the arrays in device memory, *out on the host (streams: as hs_query_dev) */
HS_API hs_status hs_density_tree_dev(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* d_edge_lo,
                                     uint32_t* d_edge_hi, double* d_edge_w, uint64_t cap, uint32_t* d_label,
                                     double* d_core, hs_density_info* out);
HS_API hs_status hs_density_tree_edges(const uint32_t* ei, const uint32_t* ej, const double* dist, uint64_t n_edges,
                                       uint64_t n, uint32_t min_pts, uint32_t* out_lo, uint32_t* out_hi, double* out_w,
                                       uint64_t cap, uint32_t* label, double* core, hs_density_info* out);
HS_API hs_status hs_density_tree_cut(const uint32_t* lo, const uint32_t* hi, const double* w, uint64_t m,
                                     const double* core, uint64_t n, double r, uint32_t* label, uint64_t* n_clusters);

/* ---- the topk best hits per query, and the k-nearest-neighbour graph --------------------------------------- */

/* "The N best matches" of every query, selected on the device: the hit list never crosses PCIe and is never ordered
 * as a whole.
 *
 * The rule.  Let H be the hit list of the UNDERLYING CALL on the same handle (named per entry point below).  For a
 * query q, N(q) is the set of hits of H with hit_q == q (each id occurs once).  Row q of the result is the
 * min(topk, |N(q)|) hits of N(q) that are smallest under (dist compared as doubles, id), in ascending order.  Each
 * entry carries the id, the table of first sight exactly as H reports it, and the distance bit-identical to hit_dist.
 * Unused entries of a row are id = 0xffffffff, table = 0xffffffff, dist = +inf (hs_bruteforce_topk's padding).
 * nn_count[q] = |N(q)|: the FULL hit count, which may exceed topk; the counts sum to the underlying call's *n_hits,
 * which is what *n_hits / *n_edges receive.  Ids within a query are distinct and no distance is a NaN or negative, so
 * the order is strict and total and the result is a pure function of the index and the arguments: batch sizes, filter
 * paths, options and scheduling do not show in it.  1 <= topk <= HS_TOPK_MAX (one entry per lane of a wave); anything
 * else is HS_ERR_INVALID.
 *
 * All outputs have fixed shapes -- nn_id, nn_table, nn_dist [rows][topk], nn_count [rows] -- and there is no capacity
 * protocol.  nn_table may be NULL everywhere.
 *
 * hs_query_topk: rows = nq.  Exactly one of centers [nq][d] / qcodes [nq][k] is non-NULL; radii == NULL: every query at
 * R; else radii [nq] and R is ignored (as in hs_annotate).  The underlying call is hs_query / hs_query_codes /
 * hs_query_radii: the handle's multi-probe setting and bucket partition apply as they do there, and recognised k-mer
 * centres and codes give the same bits as points.  Errors are as in the underlying call (a NaN R or radius -- for the
 * _dev form detected on the device --, an unbuilt index, nq >= 2^27) and are reported before any output is written; a
 * query code outside the alphabet is found by the search itself: the host form writes nothing then, the _dev form
 * may have written the rows of earlier batches.
 *
 * hs_self_knn / hs_self_knn_range: the k-nearest-neighbour graph within R.  rows = n, or count with row t = k-mer
 * first + t.  The underlying call is hs_self_join / hs_self_join_range (multi-probe and partition are ignored, as
 * there).  Two identities follow: nn_count == hs_degrees, and for 2 <= m <= topk + 1 nn_dist[i][m - 2] is bit for bit
 * hs_core_distance(h, R, sqrt_test, m)[i] (+inf where the degree is below m - 1).  The shares of a partition of
 * 0 .. n-1 into ranges concatenate to the whole.
 *
 * Every batch's hits are selected where they lie (all hits of one query lie in one batch); the scratch is sized by a
 * batch, never by n.  Every other entry point launches what it launched. */
#define HS_TOPK_MAX 64u
HS_API hs_status hs_query_topk(hs_handle* h, const double* centers, const uint8_t* qcodes, uint64_t nq, double R,
                               const double* radii, uint32_t topk, uint32_t* nn_id, uint32_t* nn_table, double* nn_dist,
                               uint32_t* nn_count, uint64_t* n_hits);
/* ... every pointer but n_hits in device memory (streams: as hs_query_dev) */
HS_API hs_status hs_query_topk_dev(hs_handle* h, const double* d_centers, const uint8_t* d_qcodes, uint64_t nq, double R,
                                   const double* d_radii, uint32_t topk, uint32_t* d_nn_id, uint32_t* d_nn_table,
                                   double* d_nn_dist, uint32_t* d_nn_count, uint64_t* n_hits);
HS_API hs_status hs_self_knn(hs_handle* h, double R, int sqrt_test, uint32_t topk, uint32_t* nn_id, uint32_t* nn_table,
                             double* nn_dist, uint32_t* nn_count, uint64_t* n_edges);
HS_API hs_status hs_self_knn_range(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test,
                                   uint32_t topk, uint32_t* nn_id, uint32_t* nn_table, double* nn_dist,
                                   uint32_t* nn_count, uint64_t* n_edges);
HS_API hs_status hs_self_knn_dev(hs_handle* h, double R, int sqrt_test, uint32_t topk, uint32_t* d_nn_id,
                                 uint32_t* d_nn_table, double* d_nn_dist, uint32_t* d_nn_count, uint64_t* n_edges);
HS_API hs_status hs_self_knn_range_dev(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test,
                                       uint32_t topk, uint32_t* d_nn_id, uint32_t* d_nn_table, double* d_nn_dist,
                                       uint32_t* d_nn_count, uint64_t* n_edges);
/* The same rule on the host (no GPU, no handle) for ANY concatenation of n_tuples (q, id, table, dist) in any order --
 * a raw hit list, the rows of the parts of a bucket or table partition, several ranks' rows (flattened, with q the
 * row number): rows [nq][topk] and nn_count [nq] as above.  Tuples whose id is 0xffffffff are skipped, so padded rows
 * can be fed back in.  Several tuples with one (q, id) count once and keep the smallest table.  Two tuples of one
 * (q, id) with different distance bits, q >= nq, a NaN or negative distance and a topk out of range are
 * HS_ERR_INVALID, reported before anything is written.  -0.0 is read as +0.0.  nn_count[q] is the number of DISTINCT
 * ids given for q: over raw hit lists that is the hit count; over rows that were already cut at topk it is only a
 * LOWER BOUND of it.  The top-k of a union is the top-k of the union of the parts' top-k rows, so merging rows
 * selected with the same topk loses nothing.  table may be NULL: every tuple then carries table 0xffffffff, and that
 * is what nn_table (which may be NULL too, independently) receives.  Outputs must not overlap inputs. */
HS_API hs_status hs_topk_merge(const uint32_t* q, const uint32_t* id, const uint32_t* table, const double* dist,
                               uint64_t n_tuples, uint64_t nq, uint32_t topk, uint32_t* nn_id, uint32_t* nn_table,
                               double* nn_dist, uint32_t* nn_count);

/* ---- hits per (query group, database sequence, diagonal) ---------------------------------------------------- */

/* "Which proteins carry this motif, how often, and where is the best site", and with a protein as the query "which
 * database proteins share runs of similar k-mers with it, and on which diagonal": what kmer_search.cpp's Search()
 * accumulates per protein in `matches` and never reports, reduced on the device.  The hit list never crosses PCIe and
 * is never ordered per query.
 *
 * The underlying hit list.  Exactly one of centers [nq][d] / qcodes [nq][k] is non-NULL; radii == NULL: every query at
 * R; else radii [nq] and R is ignored (as in hs_annotate).  Let H be the hit list hs_query / hs_query_codes (radii ==
 * NULL) or hs_query_radii returns for the same arguments on the same handle: the handle's multi-probe setting and
 * bucket partition apply as they do there, and recognised k-mer centres and codes give the same bits as points.
 *
 * Sequences.  id_start [n_seq + 1] is ascending (equal neighbours allowed: a sequence without ids), id_start[0] == 0
 * and id_start[n_seq] == n, the index's k-mers: sequence s owns the ids [id_start[s], id_start[s + 1]).  It is a
 * statement about ids, so it serves any index; for an index built by hs_index_build_windows, hs_window_id_start
 * computes it from the same seq_start (sequence s has max(0, len_s - k + 1) windows).
 *
 * The key of a hit (q, id): g = q_group[q] (q_group == NULL: g = q, and n_groups must equal nq); s = the sequence
 * that owns id; off = id - id_start[s]; diag = off - q_off[q] (q_off == NULL: no diagonals are kept, diag is 0 for
 * every hit).  The output has ONE ROW PER DISTINCT (g, s, diag) of H, rows ascending in (g, s, diag) with diag
 * compared as the signed difference (out_diag receives its low 32 bits):
 *   out_count                              the number of hits of H with that key
 *   out_best_dist, out_best_q, out_best_id the hit smallest under (dist as double, q, id); the distance is
 *                                          bit-identical to its hit_dist
 *   out_lo, out_hi                         the smallest and the largest off among the row's hits: on a diagonal they
 *                                          bound the run of seeds, without diagonals they span the matches in s
 * *n_hits = the underlying call's *n_hits; the counts sum to it.  Capacity, counted in rows, follows the two-call
 * pattern (HS_ERR_CAPACITY with *n_out set and nothing written; cap = 0 with NULL arrays asks for the count), and
 * *n_out <= *n_hits always.  Every reduction is order-free -- integer sum, min and max on integers and on distance
 * bit patterns; distances are >= +0 and never a NaN -- so the result is a pure function of the index and the
 * arguments: batch sizes, filter paths, options and scheduling do not show in it.
 *
 * Key width, a stated limit of the entry point.  Let wg, ws, wd be the bits needed for n_groups - 1, n_seq - 1 and
 * max_len + max_qoff - 1, where max_len is the largest id count of a sequence and max_qoff the largest q_off (0
 * without q_off); the diagonal is kept as off - q_off + max_qoff.  A call with wg + ws + wd > 64 is HS_ERR_INVALID.
 * What fits, for scale: 5 x 10^7 sequences x 10^3 query proteins x diagonals of 10^5 is 26 + 10 + 17 bits.  n_groups
 * and n_seq are at most 2^32.
 *
 * Errors, reported before any output is written: everything the underlying call rejects (a NaN R or radius, an
 * unbuilt index, nq >= 2^27); an id_start that does not ascend, does not start at 0 or does not end at n; a
 * q_group[q] >= n_groups; the width rule.  The _dev form finds these on the device: one small reduction over q_group /
 * q_off / id_start and one read-back per call, as hs_query_radii_dev does for the radii.  A query code outside the
 * alphabet is found by the search itself, and nothing is written then.  A row that would count more than 2^32 - 1 hits
 * is HS_ERR_CAPACITY.
 *
 * Every batch's exact hits (a multi-probe chunk's merged list likewise) are keyed, sorted and reduced where they lie,
 * and the batch's rows appended to a list of the handle; at the end of a call to which several batches contributed the
 * list is reduced once more.  Scratch is sized by a batch plus the rows found so far: never by n, by n_groups x n_seq
 * or by the call's hits.  Every other entry point launches what it launched. */
HS_API hs_status hs_seq_match(hs_handle* h, const double* centers, const uint8_t* qcodes, uint64_t nq, double R,
                              const double* radii, const uint32_t* q_group, uint64_t n_groups, const uint32_t* q_off,
                              const uint64_t* id_start, uint64_t n_seq, uint32_t* out_group, uint32_t* out_seq,
                              int32_t* out_diag, uint32_t* out_count, double* out_best_dist, uint32_t* out_best_q,
                              uint32_t* out_best_id, uint32_t* out_lo, uint32_t* out_hi, uint64_t cap, uint64_t* n_out,
                              uint64_t* n_hits);
/* ... every pointer but n_out / n_hits in device memory (streams: as hs_query_dev) */
HS_API hs_status hs_seq_match_dev(hs_handle* h, const double* d_centers, const uint8_t* d_qcodes, uint64_t nq, double R,
                                  const double* d_radii, const uint32_t* d_q_group, uint64_t n_groups,
                                  const uint32_t* d_q_off, const uint64_t* d_id_start, uint64_t n_seq,
                                  uint32_t* d_out_group, uint32_t* d_out_seq, int32_t* d_out_diag, uint32_t* d_out_count,
                                  double* d_out_best_dist, uint32_t* d_out_best_q, uint32_t* d_out_best_id,
                                  uint32_t* d_out_lo, uint32_t* d_out_hi, uint64_t cap, uint64_t* n_out,
                                  uint64_t* n_hits);
/* id_start [n_seq + 1] of an index built by hs_index_build_windows over seq_start [n_seq + 1] at k-mer length k (host
 * only): sequence s has max(0, len_s - k + 1) windows, numbered sequence-major.  A seq_start that does not ascend and
 * k == 0 are HS_ERR_INVALID. */
HS_API hs_status hs_window_id_start(const uint64_t* seq_start, uint64_t n_seq, uint32_t k, uint64_t* id_start);
/* The same rule on the host (no GPU, no handle) for ANY list of n_tuples hits (q, id, dist) in any order -- a raw hit
 * list, or the lists of the parts of a table or bucket partition after their first-seen merge: rows and capacity as
 * above.  A (q, id) given several times counts once and must carry one distance (different bits: HS_ERR_INVALID);
 * -0.0 is read as +0.0.  q >= nq, an id >= id_start[n_seq], a NaN or negative distance and every error of the
 * contract above (id_start here only has to ascend from 0) are HS_ERR_INVALID, reported before anything is
 * written.  Outputs must not overlap inputs. */
HS_API hs_status hs_seq_match_hits(const uint32_t* q, const uint32_t* id, const double* dist, uint64_t n_tuples,
                                   uint64_t nq, const uint32_t* q_group, uint64_t n_groups, const uint32_t* q_off,
                                   const uint64_t* id_start, uint64_t n_seq, uint32_t* out_group, uint32_t* out_seq,
                                   int32_t* out_diag, uint32_t* out_count, double* out_best_dist, uint32_t* out_best_q,
                                   uint32_t* out_best_id, uint32_t* out_lo, uint32_t* out_hi, uint64_t cap,
                                   uint64_t* n_out);
/* Rows combined (host only): rows with equal (group, seq, diag) become one -- counts add, best is the min under (dist,
 * q, id), lo the min, hi the max --, rows ascending as above.  Valid ONLY for parts whose hit lists are DISJOINT: the
 * query-block layout, with q (and the groups) made global first.  Parts that can report one (q, id) twice -- the
 * table and bucket partitions -- would count it twice here: their hit lists go through hs_seq_match_hits instead.  A
 * count that would pass 2^32 - 1, a zero count, lo > hi and a NaN or negative distance are HS_ERR_INVALID, reported
 * before anything is written.  Outputs must not overlap inputs. */
HS_API hs_status hs_seq_match_merge(const uint32_t* group, const uint32_t* seq, const int32_t* diag,
                                    const uint32_t* count, const double* best_dist, const uint32_t* best_q,
                                    const uint32_t* best_id, const uint32_t* lo, const uint32_t* hi, uint64_t n_rows,
                                    uint32_t* out_group, uint32_t* out_seq, int32_t* out_diag, uint32_t* out_count,
                                    double* out_best_dist, uint32_t* out_best_q, uint32_t* out_best_id, uint32_t* out_lo,
                                    uint32_t* out_hi, uint64_t cap, uint64_t* n_out);

/* ---- cluster profiles, centroids and covering radii from a label array ------------------------------------ */

/* The step from cluster labels to what a search takes: per cluster its members' position frequency matrix, their
 * centroid (Center(), centerDistanceSmapling.cpp:67-78) and the radius that makes every member a hit of a centre (the
 * reference's cluster.radius, hclust.cpp:217-222), reduced on the device from the index's codes and a label array.
 *
 * Inputs: a built index (n k-mers) and label [n].  label[i] is HS_NOISE or a value < n; the value need not be a
 * member's id nor the smallest one: the labels of hs_components, of hs_dbscan and owner[] of hs_clustering over the
 * same codes are all legal.  Any other value is HS_ERR_INVALID, reported before any output is written (the _dev forms
 * detect it on the device, as hs_query_radii_dev detects a NaN radius).  min_size >= 1; 0 is HS_ERR_INVALID.  An
 * unbuilt index is HS_ERR_STATE.
 *
 * Clusters and rows: a cluster is the set of i with one label value.  The clusters with at least min_size members
 * are the rows of the output, in ascending label value; *n_out is their number.  Capacity, counted in ROWS, follows
 * the two-call pattern (HS_ERR_CAPACITY with *n_out set; cap = 0 with null arrays asks for the count), and
 * *n_out <= n / min_size always.
 *
 * hs_cluster_profile, per row:
 *   out_label, out_size
 *   counts   [row][k][alphabet] uint32 (may be NULL): the number of members with code a at position p
 *   centroid [row][d] fp64: the coordinate p * 8 + c is S / (double)size, where S starts at +0.0 and, for
 *            a = 0 .. alphabet - 1 in ascending order, gains (double)count[p][a] * coords[a][c] -- every product and
 *            every sum rounded to fp64, no contraction into FMA -- and one division follows.
 * This is Center() with the member-order sum replaced by an order-free one: it agrees with hsearch::FamilyCenters
 * only UP TO ROUNDING.  Both lie within gamma_m * M of the exact mean, m = size + alphabet,
 * gamma_m = m 2^-53 / (1 - m 2^-53), M = max |coords|; they differ by at most 2 gamma_m M.
 *
 * hs_cluster_radii: the same labels and min_size plus centers [n_rows][d], any FINITE points -- the profile's
 * centroids, the centroids as a points file holds them (6 significant digits), medoids' embeddings.  (Finite is a
 * decision of this contract: max and min run on the d2 bit patterns, which order like the doubles only where no d2
 * is a NaN.  A NaN or infinite coordinate in a centre leaves that row's max_d2, radius and medoid unspecified and
 * every other row as it is.)  n_rows must be
 * the row count the labels give, else HS_ERR_INVALID.  Per member d2 = sum over t of (x[t] - centre[t])^2, left to
 * right in fp64 (PairwiseDistance_square, and the exact pass of the searches).  Per row:
 *   max_d2   the largest member d2
 *   radius   the smallest double r with r * r >= max_d2: r = sqrt(max_d2) correctly rounded, then the next double up
 *            if r * r < max_d2 (hsearch::RadiusCovering).  With it hs_query_radii's d2 <= r * r and the sqrt tests
 *            both accept the farthest member
 *   medoid   the member smallest under (d2, id), d2 compared as doubles
 * Counts are integers, max and min are order-free: every output is a pure function of (codes, labels, min_size,
 * centres) and bit-reproducible, whatever HS_OPT_SUMMARY_CHUNK / HS_OPT_SUMMARY_ROWS say.
 *
 * State: 36 bytes per indexed k-mer in the handle (28 for hs_cluster_profile alone; allocated by the first such call,
 * kept with the handle, reset at the start of every call), plus at most 32 MB of scratch for the counts of a batch of
 * rows when counts == NULL -- never more, however many rows there are: rows are processed in batches.
 * Every other entry point runs as before, launch for launch; the handle's multi-probe setting and bucket partition
 * play no part here. */
HS_API hs_status hs_cluster_profile(hs_handle* h, const uint32_t* label, uint32_t min_size, uint32_t* out_label,
                                    uint32_t* out_size, uint32_t* counts, double* centroid, uint64_t cap,
                                    uint64_t* n_out);
HS_API hs_status hs_cluster_radii(hs_handle* h, const uint32_t* label, uint32_t min_size, const double* centers,
                                  uint64_t n_rows, double* max_d2, double* radius, uint32_t* medoid);
/* ... every array in device memory, the counts and statuses on the host (streams: as hs_query_dev) */
HS_API hs_status hs_cluster_profile_dev(hs_handle* h, const uint32_t* d_label, uint32_t min_size, uint32_t* d_out_label,
                                        uint32_t* d_out_size, uint32_t* d_counts, double* d_centroid, uint64_t cap,
                                        uint64_t* n_out);
HS_API hs_status hs_cluster_radii_dev(hs_handle* h, const uint32_t* d_label, uint32_t min_size, const double* d_centers,
                                      uint64_t n_rows, double* d_max_d2, double* d_radius, uint32_t* d_medoid);
/* Both rules on the host (no GPU, no handle) for codes [n][k], coords [alphabet][8] (NULL: the default table, alphabet
 * 0 or 20) and label [n]: bit-identical to the device forms.  counts may be NULL; max_d2 / radius / medoid are all
 * given or all NULL (no radii); centers == NULL: the radii are taken against the call's own centroids, else against
 * centers [n_center_rows][d] (n_center_rows must be the row count).  A code >= alphabet, an illegal label, min_size 0,
 * k outside 1 .. 75 are HS_ERR_INVALID, reported before anything is written.  This is the route for label shares
 * gathered from several GPUs. */
HS_API hs_status hs_cluster_summary_codes(const uint8_t* codes, uint64_t n, uint32_t k, const double* coords,
                                          uint32_t alphabet, const uint32_t* label, uint32_t min_size,
                                          const double* centers, uint64_t n_center_rows, uint32_t* out_label,
                                          uint32_t* out_size, uint32_t* counts, double* centroid, double* max_d2,
                                          double* radius, uint32_t* medoid, uint64_t cap, uint64_t* n_out);

/* ---- clusters to weighted, searchable profiles -------------------------------------------------------------- */

/* The step from the clusters the engine discovers to profiles hs_pssm_scan can be given: per row of hs_cluster_profile
 * the position-based sequence weights of its members (so that a family present in hundreds of near-identical copies
 * does not own its cluster's profile) and, for a profile built from them, the threshold that covers the row -- the
 * profile-side counterpart of hs_cluster_radii's covering radius.
 *
 * hs_cluster_weighted_profile.  Rows, out_label, out_size, cap, *n_out, the label rules and every refusal are
 * hs_cluster_profile's (wcounts takes centroid's place among the arrays a call with cap > 0 must give).  Per row:
 *   counts   [row][k][alphabet] uint32 (may be NULL): what hs_cluster_profile gives
 *   wcounts  [row][k][alphabet] uint64: the sum of W(i) over the members i with residue a at position p
 *   wsum     [row] uint64 (may be NULL): the sum of W(i) over the members
 *   distinct [row] uint32 (may be NULL): the sum over p of r[p]
 * under the rule of hs_pssm_weighted_counts with the sites of row r being the members of row r: r[p] = the residues
 * that occur at p, u[p][a] = floor(2^56 / (r[p] counts[p][a])), W(i) = the sum over p of u[p][x_ip].  It is
 * hs_pssm_weight_hits over the tuples (m = row, id = member) without id_start.  Every column of wcounts[row] sums to
 * wsum[row] <= k 2^56.  All sums are integer sums: the result is a pure function of (codes, labels, min_size), whatever
 * HS_OPT_SUMMARY_CHUNK, HS_OPT_SUMMARY_ROWS and the device's scheduling are.
 * How: per batch of rows, behind the profile kernel, one wave per row builds the u tables, and a second pass over the
 * same member slots, items and segments adds every member's weight into uint64 LDS histograms
 * (hsearch_amd/csrc/hs_cluster_pssm.hip).  Scratch: the counts (when counts == NULL) and the tables of a row batch,
 * together at most 32 MB.  hs_profile after the call: summary_weight_rows, summary_weight_items.
 *
 * hs_cluster_pssm_cover.  The same labels and min_size plus profiles S [n_rows][k][alphabet], held to hs_pssm_scan's
 * value checks (a NaN or infinite entry, |S| > 2^100: HS_ERR_INVALID); n_rows must be the row count the labels give,
 * else HS_ERR_INVALID.  Every refusal comes before anything is written; the _dev form finds the value errors on the
 * device with one read-back.  Per row:
 *   min_score  the smallest score of the row's profile over the row's members; the score is hs_pssm_scan's, bit for
 *              bit: from +0.0, left to right in fp64
 *   argmin     the member attaining it, the smallest id among ties
 * THE CONTRACT: hs_pssm_scan(S, t = min_score) returns every member of row r among the hits of profile r -- score >= t
 * on identical bits.
 *
 * hs_cluster_profile and hs_cluster_radii launch exactly what they launched before.  Out of scope: a p-value threshold
 * mode, a device log-odds (hs_pssm_log_odds_weighted stays the host's), multi-GPU drivers (the host rules below are the
 * route for label shares gathered from several GPUs), position-specific pseudo-counts. */
HS_API hs_status hs_cluster_weighted_profile(hs_handle* h, const uint32_t* label, uint32_t min_size,
                                             uint32_t* out_label, uint32_t* out_size, uint32_t* counts,
                                             uint64_t* wcounts, uint64_t* wsum, uint32_t* distinct, uint64_t cap,
                                             uint64_t* n_out);
HS_API hs_status hs_cluster_pssm_cover(hs_handle* h, const uint32_t* label, uint32_t min_size, const double* S,
                                       uint64_t n_rows, double* min_score, uint32_t* argmin);
/* ... every array in device memory, the counts and statuses on the host (streams: as hs_query_dev) */
HS_API hs_status hs_cluster_weighted_profile_dev(hs_handle* h, const uint32_t* d_label, uint32_t min_size,
                                                 uint32_t* d_out_label, uint32_t* d_out_size, uint32_t* d_counts,
                                                 uint64_t* d_wcounts, uint64_t* d_wsum, uint32_t* d_distinct,
                                                 uint64_t cap, uint64_t* n_out);
HS_API hs_status hs_cluster_pssm_cover_dev(hs_handle* h, const uint32_t* d_label, uint32_t min_size, const double* d_S,
                                           uint64_t n_rows, double* d_min_score, uint32_t* d_argmin);
/* Both rules on the host (no GPU, no handle) for codes [n][k] over `alphabet` residues (1 .. 32) and label [n]:
 * bit-identical to the device forms.  A code >= alphabet, an illegal label, min_size 0, k outside 1 .. 75 are
 * HS_ERR_INVALID, reported before anything is written (hs_cluster_weights_codes sets *n_out on HS_ERR_CAPACITY). */
HS_API hs_status hs_cluster_weights_codes(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet,
                                          const uint32_t* label, uint32_t min_size, uint32_t* out_label,
                                          uint32_t* out_size, uint32_t* counts, uint64_t* wcounts, uint64_t* wsum,
                                          uint32_t* distinct, uint64_t cap, uint64_t* n_out);
HS_API hs_status hs_cluster_cover_codes(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet,
                                        const uint32_t* label, uint32_t min_size, const double* S, uint64_t n_rows,
                                        double* min_score, uint32_t* argmin);

/* ---- PSSM scan: every indexed k-mer scored against position-specific score matrices ------------------------- */

/* What a cluster's position frequency matrix (hs_cluster_profile's counts) becomes when it is searched with: a
 * position-specific score matrix -- log-odds per position and residue -- and a threshold per motif, over every k-mer
 * of the index.  A windows index (hs_index_build_windows) makes it a scan of every protein position.  LSH cannot index
 * this score; the scan is exhaustive.
 *
 * Inputs: S [nm][k][alphabet] fp64 (k and alphabet are the handle's), t [nm].  The scan runs over the built or loaded
 * index of the handle; ids are the DB ids of every other call.
 * Hit rule: score(m, x) = the sum over p = 0 .. k-1 of S[m][p][x_p], starting from +0.0, left to right, every sum
 * rounded to fp64.  (m, id) is a hit iff score >= t[m].  hit_score is that double, bit for bit.
 * Order: (m, id) ascending.  cnt [nm] (may be NULL): the hits per profile, valid on HS_OK and on HS_ERR_CAPACITY.
 * Capacity: the two-call pattern of hs_query (HS_ERR_CAPACITY with *n_hits set; cap = 0 with NULL arrays asks for
 * the count).  *n_hits is a uint64 and may exceed 2^32.
 * Errors, reported before any output is written: an unbuilt index is HS_ERR_STATE; nm >= 2^27 is HS_ERR_INVALID; a
 * NaN or infinite entry, an entry with |S| > 2^100, and a NaN or infinite threshold are HS_ERR_INVALID (the _dev form
 * finds these on the device with one read-back, as hs_query_radii_dev finds a NaN radius).  The magnitude cap keeps
 * every partial sum finite: 75 entries of at most 2^100 stay below 2^107, so no score is an infinity or a NaN and
 * `>=` is a total order on what it compares.
 * The handle's multi-probe setting and bucket partition play no part.  The result is a pure function of (codes, S, t):
 * batch sizes (HS_OPT_QUERY_BATCH: profiles per batch here), HS_OPT_PSSM_FILTER and the survivor order on the device
 * do not show in it.
 *
 * How: profiles in batches, each batch one pass over the index's packed codes.  A filter on FP6 MFMA (one-hot k-mer
 * rows times the profiles' entries rounded UP onto the e2m3 grid, hs_pssm_tables below; hsearch_amd/csrc/hs_pssm.hip)
 * passes every pair whose rounded fp64 score can reach t; the exact pass computes the contract's sum for what passed
 * and alone decides.  hs_profile after the call: pssm_pairs, pssm_survivors, pssm_dead, pssm_mfma_steps, hits;
 * ms_verify (tables + filter), ms_finalize (exact pass and ordering), ms_total.  Scratch is sized by a batch and
 * comes from the handle's growable buffers.  Every other entry point runs as before, launch for launch.
 * Out of scope: multi-GPU, an int8 form of the filter.  (Top-N per profile: hs_pssm_topk below; the hits reduced per
 * protein: hs_pssm_seq_scan below.) */
HS_API hs_status hs_pssm_scan(hs_handle* h, const double* S, const double* t, uint64_t nm, uint32_t* hit_m,
                              uint32_t* hit_id, double* hit_score, uint64_t cap, uint64_t* n_hits, uint64_t* cnt);
/* ... every pointer but n_hits in device memory (streams: as hs_query_dev) */
HS_API hs_status hs_pssm_scan_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm, uint32_t* d_hit_m,
                                  uint32_t* d_hit_id, double* d_hit_score, uint64_t cap, uint64_t* n_hits,
                                  uint64_t* d_cnt);
/* The filter's tables on the host (no GPU, no handle), the same bits the device builds: code [nm][k][alphabet] the
 * six-bit e2m3 code of every entry, tau [nm] the threshold on the 1/8 grid (-infinity: the profile passes every k-mer;
 * +infinity: dead), dead [nm].  Any output may be NULL.  THE INVARIANT: for every k-mer x, if the contract's rounded
 * score of x reaches t[m] then the sum over p of decode(code[m][p][x_p]) is >= tau[m]; dead[m] = 1 only if no k-mer
 * can hit.  (A dead or pass-everything profile has all codes 0.)  k outside 1 .. 75, alphabet outside 1 .. 32,
 * nm >= 2^27 and the values hs_pssm_scan refuses are HS_ERR_INVALID, with nothing written. */
HS_API hs_status hs_pssm_tables(const double* S, const double* t, uint64_t nm, uint32_t k, uint32_t alphabet,
                                uint8_t* code, double* tau, uint8_t* dead);

/* ---- PSSM top-N: the topk best k-mers of every profile, without a threshold ------------------------------------- */

/* "Show me the N best sites of each profile": hs_pssm_scan needs a threshold per profile, and log-odds thresholds do
 * not transfer from one motif to the next.  Here the threshold is found on the device and the rows are selected there.
 *
 * Inputs: S [nm][k][alphabet] as for hs_pssm_scan; t_floor [nm], or NULL for no floor (every floor -DBL_MAX);
 * 1 <= topk <= HS_TOPK_MAX.
 * Score: hs_pssm_scan's, bit for bit -- from +0.0, left to right, every sum rounded to fp64.
 * Row m: of the k-mers with score >= t_floor[m], the min(topk, their number) best under (score descending, id
 * ascending).  top_id [nm][topk] padded with 0xffffffff, top_score [nm][topk] padded with -infinity, top_count [nm] =
 * the valid entries of the row = min(topk, number of k-mers at or above the floor) -- deliberately not a hit count.
 * The order is strict and total: a score is never a NaN, an infinity (the 2^100 cap) or -0.0 (the sum starts at +0.0),
 * and ids are distinct (hsearch_amd/csrc/hs_pssm_topk.h states the argument and holds the key transform).
 * Errors, reported before anything is written: hs_pssm_scan's (an unbuilt index is HS_ERR_STATE; nm >= 2^27, a bad
 * entry, a NaN or infinite floor are HS_ERR_INVALID; the _dev form finds the values on the device), topk outside its
 * range, a null output with nm > 0.  n == 0 or nm == 0: padded rows, zero counts.
 * Purity: rows and counts are a pure function of (codes, S, t_floor, topk).  HS_OPT_PSSM_TOPK_SAMPLE, the profile batch
 * (HS_OPT_QUERY_BATCH), HS_OPT_PSSM_FILTER, survivor splits and scheduling do not show in them.
 *
 * How, and why it is exact.  With n_s = min(n, HS_OPT_PSSM_TOPK_SAMPLE), the sample is the k-mers s_j = floor(j * n /
 * n_s), j = 0 .. n_s - 1 (64-bit arithmetic).  t'[m] = the topk-th largest exact score of profile m over the sample,
 * if n_s >= topk.  At least topk k-mers of the index score >= t', so every member of the row scores >= t', ties
 * included: the scan of hs_pssm_scan at
 *   t_used[m] = max(t_floor[m], t'[m])      (t_floor[m] where there is no t')
 * returns a superset of the row, and a wave per profile selects the row from it.  t_used [nm] (may be NULL) is that
 * threshold: a diagnostic, and the one output that DOES depend on the sample size.  No hit list crosses PCIe.
 * Profiles per batch: HS_OPT_QUERY_BATCH if set; else at most 4096 and few enough that batch * topk * n / n_s, the
 * hits to expect, stays within 2^24.  A constant profile ties every k-mer at t': n hits for it, and the right row.
 * hs_profile after the call: the pssm_* fields as after a scan at t_used, pssm_topk_sample, pssm_topk_raised, hits
 * (what the scans returned); ms_hash (sample pass), ms_verify (tables + filter), ms_finalize (exact pass + selection),
 * ms_total.  Every other entry point runs as before, launch for launch.
 * Out of scope: topk above 64, a threshold from the filter's own accumulators, a ladder of growing samples,
 * multi-GPU drivers (hs_pssm_topk_hits is the merge). */
HS_API hs_status hs_pssm_topk(hs_handle* h, const double* S, const double* t_floor, uint64_t nm, uint32_t topk,
                              uint32_t* top_id, double* top_score, uint32_t* top_count, double* t_used);
/* ... every pointer in device memory (streams: as hs_pssm_scan_dev) */
HS_API hs_status hs_pssm_topk_dev(hs_handle* h, const double* d_S, const double* d_t_floor, uint64_t nm, uint32_t topk,
                                  uint32_t* d_top_id, double* d_top_score, uint32_t* d_top_count, double* d_t_used);
/* The same rule on the host (no GPU, no handle) for any list of (m, id, score) tuples: the merge of several GPUs' rows.
 * Tuples with id == 0xffffffff are skipped (padding fed back in is harmless); a repeated (m, id) with the same score
 * bits counts once, with different bits it is HS_ERR_INVALID; a NaN score, m >= nm, topk outside 1 .. HS_TOPK_MAX or a
 * null output with nm > 0 are HS_ERR_INVALID, with nothing written.  top_count[m] = min(topk, distinct ids of m). */
HS_API hs_status hs_pssm_topk_hits(const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                   uint64_t nm, uint32_t topk, uint32_t* top_id, double* top_score,
                                   uint32_t* top_count);

/* ---- PSSM hits per sequence: which proteins carry the motif, how often, and where the best site is ---------------- */

/* hs_pssm_scan answers "which k-mers match this profile"; over a protein database the question is which proteins, and
 * the hit list that answers it through the host is large at the thresholds where it matters.  Here the list is reduced
 * on the device and only the rows cross PCIe.
 *
 * Inputs: S, t, the score and the hit rule are hs_pssm_scan's, bit for bit.  Let H be the hit list hs_pssm_scan returns
 * for the same arguments on the same handle.  id_start [n_seq + 1] follows hs_seq_match's rules: ascending (equal
 * neighbours allowed: a sequence without ids), id_start[0] == 0, id_start[n_seq] == n (hs_window_id_start gives it for
 * a windows index).  Sequence s owns the ids [id_start[s], id_start[s + 1]); an id lying at equal neighbours belongs to
 * the LAST sequence that starts at or below it.
 * Rows: one per distinct (m, s) of H, ascending in (m, s).  out_count: the hits of H with that key (ids are 32-bit, so
 * it fits).  out_best_score, out_best_id: the best hit under (score descending, id ascending) -- hs_pssm_topk's order,
 * through the key transform of hsearch_amd/csrc/hs_pssm_topk.h; the score is the hit's hit_score bit for bit.  out_lo,
 * out_hi: the smallest and the largest id - id_start[s] among the row's hits.
 * Counts: *n_hits is the scan's *n_hits; the row counts sum to it.  cnt [nm] (may be NULL): the hits per profile;
 * seq_cnt [nm] (may be NULL): the rows per profile, the sequences it hits.  Both valid on HS_OK and HS_ERR_CAPACITY.
 * Capacity: counted in ROWS, the two-call pattern: HS_ERR_CAPACITY comes with *n_out set (cap = 0 with NULL arrays
 * asks for the count); *n_out <= *n_hits and *n_out <= nm * n_seq.  hs_pssm_seq_scan writes no row then; the _dev form
 * may have written the rows of the batches that still fitted, as hs_pssm_scan_dev does with hits.
 * Errors, reported before anything is written: everything hs_pssm_scan refuses; a null id_start; an id_start that does
 * not ascend, does not start at 0 or does not end at n; n_seq == 0 with n > 0; n_seq > 2^32.  All HS_ERR_INVALID but
 * the unbuilt index (HS_ERR_STATE).  The _dev form finds the value errors on the device: one small reduction over the
 * profiles, hs_seq_match's over id_start, one read-back.
 * Purity: the rows are a pure function of (codes, S, t, id_start).  The profile batch (HS_OPT_QUERY_BATCH),
 * HS_OPT_PSSM_FILTER, survivor splits and scheduling do not show in them.
 *
 * How (hsearch_amd/csrc/hs_pssm_seq.hip): the scan's batches, tables, filter and exact pass as they are.  Batches are
 * cut by profile and a sequence owns a contiguous id range, so after the scan's own (m, id) sort every row is one
 * contiguous run in output order: the sequence of every hit by a search in id_start, run heads, their scan, a wave-wide
 * segmented scan for the best hit, and the batch's rows written at the call's running offset.  No second sort, no row
 * list on the handle, no merge.  Scratch is sized by a batch's hits and rows.
 * hs_profile after the call: the pssm_* fields as after a scan, pssm_seq_rows, hits; ms_finalize covers the exact
 * pass, the sort and the reduction.  Every other entry point runs as before, launch for launch.
 * Out of scope: top-N per (profile, protein), multi-GPU drivers (hs_pssm_seq_hits is the merge).  Diagonals and
 * groups for profiles: hs_pssm_family_scan. */
HS_API hs_status hs_pssm_seq_scan(hs_handle* h, const double* S, const double* t, uint64_t nm,
                                  const uint64_t* id_start, uint64_t n_seq, uint32_t* out_m, uint32_t* out_seq,
                                  uint32_t* out_count, double* out_best_score, uint32_t* out_best_id, uint32_t* out_lo,
                                  uint32_t* out_hi, uint64_t cap, uint64_t* n_out, uint64_t* n_hits, uint64_t* cnt,
                                  uint64_t* seq_cnt);
/* ... every pointer but n_out / n_hits in device memory (streams: as hs_pssm_scan_dev) */
HS_API hs_status hs_pssm_seq_scan_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm,
                                      const uint64_t* d_id_start, uint64_t n_seq, uint32_t* d_out_m,
                                      uint32_t* d_out_seq, uint32_t* d_out_count, double* d_out_best_score,
                                      uint32_t* d_out_best_id, uint32_t* d_out_lo, uint32_t* d_out_hi, uint64_t cap,
                                      uint64_t* n_out, uint64_t* n_hits, uint64_t* d_cnt, uint64_t* d_seq_cnt);
/* The same rule on the host (no GPU, no handle) for any list of (m, id, score) tuples in any order: the merge of several
 * GPUs' hit lists.  A repeated (m, id) with equal score bits counts once, with different bits it is HS_ERR_INVALID; a
 * NaN score, m >= nm, an id at or beyond id_start[n_seq], an id_start the scan refuses (its end is not compared with
 * an index here) and a null output with cap > 0 are HS_ERR_INVALID, with nothing written.  HS_ERR_CAPACITY: *n_out
 * set, no row written. */
HS_API hs_status hs_pssm_seq_hits(const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                  uint64_t nm, const uint64_t* id_start, uint64_t n_seq, uint32_t* out_m,
                                  uint32_t* out_seq, uint32_t* out_count, double* out_best_score, uint32_t* out_best_id,
                                  uint32_t* out_lo, uint32_t* out_hi, uint64_t cap, uint64_t* n_out);

/* ---- PSSM families: the hits of related profiles reduced per family, sequence and diagonal ---------------------- */

/* A motif longer than k, or a protein family described by ordered blocks at fixed spacing, is several profiles.  Each
 * is scanned at a permissive threshold; a protein counts when several of them hit in register -- on one diagonal --
 * and their scores add up to a family threshold.  hs_seq_match does this reduction for k-mer queries; this is its
 * counterpart for profiles.  The hit list, large at permissive thresholds, never crosses PCIe.
 *
 * Underlying hits: S, t, the score and the hit rule are hs_pssm_scan's, bit for bit; H is the hit list hs_pssm_scan
 * returns for the same arguments on the same handle.  id_start [n_seq + 1] follows hs_pssm_seq_scan's rules (an id at
 * equal neighbours belongs to the LAST sequence that starts at or below it).
 * Key of a hit (m, id): g = m_group[m] (m_group == NULL: g = m, and n_groups must equal nm); s = the sequence that
 * owns id; off = id - id_start[s]; diag = off - m_off[m] as a signed number, of which out_diag holds the low 32 bits.
 * m_off == NULL: no diagonals are kept, diag is 0 for every hit (as in hs_seq_match).
 * Rows: one per distinct (g, s, diag) of H, ascending in that order (diag as the signed number).
 *   out_count       the row's hits.  On a diagonal a profile contributes at most one hit to a row, so with m_off given
 *                   the count is the number of the family's profiles that hit in register.
 *   out_sum         the sum of the row's hit_score: it starts from +0.0, the hits are added in ascending (m, id)
 *                   order, every partial sum is rounded to fp64; no FMA, no re-association.  The order is part of
 *                   the contract.
 *   out_best_score, out_best_m, out_best_id   the best hit under (score descending, m ascending, id ascending),
 *                   through the key transform of hsearch_amd/csrc/hs_pssm_topk.h; the score keeps the hit's bits.
 *   out_lo, out_hi  the smallest and the largest off among the row's hits.
 * Row filters, applied on the device: a row is reported iff count >= min_count and (t_group == NULL or
 * sum >= t_group[g]); t_group [n_groups].  *n_out, the capacity protocol and grp_rows [n_groups] (may be NULL: the
 * reported rows per group) count reported rows only.  *n_hits and cnt [nm] (may be NULL) are the scan's.
 * Capacity: counted in reported rows, the two-call pattern of hs_pssm_seq_scan: HS_ERR_CAPACITY comes with *n_out set
 * (cap = 0 with NULL arrays asks for the count); cnt and grp_rows are valid then.  hs_pssm_family_scan writes no row
 * then; the _dev form may have written the rows of the batches that still fitted.
 * Groups and batches: m_group must not decrease (a family's profiles are passed next to each other; a group may be
 * empty) and a group holds at most 4096 profiles, the scan's default batch.  Batches are cut at group starts, so every
 * row lies in one batch and the batches' rows follow one another in output order.  HS_OPT_QUERY_BATCH below a group's
 * size is raised to that group for the batch that holds it.  A batch whose survivors overflow the counter runs again
 * in smaller batches, still cut at group starts; a single group that overflows on its own is HS_ERR_CAPACITY with the
 * cause in hs_last_error, *n_out = 0, and nothing written by the host form.
 * Key width (hs_seq_match's rule): bits(n_groups - 1) + bits(n_seq - 1) + bits(max_len + max_off - 1) <= 64, where
 * max_len is the most ids of one sequence and max_off the largest m_off (0 without m_off); n_groups and n_seq are at
 * most 2^32, an m_off at most 2^31 - 1.
 * Errors, reported before anything is written: everything hs_pssm_scan and hs_pssm_seq_scan refuse; an m_group that
 * decreases or holds a value >= n_groups; a group above 4096 profiles; n_groups != nm with m_group == NULL;
 * min_count == 0; a NaN or infinite t_group entry; an m_off above 2^31 - 1; the width rule; null outputs with
 * cap > 0.  All HS_ERR_INVALID but the unbuilt index (HS_ERR_STATE).  The _dev form finds the value errors on the
 * device: the scan's reduction over the profiles, hs_seq_match's over m_group, m_off and id_start, one more over the
 * family arguments, and one read-back (which also brings m_group, nm words, for the cut points).
 * Purity: the rows are a pure function of (codes, S, t, m_group, m_off, id_start, min_count, t_group).  The profile
 * batch, HS_OPT_PSSM_FILTER, survivor splits and scheduling do not show in them.
 *
 * How (hsearch_amd/csrc/hs_pssm_family.hip): per batch, after the scan's own (m, id) sort, the sequence of every hit
 * (hs_pssm_seq.hip's search), a 64-bit row key, one stable radix sort of (row key, hit index), run heads and their
 * scan, one lane per row walking its run in order, the filters, a scan of their flags, and the kept rows written at the
 * call's running offset.  A row of L hits costs L dependent fp64 adds in one lane: the order of the sum is kept.
 * hs_profile after the call: the pssm_* fields as after a scan, hits, pssm_fam_rows (rows before the filters),
 * pssm_fam_kept (*n_out); ms_finalize covers the exact pass, the sorts and the reduction.  Every other entry point
 * runs as before, launch for launch.
 * Out of scope: groups that span batches, multi-GPU drivers (hs_pssm_family_hits is the merge), per-row p-values.
 * Chains with variable spacing between blocks (a gap penalty between diagonals): hs_pssm_family_chain below. */
HS_API hs_status hs_pssm_family_scan(hs_handle* h, const double* S, const double* t, uint64_t nm,
                                     const uint32_t* m_group, uint64_t n_groups, const uint32_t* m_off,
                                     const uint64_t* id_start, uint64_t n_seq, uint32_t min_count,
                                     const double* t_group, uint32_t* out_group, uint32_t* out_seq, int32_t* out_diag,
                                     uint32_t* out_count, double* out_sum, double* out_best_score,
                                     uint32_t* out_best_m, uint32_t* out_best_id, uint32_t* out_lo, uint32_t* out_hi,
                                     uint64_t cap, uint64_t* n_out, uint64_t* n_hits, uint64_t* cnt,
                                     uint64_t* grp_rows);
/* ... every pointer but n_out / n_hits in device memory (streams: as hs_pssm_scan_dev) */
HS_API hs_status hs_pssm_family_scan_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm,
                                         const uint32_t* d_m_group, uint64_t n_groups, const uint32_t* d_m_off,
                                         const uint64_t* d_id_start, uint64_t n_seq, uint32_t min_count,
                                         const double* d_t_group, uint32_t* d_out_group, uint32_t* d_out_seq,
                                         int32_t* d_out_diag, uint32_t* d_out_count, double* d_out_sum,
                                         double* d_out_best_score, uint32_t* d_out_best_m, uint32_t* d_out_best_id,
                                         uint32_t* d_out_lo, uint32_t* d_out_hi, uint64_t cap, uint64_t* n_out,
                                         uint64_t* n_hits, uint64_t* d_cnt, uint64_t* d_grp_rows);
/* The same rule on the host (no GPU, no handle) over any list of (m, id, score) tuples in any order: the merge of
 * several GPUs' hit lists and the reference the device is held to.  A repeated (m, id) with equal score bits counts
 * once, with different bits it is HS_ERR_INVALID.  The other refusals are hs_pssm_seq_hits' and the family arguments'
 * above (id_start's end is not compared with an index here).  A score of -0.0 in a tuple is read as +0.0 (no scan
 * produces it), so for such a tuple out_best_score does not keep the sign bit.  HS_ERR_CAPACITY: *n_out set, no row
 * written. */
HS_API hs_status hs_pssm_family_hits(const uint32_t* m, const uint32_t* id, const double* score, uint64_t n_tuples,
                                     uint64_t nm, const uint32_t* m_group, uint64_t n_groups, const uint32_t* m_off,
                                     const uint64_t* id_start, uint64_t n_seq, uint32_t min_count,
                                     const double* t_group, uint32_t* out_group, uint32_t* out_seq, int32_t* out_diag,
                                     uint32_t* out_count, double* out_sum, double* out_best_score,
                                     uint32_t* out_best_m, uint32_t* out_best_id, uint32_t* out_lo, uint32_t* out_hi,
                                     uint64_t cap, uint64_t* n_out);
/* The grouping call over hs_pssm_compare's self-mode hits (host only): families and offsets for hs_pssm_family_scan.
 * A hit (x, y, d) follows hs_pssm_compare's convention -- column p of Y meets column p + d of X, so Y lies d to the
 * right of X: pos[y] - pos[x] = d.  The hits are taken in the given order through a union-find that carries a position
 * relative to the root: a hit that joins two components fixes that distance; a hit inside one component that disagrees
 * with the positions already fixed is counted in *n_conflicts and changes nothing.  Components are numbered by their
 * smallest member, ascending (*n_groups of them; a profile without hits is a group of one).  out_group [nm];
 * out_off [nm] = pos[m] minus its component's minimum; out_order [nm] = the profiles sorted by (group, off, m): the
 * order in which to pass them to the scan.  The result depends on the order of the hits; hs_pssm_compare's (x, y)
 * ascending order makes it canonical.  HS_ERR_INVALID, before anything is written: x == y, an index >= nm,
 * |d| >= 2^30, an offset that passes 2^31 - 1, a component above 4096 members, a null array that is needed. */
HS_API hs_status hs_pssm_family_layout(const uint32_t* hit_x, const uint32_t* hit_y, const int32_t* hit_d,
                                       uint64_t n_hits, uint64_t nm, uint32_t* out_group, uint32_t* out_off,
                                       uint32_t* out_order, uint64_t* n_groups, uint64_t* n_conflicts);

/* ---- PSSM family chains: the best gapped chain of a family's hits per sequence ----------------------------------- */

/* hs_pssm_family_scan sees blocks at FIXED spacing: one inserted or deleted residue between two blocks moves the later
 * blocks onto another diagonal, and the protein falls apart into rows that each miss min_count.  This call links a
 * family's hits across neighbouring diagonals at a gap penalty and reports, per (family, sequence), the best chain.
 * Arguments, stream rules, host and device pointer rules and the capacity protocol are hs_pssm_family_scan's; new are
 * max_shift, gap_open, gap_ext, and the ten output arrays.
 *
 * Underlying hits: H is the hit list hs_pssm_scan(S, t) returns on the same handle, bit for bit.  A hit i = (m_i, id_i,
 * score_i) has g, s, off and diag = off - m_off[m] (a signed 64-bit number) as in hs_pssm_family_scan.  m_off is
 * REQUIRED here and must not decrease inside a group: a family's profiles are passed in block order, which is what
 * hs_pssm_family_layout's out_order produces.
 * Links: hit j may precede hit i iff both have the same g and the same s, m_j < m_i, off_j < off_i and
 * d = |diag_i - diag_j| <= max_shift.  Blocks may be skipped.  The penalty of a link, every operation a rounded fp64
 * operation, no FMA, no re-association: pen(0) = +0.0, and the link's value is then C(j) itself;
 * pen(d) = gap_open + gap_ext * (double)d for d >= 1, the product rounded first, then the sum.
 * Chain score: with the hits of a (g, s) segment in ascending (m, id), and v(j) = C(j) - pen(d) over the predecessors
 * of hit i, the best predecessor is the first under (v descending, n(j) descending, m_j descending, id_j ascending).
 * It is taken iff its v > +0.0:  C(i) = v + score_i, n(i) = n(j) + 1, first(i) = first(j), gaps(i) = gaps(j) + (d != 0).
 * Otherwise the chain starts at i:  C(i) = +0.0 + score_i, n(i) = 1, first(i) = i, gaps(i) = 0.  A local chain: a
 * non-positive prefix is dropped.  The maximum over predecessors is an exact comparison, so its order of evaluation
 * does not show; only the depth (the blocks of a family, at most 4096) is sequential.
 * No NaN arises: a predecessor is taken only at v > 0, scores are finite, pen is finite or, where gap_ext * d
 * overflows, +inf (v = -inf is not taken), and +inf + score is +inf.  No C is -0.0.
 * Rows: at most one per (g, s), ascending in (g, s).  Candidate ends are the hits i of the segment with
 * n(i) >= min_count and (t_group == NULL or C(i) >= t_group[g]); the row is the first candidate under (C descending,
 * n descending, m ascending, id ascending); a segment without a candidate reports nothing.
 *   out_group, out_seq           g, s
 *   out_count                    n: the blocks in the chain
 *   out_gaps                     its links with d != 0
 *   out_score                    C, its bits
 *   out_first_m, out_first_id    the chain's first hit
 *   out_last_m, out_last_id      the chain's last hit
 *   out_shift                    diag_last - diag_first (|shift| <= 4096 * 65535 fits)
 * *n_out, grp_rows [n_groups] and the capacity protocol count reported rows only; *n_hits and cnt [nm] are the scan's.
 * Purity: the rows are a pure function of (codes, S, t, m_group, m_off, id_start, max_shift, gap_open, gap_ext,
 * min_count, t_group).  Profile batch, HS_OPT_PSSM_FILTER, survivor splits and scheduling do not show.
 * Errors, reported before anything is written, all HS_ERR_INVALID but the unbuilt index (HS_ERR_STATE): everything
 * hs_pssm_family_scan refuses (its width rule included); m_off == NULL; an m_off that decreases inside a group (the
 * _dev form finds it in the family arguments' check kernel); max_shift > 65535 (HS_PSSM_CHAIN_MAX_SHIFT in
 * hsearch_amd/csrc/hs_pssm_chain.h: the cost of a hit is linear in it); gap_open or gap_ext NaN, infinite or negative
 * (-0.0 is read as +0.0).  Batches are cut at group starts as in hs_pssm_family_scan; a single group that overflows the
 * survivor counter is HS_ERR_CAPACITY with the cause in hs_last_error.
 *
 * How (hsearch_amd/csrc/hs_pssm_chain.hip): per batch, after the scan's own (m, id) sort, the sequence of every hit, a
 * segment key g << ws | s, one stable radix sort of (key, hit index) -- a segment's hits come out as runs by profile,
 * off ascending inside a run --, segment starts, then one wave per segment: a run is one DP level, its hits go to the
 * lanes, every lane bisects the admissible range of each earlier run and takes the maximum of at most 2 max_shift + 1
 * entries; the state lies in LDS for small segments and in global scratch otherwise; the wave then reduces the
 * candidate ends with shuffles.  A segment of H hits over r runs costs about H r (log H + 2 max_shift + 1) / 64 steps of
 * ONE wave: a huge segment (an everything-hits threshold on one long protein) is slow by design.
 * hs_profile after the call: the pssm_* fields as after a scan, hits, pssm_chain_segs (segments before the filters),
 * pssm_chain_kept (*n_out); ms_finalize covers the exact pass, the sorts and the chain.  Every other entry point runs
 * as before, launch for launch.
 * Out of scope: several non-overlapping chains per protein, the path from the device form (hs_pssm_family_chain_hits
 * gives it), families above 4096 profiles, per-chain p-values, multi-GPU drivers (the host rule is the merge). */
HS_API hs_status hs_pssm_family_chain(hs_handle* h, const double* S, const double* t, uint64_t nm,
                                      const uint32_t* m_group, uint64_t n_groups, const uint32_t* m_off,
                                      const uint64_t* id_start, uint64_t n_seq, uint32_t max_shift, double gap_open,
                                      double gap_ext, uint32_t min_count, const double* t_group, uint32_t* out_group,
                                      uint32_t* out_seq, uint32_t* out_count, uint32_t* out_gaps, double* out_score,
                                      uint32_t* out_first_m, uint32_t* out_first_id, uint32_t* out_last_m,
                                      uint32_t* out_last_id, int32_t* out_shift, uint64_t cap, uint64_t* n_out,
                                      uint64_t* n_hits, uint64_t* cnt, uint64_t* grp_rows);
/* ... every pointer but n_out / n_hits in device memory (streams: as hs_pssm_scan_dev) */
HS_API hs_status hs_pssm_family_chain_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm,
                                          const uint32_t* d_m_group, uint64_t n_groups, const uint32_t* d_m_off,
                                          const uint64_t* d_id_start, uint64_t n_seq, uint32_t max_shift,
                                          double gap_open, double gap_ext, uint32_t min_count, const double* d_t_group,
                                          uint32_t* d_out_group, uint32_t* d_out_seq, uint32_t* d_out_count,
                                          uint32_t* d_out_gaps, double* d_out_score, uint32_t* d_out_first_m,
                                          uint32_t* d_out_first_id, uint32_t* d_out_last_m, uint32_t* d_out_last_id,
                                          int32_t* d_out_shift, uint64_t cap, uint64_t* n_out, uint64_t* n_hits,
                                          uint64_t* d_cnt, uint64_t* d_grp_rows);
/* The same rule on the host (no GPU, no handle) over any list of (m, id, score) tuples in any order: the merge of
 * several GPUs' hit lists and the reference the device is held to.  A repeated (m, id) and a score of -0.0 are handled
 * as hs_pssm_family_hits handles them; a tuple with an infinite score is HS_ERR_INVALID here (no scan produces one, and
 * the rule's freedom from NaN rests on it).  The three path arrays may all be NULL (n_path too, then).  When given,
 * out_path_start [*n_out + 1] delimits, per reported row, the chain's hits (out_path_m, out_path_id) from first to
 * last, and *n_path is their total.  HS_ERR_CAPACITY: the rows exceed cap or the paths exceed path_cap; *n_out and
 * *n_path are set, nothing else is written.  Not quadratic in a segment's hits at a small max_shift: inside a segment
 * the hits of one profile are ascending in off, so the predecessors of a hit among one earlier profile's hits are one
 * contiguous range found by bisection: O(hits x profiles present x (log + 2 max_shift + 1)). */
HS_API hs_status hs_pssm_family_chain_hits(const uint32_t* m, const uint32_t* id, const double* score,
                                           uint64_t n_tuples, uint64_t nm, const uint32_t* m_group, uint64_t n_groups,
                                           const uint32_t* m_off, const uint64_t* id_start, uint64_t n_seq,
                                           uint32_t max_shift, double gap_open, double gap_ext, uint32_t min_count,
                                           const double* t_group, uint32_t* out_group, uint32_t* out_seq,
                                           uint32_t* out_count, uint32_t* out_gaps, double* out_score,
                                           uint32_t* out_first_m, uint32_t* out_first_id, uint32_t* out_last_m,
                                           uint32_t* out_last_id, int32_t* out_shift, uint64_t cap, uint64_t* n_out,
                                           uint64_t* out_path_start, uint32_t* out_path_m, uint32_t* out_path_id,
                                           uint64_t path_cap, uint64_t* n_path);

/* ---- PSSM hit counts and refinement: from a profile's hits back to a profile ------------------------------------- */

/* The step that makes a profile search iterative: scan, rebuild the position frequency matrix from what was found, take
 * log-odds, scan again (the PSI-BLAST loop; the hard-assignment EM step of a motif finder).  The counts are reduced on
 * the device; the hit list never crosses PCIe.
 *
 * hs_pssm_hit_counts.  S, t, the score and the hit rule are hs_pssm_scan's, bit for bit; H is the hit list hs_pssm_scan
 * returns for the same handle, S and t.
 *   id_start == NULL (every site counts): counts[m][p][a] = the (m, id) in H with codes[id][p] == a.
 *   id_start [n_seq + 1] given, under hs_pssm_seq_scan's rules (one site per protein): with Rows the rows
 *   hs_pssm_seq_scan returns for the same arguments, counts[m][p][a] = the rows (m, s) with codes[best_id][p] == a.
 * counts: uint32 [nm][k][alphabet], all of it written (zeros for a profile without hits); cnt [nm] (may be NULL): the
 * hits per profile, hs_pssm_scan's cnt; used [nm] (may be NULL): the sites counted -- cnt without id_start,
 * hs_pssm_seq_scan's seq_cnt with it; *n_hits: the scan's.  For every m and p the sum over a of counts[m][p][a] is
 * used[m].  The output is dense: there is no capacity protocol.
 * Errors, reported before anything is written: everything hs_pssm_scan refuses; with id_start given, everything
 * hs_pssm_seq_scan refuses about it (n_seq == 0 with n > 0, n_seq > 2^32, an id_start that does not ascend from 0 to
 * n); a null counts with nm > 0.  The _dev form finds the value errors on the device with one read-back.
 * Purity: a pure function of (codes, S, t, id_start).  HS_OPT_QUERY_BATCH, HS_OPT_PSSM_FILTER,
 * HS_OPT_PSSM_COUNT_CHUNK, survivor splits and scheduling do not show in it.
 * How (hsearch_amd/csrc/hs_pssm_counts.hip): the scan's batches, tables, filter and exact pass as they are.  Every
 * site: a batch's hits are ordered on their profile bits alone; one site per protein: the passes of hs_pssm_seq.hip
 * give the rows' best ids.  Work items (profile run, chunk of HS_OPT_PSSM_COUNT_CHUNK sites) go one to a wave, which
 * counts in an LDS histogram and stores it (a whole run) or adds its non-zero bins with integer atomics (a cut run).
 * hs_profile after the call: the pssm_* fields as after a scan, pssm_count_sites, pssm_count_items, hits.
 *
 * hs_pssm_refine (host pointers).  S0 [nm][k][alphabet]; t [nm], fixed over the iterations; id_start or NULL as above;
 * bg [alphabet] (NULL: hs_pssm_background of the counts of one all-zero profile at t = 0 without id_start -- the
 * residue composition of the index, one extra scan; an empty index is HS_ERR_INVALID then); pseudo; 1 <= n_iter <= 100.
 * Iteration i = 0, 1, ... computes C_i = hs_pssm_hit_counts(S_i, t).  If i > 0 and C_i equals C_{i-1} byte for byte the
 * loop has converged and stops.  Otherwise S_{i+1}[m] = hs_pssm_log_odds(C_i[m]) where used_i[m] > 0, else S_i[m] (a
 * profile that finds nothing keeps its matrix), and the loop stops after n_iter scans.  S_out: the last S computed
 * (S_i on convergence at i, else S_{n_iter}); counts, used (may be NULL): of the last scan; *iters: the scans run, not
 * counting the background's; *converged.  If it converged, hs_pssm_hit_counts(S_out, t) gives counts.  Per iteration
 * only counts (down) and S (up) cross PCIe.  Nothing is written when the arguments or S0's values are refused.
 * Out of scope: a device log-odds (device log2 is not the host's bit for bit), multi-GPU drivers (hs_pssm_count_hits is
 * the merge).  (A threshold update rule: hs_pssm_refine_rank below; sequence weights: hs_pssm_refine_weighted below.) */
HS_API hs_status hs_pssm_hit_counts(hs_handle* h, const double* S, const double* t, uint64_t nm,
                                    const uint64_t* id_start, uint64_t n_seq, uint32_t* counts, uint64_t* cnt,
                                    uint64_t* used, uint64_t* n_hits);
/* ... every pointer but n_hits in device memory (streams: as hs_pssm_scan_dev) */
HS_API hs_status hs_pssm_hit_counts_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm,
                                        const uint64_t* d_id_start, uint64_t n_seq, uint32_t* d_counts, uint64_t* d_cnt,
                                        uint64_t* d_used, uint64_t* n_hits);
HS_API hs_status hs_pssm_refine(hs_handle* h, const double* S0, const double* t, uint64_t nm, const uint64_t* id_start,
                                uint64_t n_seq, const double* bg, double pseudo, uint32_t n_iter, double* S_out,
                                uint32_t* counts, uint64_t* used, uint32_t* iters, uint32_t* converged);
/* The counting rule on the host (no GPU, no handle) for any list of (m, id, score) tuples in any order over codes
 * [n][k]: the merge of several GPUs' shares.  A repeated (m, id) with equal score bits counts once, with different bits
 * it is HS_ERR_INVALID (as hs_pssm_seq_hits); with id_start (which must ascend from 0 to n) the sites are the best
 * hits of hs_pssm_seq_hits' rows.  m >= nm, id >= n, a NaN score, a counted code >= alphabet, alphabet > 32, k == 0 and
 * a null counts with nm > 0 are HS_ERR_INVALID, with nothing written.  used may be NULL. */
HS_API hs_status hs_pssm_count_hits(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet, const uint32_t* m,
                                    const uint32_t* id, const double* score, uint64_t n_tuples, uint64_t nm,
                                    const uint64_t* id_start, uint64_t n_seq, uint32_t* counts, uint64_t* used);
/* S[m][p][a] = log2((((double)c + pseudo * bg[a]) / ((double)size + pseudo)) / bg[a]), c = counts[m][p][a], size = the
 * sum over a of counts[m][p][a]; every operation rounded to fp64, no FMA contraction, log2 the C library's.  bg[a] <= 0,
 * a bg that is not finite and a pseudo that is not finite and > 0 are HS_ERR_INVALID, as is a bg so small that an entry
 * would not be finite; nothing is written then.  Every entry written is finite and passes the scan's value check. */
HS_API hs_status hs_pssm_log_odds(const uint32_t* counts, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                  double pseudo, double* S_out);
/* bg[a] = (the sum over p of counts_row[p][a]) / (the sum over p and a) for the counts [k][alphabet] of one profile; a
 * zero is then replaced by the smallest positive entry, without renormalising.  All-zero counts: HS_ERR_INVALID. */
HS_API hs_status hs_pssm_background(const uint32_t* counts_row, uint32_t k, uint32_t alphabet, double* bg_out);

/* ---- PSSM rank: the threshold that admits a profile's N best k-mers ---------------------------------------------- */

/* Every profile call above takes t [nm] in the units of the scores, and nobody has such a number for a log-odds matrix.
 * This is the order statistic: for each profile the exact score of its rank-th best k-mer over the whole index, for any
 * rank from 1 to n, found on the device.  "The 10 000 best windows" becomes a t that every call above accepts.
 *
 * Inputs: S [nm][k][alphabet] as for hs_pssm_scan, with the same value checks; rank [nm], each within 1 .. n.
 * Score: hs_pssm_scan's, bit for bit -- from +0.0, left to right, every sum rounded to fp64.
 * t_rank[m]: the rank[m]-th largest score of profile m over the index's n k-mers, counted with multiplicity: the bits
 * of a score that occurs.  cnt_ge[m]: the k-mers with score >= t_rank[m]; at least rank[m], larger where scores tie at
 * the threshold; hs_pssm_scan at t_rank returns exactly cnt_ge[m] hits for profile m.  cnt_gt[m]: the k-mers with score
 * > t_rank[m]; below rank[m].  t_scan [nm], rounds [nm] (either may be NULL): diagnostics defined by the sample rule
 * below, and the only outputs that depend on the sample size.
 * Errors, reported before anything is written: everything hs_pssm_scan refuses about the handle, nm and S; a null rank,
 * t_rank, cnt_ge or cnt_gt with nm > 0; a rank of 0 or above n (with n == 0 and nm > 0 every rank is refused).  The
 * _dev form finds the value errors on the device with one read-back.  nm == 0 is HS_OK with nothing written.
 * Purity: t_rank, cnt_ge and cnt_gt are a pure function of (codes, S, rank).  HS_OPT_PSSM_RANK_SAMPLE,
 * HS_OPT_QUERY_BATCH, HS_OPT_PSSM_FILTER, survivor splits, scheduling and the number of rounds do not show in them.
 *
 * How, and why it is exact (hsearch_amd/csrc/hs_pssm_rank.hip; the rule in integers: hs_pssm_rank.h).  The N-th best of
 * a sample bounds nothing above the sample's own rank, so the sample only proposes a threshold and the scan's hit count
 * disposes.  n_s = min(n, HS_OPT_PSSM_RANK_SAMPLE); the sample is hs_pssm_topk's, the k-mers floor(j * n / n_s).
 * q = ceil(rank * n_s / n), slack0 = 4 * ceil(sqrt(q)) + 8, and in round j = 0, 1, ... the sample rank is r_s = q +
 * slack0 * 4^j (n_s == n: r_s = rank, round 0 is final).  t_scan = the r_s-th largest sample score, -DBL_MAX (every
 * k-mer) once r_s > n_s.  A round scans the unresolved profiles at t_scan with hs_pssm_scan's tables, filter and exact
 * pass; a profile is resolved iff its hits number at least rank[m] -- then every k-mer at or above the true t_rank is
 * among them and a segmented radix select over their keys is exact.  The others go to round j + 1; the round at
 * -DBL_MAX resolves everything.  t_scan[m] and rounds[m] report the round that resolved profile m (rounds counts the
 * retries: 0 for the first round).  A retry reruns the batches with the resolved profiles at +DBL_MAX.
 * The constant 8 and the sample's grain make small ranks cost several times their size in hits: ranks up to 64 are
 * hs_pssm_topk's business.
 * hs_profile after the call: the pssm_* scan fields and hits summed over every scan the call ran; pssm_rank_sample,
 * pssm_rank_retries; ms_hash (sample pass + its select), ms_verify (tables + filter), ms_finalize (exact pass +
 * select), ms_total.  Every other entry point runs as before, launch for launch.
 * Out of scope: per-protein ranks, multi-GPU drivers -- ranks do NOT merge from per-GPU thresholds (the rank-th best of
 * a union is no function of the parts' rank-th bests).  Thresholds from a null model: hs_pssm_pvalue_threshold below. */
HS_API hs_status hs_pssm_rank(hs_handle* h, const double* S, const uint64_t* rank, uint64_t nm, double* t_rank,
                              uint64_t* cnt_ge, uint64_t* cnt_gt, double* t_scan, uint32_t* rounds);
/* ... every pointer in device memory (streams: as hs_pssm_scan_dev) */
HS_API hs_status hs_pssm_rank_dev(hs_handle* h, const double* d_S, const uint64_t* d_rank, uint64_t nm,
                                  double* d_t_rank, uint64_t* d_cnt_ge, uint64_t* d_cnt_gt, double* d_t_scan,
                                  uint32_t* d_rounds);
/* The same rule on the host (no GPU, no handle): every (profile, k-mer) pair scored under the contract over codes
 * [n][k], and the selection.  The refusals above, and k == 0, alphabet outside 1 .. 32, a code >= alphabet, n >= 2^32,
 * nm >= 2^27, null codes with n > 0: HS_ERR_INVALID with nothing written.  The answer for an index that is on no GPU. */
HS_API hs_status hs_pssm_rank_scores(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet, const double* S,
                                     uint64_t nm, const uint64_t* rank, double* t_rank, uint64_t* cnt_ge,
                                     uint64_t* cnt_gt);
/* The sample rule: *sample_rank = r_s of `round`, n_s + 1 where r_s lies beyond the sample (scan at -DBL_MAX).  rank
 * outside 1 .. n, n_s outside 1 .. n, n >= 2^32 and a null output are HS_ERR_INVALID. */
HS_API hs_status hs_pssm_rank_plan(uint64_t rank, uint64_t n, uint64_t n_s, uint32_t round, uint64_t* sample_rank);
/* hs_pssm_refine's loop, rules, refusals and outputs with one change: iteration i first computes t_i = hs_pssm_rank(S_i,
 * rank) and then C_i = hs_pssm_hit_counts(S_i, t_i), so the hit count stays at rank (and its ties) while the matrix
 * moves.  rank [nm], each within 1 .. n; t_out [nm]: the threshold of the last scan.  Convergence is still C_i ==
 * C_{i-1} byte for byte.  used may exceed rank (ties at the threshold); in the one-per-protein mode (id_start given)
 * rank still counts k-mers, not proteins, so used is then at most cnt_ge.  An iteration is two scans. */
HS_API hs_status hs_pssm_refine_rank(hs_handle* h, const double* S0, const uint64_t* rank, uint64_t nm,
                                     const uint64_t* id_start, uint64_t n_seq, const double* bg, double pseudo,
                                     uint32_t n_iter, double* S_out, double* t_out, uint32_t* counts, uint64_t* used,
                                     uint32_t* iters, uint32_t* converged);

/* ---- PSSM sequence weights: Henikoff-weighted counts and the weighted refine loop -------------------------------- */

/* hs_pssm_hit_counts counts every site as 1, so a family present in hundreds of near-identical copies owns the profile
 * rebuilt from it.  These calls weigh the sites with position-based sequence weights (Henikoff and Henikoff 1994), in
 * integers, so that the result is as free of summation order as the raw counts are.
 *
 * The rule.  For profile m let its sites be exactly hs_pssm_hit_counts' (every hit, or with id_start the best hit of
 * every (profile, protein) row), x_i the k-mer of site i and c[p][a] the raw counts.
 *   r[p]        = the residues a with c[p][a] > 0;     distinct[m] = the sum over p of r[p]            (uint32)
 *   u[p][a]     = floor(2^56 / (r[p] * c[p][a])) in 64-bit integers, 0 where c[p][a] == 0           (hs_pssm_weight_u)
 *   W(i)        = the sum over p of u[p][x_ip]                                                       (uint64)
 *   wcounts[m][p][a] = the sum of W(i) over the sites with x_ip == a;   wsum[m] = the sum of W(i) over the sites
 * For every m and p the sum over a of wcounts[m][p][a] is wsum[m].  Nothing overflows: wsum = sum_p sum_a c[p][a] *
 * u[p][a] and c * floor(2^56 / (r c)) <= 2^56 / r for each of the r residues that occur, so wsum[m] <= k * 2^56 <= 75 *
 * 2^56 < 2^63, and every W(i) and wcounts entry is a partial sum of it.
 *
 * hs_pssm_weighted_counts.  S, t, id_start, n_seq, cnt, used, *n_hits: hs_pssm_hit_counts'.  counts (may be NULL: the
 * handle's scratch holds them), wsum [nm], distinct [nm], cnt, used may be NULL; wcounts uint64 [nm][k][alphabet] is
 * required with nm > 0.  Every array given is written whole (zeros for a profile without hits); the output is dense,
 * there is no capacity protocol.  counts is what hs_pssm_hit_counts gives on the same handle.
 * Errors, reported before anything is written: everything hs_pssm_hit_counts refuses (wcounts in the place of counts).
 * The _dev form finds the value errors on the device with one read-back.
 * Purity: a pure function of (codes, S, t, id_start).  HS_OPT_QUERY_BATCH, HS_OPT_PSSM_FILTER,
 * HS_OPT_PSSM_COUNT_CHUNK, survivor splits and scheduling do not show in it.
 * How (hsearch_amd/csrc/hs_pssm_weights.hip): hs_pssm_hit_counts' batches and count pass as they are; every hit of a
 * profile lies in one batch, so after the count pass a small kernel turns the batch's counts into u tables and
 * distinct, and a second pass over the same sites and work items reduces W(i) across the lanes of a site and adds it
 * into a uint64 LDS histogram per wave -- stored plainly for a whole run, added with 64-bit integer atomics for a cut
 * one.  hs_pssm_hit_counts itself launches what it launched.
 * hs_profile after the call: as after hs_pssm_hit_counts, and pssm_weight_sites, pssm_weight_items.
 *
 * hs_pssm_refine_weighted (host pointers).  hs_pssm_refine's loop, refusals and outputs (t given, rank NULL) or
 * hs_pssm_refine_rank's (rank given, t NULL; t_out required) -- exactly one of t and rank -- with these changes:
 * iteration i computes (C_i, WC_i, wsum_i, distinct_i) = hs_pssm_weighted_counts(S_i, t_i); the loop has converged when
 * C_i == C_{i-1} and WC_i == WC_{i-1} byte for byte; otherwise S_{i+1}[m] = hs_pssm_log_odds_weighted(WC_i[m], wsum_i[m],
 * n_eff) where used_i[m] > 0, with n_eff = (double)used_i[m] (neff_rule 0: the weights only reshape the frequencies) or
 * (double)distinct_i[m] / (double)k (neff_rule 1: the mean number of distinct residues per column, PSI-BLAST's measure
 * of the independent evidence).  Another neff_rule is HS_ERR_INVALID.  counts, wcounts, wsum, distinct, used (each may
 * be NULL): of the last scan.  hs_pssm_refine and hs_pssm_refine_rank are unchanged.
 * Out of scope: weights for hs_cluster_profile, position-specific pseudo-counts, a device log-odds, multi-GPU drivers --
 * weights do NOT merge from per-GPU wcounts (they depend on the global counts); hs_pssm_weight_hits over the merged hit
 * list is the merge. */
HS_API hs_status hs_pssm_weighted_counts(hs_handle* h, const double* S, const double* t, uint64_t nm,
                                         const uint64_t* id_start, uint64_t n_seq, uint32_t* counts, uint64_t* wcounts,
                                         uint64_t* wsum, uint32_t* distinct, uint64_t* cnt, uint64_t* used,
                                         uint64_t* n_hits);
/* ... every pointer but n_hits in device memory (streams: as hs_pssm_scan_dev) */
HS_API hs_status hs_pssm_weighted_counts_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm,
                                             const uint64_t* d_id_start, uint64_t n_seq, uint32_t* d_counts,
                                             uint64_t* d_wcounts, uint64_t* d_wsum, uint32_t* d_distinct,
                                             uint64_t* d_cnt, uint64_t* d_used, uint64_t* n_hits);
HS_API hs_status hs_pssm_refine_weighted(hs_handle* h, const double* S0, const double* t, const uint64_t* rank,
                                         uint64_t nm, const uint64_t* id_start, uint64_t n_seq, const double* bg,
                                         double pseudo, uint32_t neff_rule, uint32_t n_iter, double* S_out,
                                         double* t_out, uint32_t* counts, uint64_t* wcounts, uint64_t* wsum,
                                         uint32_t* distinct, uint64_t* used, uint32_t* iters, uint32_t* converged);
/* The weighting rule on the host (no GPU, no handle) for any list of (m, id, score) tuples in any order: the site
 * selection and every refusal are hs_pssm_count_hits'; k > 127 and a null wcounts with nm > 0 are HS_ERR_INVALID too.
 * counts, wsum, distinct and used may be NULL.  Nothing is written when it refuses. */
HS_API hs_status hs_pssm_weight_hits(const uint8_t* codes, uint64_t n, uint32_t k, uint32_t alphabet, const uint32_t* m,
                                     const uint32_t* id, const double* score, uint64_t n_tuples, uint64_t nm,
                                     const uint64_t* id_start, uint64_t n_seq, uint32_t* counts, uint64_t* wcounts,
                                     uint64_t* wsum, uint32_t* distinct, uint64_t* used);
/* S[m][p][a] = log2(((f * n_eff[m] + pseudo * bg[a]) / (n_eff[m] + pseudo)) / bg[a]), f = wsum[m] ? (double)wcounts[m][p][a]
 * / (double)wsum[m] : 0.0; every operation rounded to fp64, no FMA contraction, log2 the C library's.  Everything
 * hs_pssm_log_odds refuses, an n_eff that is not finite or below 0 and a wcounts entry above its wsum are
 * HS_ERR_INVALID; nothing is written then. */
HS_API hs_status hs_pssm_log_odds_weighted(const uint64_t* wcounts, const uint64_t* wsum, const double* n_eff,
                                           uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg, double pseudo,
                                           double* S_out);
/* u(r, c) = floor(2^56 / (r * c)), 0 where r == 0 or c == 0: r residues occur at the position, this one c times. */
HS_API uint64_t hs_pssm_weight_u(uint32_t r, uint32_t c);

/* ---- PSSM p-values: thresholds and hit significance from a null model ------------------------------------------- */

/* hs_pssm_topk and hs_pssm_rank read a threshold off the database.  This is the answer that does not depend on it: the
 * probability that a random k-mer scores at least t, and the t that belongs to a probability.  Scores of two profiles
 * become comparable, and a threshold can be carried from one database to the next.
 *
 * The null model: positions independent, residue a with weight bg[a].  bg [alphabet]: every entry finite and within
 * 0 .. 1, at least one positive; it is NOT renormalised (hs_pssm_background's output does not sum to exactly 1), and P
 * below is the product measure of these weights.  bg == NULL (handle forms): the index's residue composition exactly as
 * hs_pssm_refine takes it -- one extra scan; the index must be built and hold k-mers then.  With bg given no index is
 * needed.
 * S [nm][k][alphabet]: as for hs_pssm_scan, with the same value checks.  t_lo [nm] (NULL: 0 for every profile; each
 * finite): the lowest score the caller wants p-values for -- the grid of `bins` = B bins (HS_OPT_PSSM_NULL_BINS, default
 * 4096, 64 .. 8192; an argument of the host forms) covers t_lo .. the profile's maximal score.  0 is the natural choice
 * for log-odds.  A profile whose maximal score lies below t_lo is dead: p_hi = 0 at and above t_lo.
 *
 * THE INVARIANT: for every t,  p_lo(t) <= P{ x : fl(x) >= t } <= p_hi(t),  fl the contract's rounded score.  The rule,
 * its explicit margins and the proof: hsearch_amd/csrc/hs_pssm_null.h.  In short: the entries
 * are moved up (down) by the bound of the sum's rounding, the deficits below each position's maximum are rounded down
 * (up) to multiples of delta >= (max score - t_lo) / (B - 1), the two integer distributions are convolved over the k
 * positions in a fixed order of fp64 operations, summed to cdfs in a fixed blocked order, and looked up at J_hi(t) =
 * floor((max - t) / delta) moved up, J_lo moved down, times (1 +- e) with e = (k (alphabet + 1) + 202) 2^-52, -+ 1e-300.
 * A forbidden residue of -10^30 saturates its own bin shift and does not widen the grid.  t below the grid (J_hi >= B):
 * p_hi = 1, which reads "not computed".  p_hi / p_lo tightens with B and widens with k; both are monotone in t.
 *
 * hs_pssm_pvalue: the bracket of n hits (hit_m[i] < nm, hit_score[i] anything but NaN) in any order -- what
 * hs_pssm_scan returns, or any other list.  p_lo may be NULL: the upper side alone runs, which halves the work.
 * hs_pssm_pvalue_threshold: per profile the threshold of p[m] in (0, 1]: with J* the largest bin whose p_hi is <= p[m],
 * t_p[m] = the smallest double t with J_hi(t) <= J* and flag[m] = 0 -- then p_hi(t_p) <= p, and p_hi of the next double
 * below t_p exceeds p; J* = B - 1: t_p = t_lo[m], flag 1 (clipped: a lower t_lo might admit more); no such bin: t_p =
 * +DBL_MAX, flag 2 (nothing is admissible on this grid; a scan at t_p finds nothing).  p_hi [nm], p_lo [nm] (may be
 * NULL): the bracket at t_p.  t_p is a threshold every profile call above accepts.
 * Errors, reported before anything is written: nm >= 2^27; a null S, or a null bg without a built, non-empty index
 * (HS_ERR_STATE for an unbuilt one); a profile entry NaN, infinite or beyond 2^100; a bg or t_lo outside the rule above;
 * a p that is NaN or outside (0, 1]; hit_m >= nm; a NaN hit_score; null outputs (p_lo excepted) with work to do.  The
 * _dev forms find the value errors on the device with one read-back.  nm == 0 (thresholds) and n == 0 (p-values) are
 * HS_OK with nothing written.
 * Purity: the outputs are a pure function of (S, bg, t_lo, bins, and the hits or p).  HS_OPT_QUERY_BATCH (profiles per
 * batch here; default: at most 4096 and few enough that a batch's cdf tables stay within 2^28 bytes) and scheduling do
 * not show.  The device's bits are the host forms' bits.
 * hs_profile after the call: pssm_null_bins, pssm_null_profiles, ms_hash (the tables and the convolution), ms_finalize
 * (the lookups or the threshold search), ms_total.  Every other entry point runs as before, launch for launch.
 * Out of scope: more than 8192 bins, Markov backgrounds, E-values (a multiplication by n * nm the caller can do), a
 * p-value form of hs_pssm_refine, per-protein p-values, multi-GPU drivers (the rule does not read the database). */
HS_API hs_status hs_pssm_pvalue(hs_handle* h, const double* S, const double* bg, const double* t_lo, uint64_t nm,
                                const uint32_t* hit_m, const double* hit_score, uint64_t n, double* p_hi, double* p_lo);
/* ... every pointer in device memory (streams: as hs_pssm_scan_dev): the hit list of hs_pssm_scan_dev never crosses PCIe */
HS_API hs_status hs_pssm_pvalue_dev(hs_handle* h, const double* d_S, const double* d_bg, const double* d_t_lo,
                                    uint64_t nm, const uint32_t* d_hit_m, const double* d_hit_score, uint64_t n,
                                    double* d_p_hi, double* d_p_lo);
HS_API hs_status hs_pssm_pvalue_threshold(hs_handle* h, const double* S, const double* bg, const double* t_lo,
                                          const double* p, uint64_t nm, double* t_p, double* p_hi, double* p_lo,
                                          uint32_t* flag);
HS_API hs_status hs_pssm_pvalue_threshold_dev(hs_handle* h, const double* d_S, const double* d_bg,
                                              const double* d_t_lo, const double* d_p, uint64_t nm, double* d_t_p,
                                              double* d_p_hi, double* d_p_lo, uint32_t* d_flag);
/* The same rule on the host (no GPU, no handle); k within 1 .. 75, alphabet within 1 .. 32, bins within 64 .. 8192, bg
 * required; everything else refused as above, HS_ERR_INVALID with nothing written.  hs_pssm_null_tables: the tables the
 * device builds, bit for bit -- q_dn, q_up [nm][k][alphabet] the bin shifts (saturated at bins), delta [nm], dead [nm],
 * cdf_dn, cdf_up [nm][bins]; any output may be NULL.  hs_pssm_pvalue_host and hs_pssm_threshold_host together are the
 * whole rule. */
HS_API hs_status hs_pssm_null_tables(const double* S, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                     const double* t_lo, uint32_t bins, uint16_t* q_dn, uint16_t* q_up, double* delta,
                                     uint8_t* dead, double* cdf_dn, double* cdf_up);
HS_API hs_status hs_pssm_pvalue_host(const double* S, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                     const double* t_lo, uint32_t bins, const uint32_t* hit_m, const double* hit_score,
                                     uint64_t n, double* p_hi, double* p_lo);
HS_API hs_status hs_pssm_threshold_host(const double* S, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                        const double* t_lo, uint32_t bins, const double* p, double* t_p, double* p_hi,
                                        double* p_lo, uint32_t* flag);

/* ---- hs_pssm_compare: profile against profile, at every offset -----------------------------
 * X [nx][k][alphabet] and Y [ny][k][alphabet] are fp64 profiles of the handle's k and alphabet (a narrower motif is
 * passed zero-padded to k columns: zero columns add +0.0), t [nx] one threshold per X profile, min_overlap = v in
 * 1..k.  No index is needed: the call works on a handle that was never built.
 *   col(x, i, y, j)  = sum over r = 0 .. alphabet - 1 of X[x][i][r] * Y[y][j][r], from +0.0, left to right, every
 *                      product and every sum rounded to fp64 on its own (no FMA);
 *   score(x, y, d)   = sum of col(x, p + d, y, p) over p ascending from max(0, -d) to min(k, k - d) - 1, from +0.0,
 *                      every sum rounded: column p of Y meets column p + d of X, d in -(k - v) .. k - v;
 *   best(x, y)       = the largest score over the allowed d; among equal scores the first in the order (|d|, d)
 *                      ascending (0, -1, +1, -2, +2, ...) wins;
 *   (x, y) is a hit  iff best(x, y) >= t[x].
 * One hit per pair in (x, y) ascending order: hit_x, hit_y, hit_d (int32: the winning offset), hit_score (bit for
 * bit).  cnt [nx] (may be NULL) = the hits of every X profile, valid on HS_OK and on HS_ERR_CAPACITY; the two-call
 * capacity pattern is hs_pssm_scan's (cap = 0 with null outputs counts).  Y == NULL: X against itself -- only pairs
 * x < y are examined and reported, under t[x]; score(x, y, d) and score(y, x, -d) are the same bits.
 * Refused with HS_ERR_INVALID before anything is written: nx or ny at or above 2^27, or 0 beside a non-zero other;
 * v outside 1..k; a NaN, an infinity or |entry| > 2^100 in X or Y; a NaN or infinite threshold; null outputs with
 * cap > 0.  The _dev form (every pointer but n_hits on the device) finds the value errors on the device with one
 * read-back.
 * The result is a pure function of (X, Y, t, v): neither HS_OPT_QUERY_BATCH (X profiles per batch), nor
 * HS_OPT_PSSM_CMP_FILTER, nor the survivors' order shows in it.  The filter (hsearch_amd/csrc/hs_pssm_compare.h:
 * int8 codes on v_mfma_i32_16x16x64_i8, one chain per offset) never decides a hit; it runs wherever
 * k * stride <= 1024 bytes, stride = the alphabet rounded up to 16; other shapes go through the exact pass alone
 * (pssm_cmp_steps = 0).  hs_profile after the call: pssm_cmp_pairs, pssm_cmp_survivors, pssm_cmp_steps, hits,
 * ms_verify (tables + filter), ms_finalize (exact pass + ordering), ms_total. */
HS_API hs_status hs_pssm_compare(hs_handle* h, const double* X, uint64_t nx, const double* Y, uint64_t ny,
                                 const double* t, uint32_t min_overlap, uint32_t* hit_x, uint32_t* hit_y,
                                 int32_t* hit_d, double* hit_score, uint64_t cap, uint64_t* n_hits, uint64_t* cnt);
HS_API hs_status hs_pssm_compare_dev(hs_handle* h, const double* d_X, uint64_t nx, const double* d_Y, uint64_t ny,
                                     const double* d_t, uint32_t min_overlap, uint32_t* d_hit_x, uint32_t* d_hit_y,
                                     int32_t* d_hit_d, double* d_hit_score, uint64_t cap, uint64_t* n_hits,
                                     uint64_t* d_cnt);
/* The same rule on the host, no GPU and no handle: hs_pssm_compare_host is the contract on one CPU thread (same
 * outputs, same refusals; HS_ERR_CAPACITY with *n_hits when cap is short).  hs_pssm_compare_tables: the filter's
 * tables per profile, the bits the device builds -- q [nx][k][alphabet] int8 codes rint(x / s), s [nx] the scale
 * amax / 127, l1 [nx] an upper bound of the profile's sum of |x|, amax [nx]; any output may be NULL.
 * hs_pssm_compare_pass: the filter's test on a pair from those tables and I = the largest exact integer sum of code
 * products over the allowed offsets (1: the pair goes to the exact pass).  hs_pssm_compare_columns: the column
 * transform a user applies before comparing, out [nm][k][alphabet] -- mode 0: every column centred on its mean and
 * divided by its Euclidean norm (the score is then a sum of column Pearson correlations; a constant column becomes
 * zeros), mode 1: divided by the norm only (cosine).  The order of operations: hs_pssm_compare.h. */
HS_API hs_status hs_pssm_compare_host(const double* X, uint64_t nx, const double* Y, uint64_t ny, uint32_t k,
                                      uint32_t alphabet, const double* t, uint32_t min_overlap, uint32_t* hit_x,
                                      uint32_t* hit_y, int32_t* hit_d, double* hit_score, uint64_t cap,
                                      uint64_t* n_hits, uint64_t* cnt);
HS_API hs_status hs_pssm_compare_tables(const double* X, uint64_t nx, uint32_t k, uint32_t alphabet, int8_t* q,
                                        double* s, double* l1, double* amax);
HS_API int hs_pssm_compare_pass(int64_t I, double s_x, double l1_x, double amax_x, double s_y, double l1_y,
                                uint32_t k, uint32_t alphabet, double t);
HS_API hs_status hs_pssm_compare_columns(const double* X, uint64_t nm, uint32_t k, uint32_t alphabet, int mode,
                                         double* out);

/* Replaces Clustering() (hclust2.cpp:86-151) with explicit planes a[L][K][d], b[L][K]: table by
 * table, an LSH table over the not-yet-absorbed k-mers, then greedy leader clustering inside every
 * bucket in ascending id order.  The distance work runs on the GPU (hs_self_join per table), the
 * order-dependent greedy pass on the host.  Outputs: merged[n] in {0 unprocessed, 1 center,
 * 2 absorbed} (hclust2.cpp:93-96), owner[n] = absorbing center (itself if not absorbed),
 * absorbed_table[n] = table in which it was absorbed (0xffffffff if not): members of a cluster in
 * the reference's file order are its center followed by its members sorted by (absorbed_table, id). */
HS_API hs_status hs_clustering(const hs_params* params, const double* a, const double* b,
                               const double* coords, const uint8_t* codes, uint64_t n, double R,
                               uint8_t* merged, uint32_t* owner, uint32_t* absorbed_table,
                               char* err, uint32_t err_cap);

/* Clustering() spread over `world` GPUs: the distance work of a table --
 * the within-bucket join over the not-yet-absorbed k-mers -- is sharded by the `i` side, one
 * contiguous block of the active k-mers per rank; the one exchange step is an all-gather of the
 * edge lists (done by the caller, e.g. over RCCL); the order-dependent greedy pass then runs
 * identically on every rank.  Per table l = 0..L-1 every rank calls
 *   hs_clustering_table_edges(st, l, rank, world, ...)  -> its edges (i, j) in ORIGINAL k-mer
 *                                   numbers, sqrt(d2) <= R, two-call capacity protocol
 *   <all-gather of the edges>
 *   hs_clustering_table_apply(st, l, all edges in any order)   (host only, no GPU)
 * and after the last table hs_clustering_end, which writes the outputs of hs_clustering and frees
 * the state (outputs may be NULL to just free).  hs_clustering is the world = 1 composition.
 * `codes` must stay valid until hs_clustering_end. */
typedef struct hs_cluster_state hs_cluster_state;
HS_API hs_status hs_clustering_begin(const hs_params* params, const double* a, const double* b,
                                     const double* coords, const uint8_t* codes, uint64_t n, double R,
                                     hs_cluster_state** out, char* err, uint32_t err_cap);
HS_API hs_status hs_clustering_table_edges(hs_cluster_state* st, uint32_t l, uint32_t rank,
                                           uint32_t world, uint32_t* edge_i, uint32_t* edge_j,
                                           double* edge_dist, uint64_t cap, uint64_t* n_edges,
                                           char* err, uint32_t err_cap);
HS_API hs_status hs_clustering_table_apply(hs_cluster_state* st, uint32_t l, const uint32_t* edge_i,
                                           const uint32_t* edge_j, uint64_t n_edges);
HS_API hs_status hs_clustering_end(hs_cluster_state* st, uint8_t* merged, uint32_t* owner,
                                   uint32_t* absorbed_table);

#ifdef __cplusplus
}
#endif
#endif /* HSEARCH_H */
