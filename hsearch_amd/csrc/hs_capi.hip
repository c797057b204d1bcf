// hs_capi.hip -- the C ABI of include/hsearch.h on top of the gfx950 kernels (hs_kernels.hip) and
// the device primitives (hs_prims.hip).  One handle = one GPU, one stream, one index.  Here: the handle's life and
// options, embedding and hashing, the queries, the self-joins and what reduces their hits.
//
// struct hs_handle, its member types, HS_HIP / HS_CHECK and filter_passes: hs_handle.h.  The index calls
// (hs_index_*, with the HBM layout of an index): hs_capi_index.hip.  The profile calls (hs_pssm_*): hs_capi_pssm.hip.
#include <math.h>
#include <random>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/hs_tables.h"
#include "hs_handle.h"

// (declared in hs_handle.h: hs_capi_index.hip and hs_capi_pssm.hip call these too)
hs_status fail(hs_handle* h, hs_status st, const std::string& msg) {
  if (h) h->err = msg;
  return st;
}

float ev_ms(hs_handle* h, int i0, int i1) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->ev[i0], h->ev[i1]) != hipSuccess) return 0.f;
  return ms;
}

hs_status ensure_device(hs_handle* h) {
  HS_HIP(h, hipSetDevice(h->p.device));
  return HS_OK;
}

// The pinned words a pass's counter block lands in (small device -> host copies into pageable memory cost ~ 50 us
// per batch)
hs_status ensure_pin_cnt(hs_handle* h) {
  if (h->pin_cnt) return HS_OK;
  HS_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&h->pin_cnt), HS_CNT_WORDS * 4, hipHostMallocDefault));
  memset(h->pin_cnt, 0, HS_CNT_WORDS * 4);
  return HS_OK;
}

// The index is about to change (or go): nothing learnt from batches against the old one may size or
// steer batches against the new one (a stale capacity hint made the first batches after a rebuild to
// another shape run their join twice: once with the stale capacity, then again the slow way).
void drop_index(hs_handle* h) {
  h->built = false;
  h->rec8w_ready = false;
  h->rec6_state = 0;
  h->hist = {};
}

namespace {

// smallest float >= x (x >= 0), then one more ulp: the fp32 filter bound must never undercut.
float filter_bound(double r2) { return hs_filter_bound(r2); }

// Queries per batch at most: the probe numbers (query x table) carry a flag in bit 31
uint32_t max_query_batch(const hs_handle* h) { return (uint32_t)((1ull << 31) / h->p.L) - 1; }


// The device code of the library's kernels -- rocPRIM's sort / scan / run-length kernels in
// particular -- is loaded lazily, at first launch: measured 57 ms of host time inside the first
// table's sort of the first index build of a process (rocprofv3 timeline).  One launch of each
// on a few elements at handle creation moves that out of hs_index_build and out of the first query.
hs_status warm_up_device_code(hs_handle* h) {
  static bool done = false;  // per process
  if (done) return HS_OK;
  const size_t n = 64;
  DevBuf k0, k1, v0, v1, cnt, tmp;
  struct G {
    DevBuf* b[6];
    ~G() { for (DevBuf* x : b) x->release(); }
  } g = {{&k0, &k1, &v0, &v1, &cnt, &tmp}};
  HS_HIP(h, k0.reserve(n * 8));
  HS_HIP(h, k1.reserve(n * 8));
  HS_HIP(h, v0.reserve(n * 8));
  HS_HIP(h, v1.reserve(n * 8));
  HS_HIP(h, cnt.reserve((n + 2) * 4));
  const size_t tb = std::max(std::max(hs_sort_pairs_u64_u32_temp(n), hs_sort_pairs_u64_u64_temp(n)),
                             std::max(hs_rle_u64_temp(n), hs_scan_u32_temp(n))) + 256;
  HS_HIP(h, tmp.reserve(tb));
  HS_HIP(h, hipMemsetAsync(k0.p, 0, n * 8, h->stream));
  HS_HIP(h, hipMemsetAsync(v0.p, 0, n * 8, h->stream));
  HS_HIP(h, hs_sort_pairs_u64_u32(tmp.p, tmp.cap, k0.as<uint64_t>(), k1.as<uint64_t>(), v0.as<uint32_t>(),
                                  v1.as<uint32_t>(), n, 0, 64, h->stream));
  HS_HIP(h, hs_sort_pairs_u64_u64(tmp.p, tmp.cap, k0.as<uint64_t>(), k1.as<uint64_t>(), v0.as<uint64_t>(),
                                  v1.as<uint64_t>(), n, 64, h->stream));
  HS_HIP(h, hs_rle_u64(tmp.p, tmp.cap, k1.as<uint64_t>(), k0.as<uint64_t>(), v0.as<uint32_t>(),
                       cnt.as<uint32_t>(), n, h->stream));
  HS_HIP(h, hs_exclusive_scan_u32(tmp.p, tmp.cap, v0.as<uint32_t>(), v1.as<uint32_t>(), n, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  done = true;
  return HS_OK;
}

// (Re)quantise the handle's planes -- and, the first time, its coordinate table -- for the MFMA
// projection, and decide whether the auto mode uses it: the bound's typical half-width, in bucket
// units, is est = (da k max|row|_1 + dx max|a^|_1) / W; about 2 est of all values are recomputed.
hs_status setup_projection(hs_handle* h, bool table_too) {
  h->proj_usable = false;
  h->proj_auto = false;
  h->proj_S = hs_proj_steps((int)h->p.k);
  if (!h->proj_S) return HS_OK;
  const int S = h->proj_S, LK = h->LK, L = (int)h->p.L;
  const size_t tile = (size_t)S * 2 * 64 * 16;
  const size_t all_bytes = (size_t)((LK + 31) / 32) * tile, tab_bytes = (size_t)L * tile;
  HS_HIP(h, h->proj_aq_all.reserve(all_bytes));
  HS_HIP(h, h->proj_aq_tab.reserve(tab_bytes));
  HS_HIP(h, h->proj_fn.reserve((size_t)LK * 32));
  HS_HIP(h, h->proj_tab.reserve(sizeof(hs_proj_table)));
  HS_HIP(h, h->proj_stats.reserve(64));
  HS_HIP(h, h->proj_cnt.reserve(64));
  HS_HIP(h, hipMemsetAsync(h->proj_aq_all.p, 0, all_bytes, h->stream));
  HS_HIP(h, hipMemsetAsync(h->proj_aq_tab.p, 0, tab_bytes, h->stream));
  HS_HIP(h, hipMemsetAsync(h->proj_stats.p, 0, 64, h->stream));
  if (table_too)
    HS_HIP(h, hs_launch_quant_table(h->coords.as<double>(), h->alphabet, h->proj_tab.as<hs_proj_table>(), h->stream));
  HS_HIP(h, hs_launch_quant_planes(h->a.as<double>(), h->b.as<double>(), LK, h->d, (int)h->p.K, S, h->p.W,
                                   h->proj_eps_scale, h->proj_aq_all.p, h->proj_aq_tab.p, h->proj_fn.p,
                                   h->proj_stats.as<unsigned long long>(), h->stream));
  unsigned long long stats[3] = {0, 0, 0};
  hs_proj_table tab;
  HS_HIP(h, hipMemcpyAsync(stats, h->proj_stats.p, 24, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(&tab, h->proj_tab.p, sizeof(tab), hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  double da, a1;
  memcpy(&da, &stats[0], 8);
  memcpy(&a1, &stats[1], 8);
  h->proj_usable = true;
  h->proj_est = h->proj_eps_scale * (da * (double)h->p.k * tab.l1max + tab.dx * a1) / h->p.W;
  // auto: at most ~3 % of the values recomputed, every function and the table representable
  h->proj_auto = !tab.unsafe && !stats[2] && h->proj_est <= 1.0 / 64.0;
  return HS_OK;
}

inline bool use_projection(const hs_handle* h) {
  return h->proj_usable && (h->hash_mode == 2 || (h->hash_mode == 0 && h->proj_auto));
}

}  // namespace

// (hash_dispatch and hash_account are declared in hs_handle.h: the index calls hash too)
// Bucket ints of functions [f0, f0 + F) -- one whole table (table >= 0: f0 = table * K, F = K) or
// all of them (table < 0) -- for n points given as codes or as doubles, into out[i * out_stride + f - f0],
// on stream s: the MFMA pass + exact recomputation of the flagged values, or the exact kernel alone.
// set = which flag list / counter pair to use (two tables are in flight during a build).
#define HS_PROJ_SET_BATCH 3  // flag list 2 with the counter pair of the batch's counter block (HS_CNT_PROJ)
hs_status hash_dispatch(hs_handle* h, const uint8_t* d_codes, const double* d_pts, uint64_t n, int table,
                        int32_t* out, int out_stride, int set, hipStream_t s) {
  const int K = (int)h->p.K, k = (int)h->p.k;
  const int f0 = table >= 0 ? table * K : 0, F = table >= 0 ? K : h->LK;
  if (!n) return HS_OK;
  if (!use_projection(h) || n >= (1ull << 31)) {
    if (d_codes)
      HS_HIP(h, hs_launch_hash_codes(d_codes, n, k, h->aT.as<double>() + f0, h->LK, h->b.as<double>() + f0, F,
                                     h->p.W, h->coords.as<double>(), out, out_stride, s));
    else
      HS_HIP(h, hs_launch_hash_points(d_pts, n, k, h->aT.as<double>() + f0, h->LK, h->b.as<double>() + f0, F,
                                      h->p.W, out, out_stride, s));
    return HS_OK;
  }
  // the flag list's counter is 32 bits and every value may be flagged (an inflated bound, a table the
  // fixed point cannot carry): at most 0xE0000000 / F points per pass
  const uint64_t n_max = 0xE0000000ull / (uint64_t)F;
  if (n > n_max) {
    if (set == HS_PROJ_SET_BATCH) set = 2;  // (pieces count from zero each: set 2's pair, with its fill)
    for (uint64_t i0 = 0; i0 < n; i0 += n_max)
      HS_CHECK(hash_dispatch(h, d_codes ? d_codes + i0 * k : nullptr, d_pts ? d_pts + i0 * h->d : nullptr,
                             std::min(n_max, n - i0), table, out + i0 * out_stride, out_stride, set, s));
    return HS_OK;
  }
  const int S = h->proj_S;
  const size_t tile = (size_t)S * 2 * 64;  // uint4 per function tile
  const uint4* aq = table >= 0 ? h->proj_aq_tab.as<uint4>() + (size_t)table * tile : h->proj_aq_all.as<uint4>();
  const char* fn = h->proj_fn.as<char>() + (size_t)f0 * 32;
  // room for 1/32 of the values (the auto mode expects ~ 2 est <= 1/32 of them at worst) plus the
  // slack of the per-wave reservations (2 n_cu x 4 waves x 128 slots); when the list overflows the
  // fix kernel recomputes everything, which is still correct
  const uint64_t want = (uint64_t)n * (uint64_t)F / 32 + (1u << 20);
  const uint32_t cap = (uint32_t)std::min<uint64_t>(want, 1ull << 28);
  // set HS_PROJ_SET_BATCH: a search batch's queries (flag list of set 2) counting in the batch's counter block,
  // which the batch's reset has just cleared: no fill here, no copy of its own after the pass
  const bool in_block = set == HS_PROJ_SET_BATCH;
  if (in_block) set = 2;
  HS_HIP(h, h->proj_flags[set].reserve((size_t)cap * 8));
  uint32_t* cnt = in_block ? h->counters.as<uint32_t>() + HS_CNT_PROJ : h->proj_cnt.as<uint32_t>() + 2 * set;
  if (!in_block) HS_HIP(h, hipMemsetAsync(cnt, 0, 8, s));
  if (!d_codes) {
    HS_HIP(h, h->proj_xq.reserve((size_t)n * S * 64));
    HS_HIP(h, h->proj_xmeta.reserve((size_t)n * 24));
    HS_HIP(h, hs_launch_quant_points(d_pts, n, k, S, h->proj_xq.p, h->proj_xmeta.as<double>(), s));
  }
  HS_HIP(h, hs_launch_proj(d_codes, h->proj_xq.p, h->proj_xmeta.as<double>(), n, k, S, aq, fn, F,
                           h->proj_tab.as<hs_proj_table>(), h->p.W, out, out_stride,
                           h->proj_flags[set].as<uint2>(), cap, cnt, h->n_cu, s));
  HS_HIP(h, hs_launch_proj_fix(d_codes, d_pts, n, k, h->aT.as<double>() + f0, h->LK, h->b.as<double>() + f0, F,
                               h->p.W, h->coords.as<double>(), out, out_stride, h->proj_flags[set].as<uint2>(),
                               cap, cnt, s));
  return HS_OK;
}

// after a synchronisation of the stream the hash ran on: add the pass's statistics to the profile
hs_status hash_account(hs_handle* h, uint64_t n, int F, int set) {
  if (!use_projection(h) || !n || n >= (1ull << 31)) return HS_OK;
  uint32_t c[2] = {0, 0};
  // (on the handle's stream, which the callers have just drained: a plain hipMemcpy goes through the
  // process's default stream, whose first use cost 6.8 ms of a first build's 30)
  HS_HIP(h, hipMemcpyAsync(c, h->proj_cnt.as<uint32_t>() + 2 * set, 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->prof.hash_values += n * (uint64_t)F;
  h->prof.hash_flagged += c[1];
  return HS_OK;
}

namespace {

// The environment is read ONCE per handle, for diagnostics and defaults only: HS_BUILD_DEBUG / HS_CLUSTER_TIMING
// / HS_DEBUG_REFINE (prints), HS_VERIFY_MODE / HS_HASH_MODE (documented defaults of hs_set_verify_mode /
// hs_set_hash_mode), HS_OPTIONS = "name=value,..." (hs_set_option by name, for the A/B scripts under tools/),
// and -- test build of the library only -- the fault-injection hooks.  Every path selection is an hs_option.
const struct { const char* name; int option; } kOptionNames[] = {
    {"query_batch", HS_OPT_QUERY_BATCH}, {"seg_mode", HS_OPT_SEG_MODE}, {"join_resident", HS_OPT_JOIN_RESIDENT},
    {"recognise_kmers", HS_OPT_RECOGNISE_KMERS}, {"build_grouping", HS_OPT_BUILD_GROUPING}, {"wide_rows", HS_OPT_WIDE_ROWS},
    {"refine8", HS_OPT_REFINE8}, {"self_codes", HS_OPT_SELF_CODES},
    {"sort_hits", HS_OPT_SORT_HITS}, {"sync_items", HS_OPT_SYNC_ITEMS}, {"join_min_q", HS_OPT_JOIN_MIN_Q},
    {"join_min_m", HS_OPT_JOIN_MIN_M}, {"sort_from_bit", HS_OPT_SORT_FROM_BIT}, {"build_serial", HS_OPT_BUILD_SERIAL},
    {"join_xcd_run", HS_OPT_JOIN_XCD_RUN}, {"probe_records", HS_OPT_PROBE_RECORDS},
    {"join_chunk", HS_OPT_JOIN_CHUNK}, {"join_f6", HS_OPT_JOIN_F6}, {"join_f6_form", HS_OPT_JOIN_F6_FORM}, {"pssm_filter", HS_OPT_PSSM_FILTER}, {"pssm_cmp_filter", HS_OPT_PSSM_CMP_FILTER},{"pssm_topk_sample", HS_OPT_PSSM_TOPK_SAMPLE}, {"pssm_rank_sample", HS_OPT_PSSM_RANK_SAMPLE}, {"pssm_null_bins", HS_OPT_PSSM_NULL_BINS}, {"pssm_count_chunk", HS_OPT_PSSM_COUNT_CHUNK}, {"summary_chunk", HS_OPT_SUMMARY_CHUNK}, {"summary_rows", HS_OPT_SUMMARY_ROWS},
    {"msf_edge_budget", HS_OPT_MSF_EDGE_BUDGET}};

void read_knobs(hs_handle* h) {
  Knobs& kn = h->knobs;
  auto on = [](const char* name) { return getenv(name) != nullptr; };
  kn.build_debug = on("HS_BUILD_DEBUG");
  kn.cluster_timing = on("HS_CLUSTER_TIMING");
  kn.debug_refine = on("HS_DEBUG_REFINE");
#ifdef HS_TEST_HOOKS
  if (const char* m = getenv("HS_TEST_SPLIT_ABOVE")) kn.test_split_above = (uint32_t)std::max(0, atoi(m));
  kn.test_group_fallback = on("HS_TEST_GROUP_FALLBACK");
  kn.test_append_collision = on("HS_TEST_APPEND_COLLISION");
  kn.test_remove_reseed = on("HS_TEST_REMOVE_RESEED");
  kn.test_rec6_no_room = on("HS_TEST_REC6_NO_ROOM");
#endif
  if (const char* m = getenv("HS_HASH_MODE")) {
    if (!strcmp(m, "exact")) h->hash_mode = 1;
    if (!strcmp(m, "mfma")) h->hash_mode = 2;
  }
  if (const char* m = getenv("HS_VERIFY_MODE")) {
    if (!strcmp(m, "stream")) h->verify_mode = 1;
    if (!strcmp(m, "join")) h->verify_mode = 2;
    if (!strcmp(m, "join16")) h->verify_mode = 3;
  }
  if (const char* m = getenv("HS_OPTIONS")) {
    std::string all(m);
    for (size_t at = 0; at < all.size();) {
      const size_t end = std::min(all.find(',', at), all.size());
      const std::string item = all.substr(at, end - at);
      at = end + 1;
      const size_t eq = item.find('=');
      if (eq == std::string::npos) continue;
      for (const auto& o : kOptionNames)
        if (item.substr(0, eq) == o.name) (void)hs_set_option(h, o.option, atoll(item.c_str() + eq + 1));
    }
  }
}

}  // namespace

extern "C" {

#ifdef HS_TEST_HOOKS
const char* hs_version(void) { return "hsearch_amd 0.3 (gfx950, test hooks)"; }
#else
const char* hs_version(void) { return "hsearch_amd 0.3 (gfx950)"; }
#endif
const char* hs_last_error(const hs_handle* h) { return h ? h->err.c_str() : "null handle"; }

hs_status hs_get_profile(const hs_handle* h, hs_profile* out) {
  if (!h || !out) return HS_ERR_INVALID;
  *out = h->prof;
  return HS_OK;
}

hs_status hs_get_params(const hs_handle* h, hs_params* out) {
  if (!h || !out) return HS_ERR_INVALID;
  *out = h->p;
  out->alphabet = (uint32_t)h->alphabet;
  return HS_OK;
}

uint32_t hs_key_string(const int32_t* buckets, uint32_t K, char* out, uint32_t cap) {
  if (K > HS_MAX_K) K = HS_MAX_K;
  char tmp[HS_KEY_CHARS];
  int n = hs_key_chars(buckets, (int)K, tmp);
  if (cap) {
    uint32_t m = std::min<uint32_t>((uint32_t)n, cap - 1);
    memcpy(out, tmp, m);
    out[m] = 0;
  }
  return (uint32_t)n;
}

uint64_t hs_key_fingerprint(const int32_t* buckets, uint32_t K, uint32_t seed) {
  return hs_key_of(buckets, (int)std::min<uint32_t>(K, HS_MAX_K), seed);
}

int hs_key_strings_equal(const int32_t* x, const int32_t* y, uint32_t K) {
  return hs_key_equal(x, y, (int)std::min<uint32_t>(K, HS_MAX_K)) ? 1 : 0;
}

#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
static void hs_abort_backtrace(int) {
  void* frames[64];
  (void)!write(2, "HS ABORT\n", 9);
  const int nf = backtrace(frames, 64);
  backtrace_symbols_fd(frames, nf, 2);
  _exit(134);
}

hs_status hs_create(const hs_params* params, const double* a, const double* b, const double* coords,
                    hs_handle** out) {
  if (!out) return HS_ERR_INVALID;
  *out = nullptr;
  if (!params || !a || !b) return HS_ERR_INVALID;
  if (params->k < 1 || params->k > 75 || params->K < 1 || params->K > HS_MAX_K || params->L < 1 ||
      params->L > HS_MAX_L || !(params->W > 0.0) || !isfinite(params->W) ||
      params->alphabet > HS_ALPHABET_PAD || (params->alphabet && !coords))
    return HS_ERR_INVALID;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || params->device < 0 ||
      params->device >= n_dev)
    return HS_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, params->device) != hipSuccess) return HS_ERR_NO_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return HS_ERR_NO_DEVICE;  // CDNA4 code objects only
  hs_handle* h = new hs_handle();
  h->p = *params;
  h->d = 8 * (int)params->k;
  h->LK = (int)(params->L * params->K);
  h->PW = hs_packed_words((int)params->k);
  h->alphabet = params->alphabet ? (int)params->alphabet : HS_ALPHABET;
  h->n_cu = prop.multiProcessorCount;
  memset(&h->tabs, 0, sizeof(h->tabs));
  memset(&h->info, 0, sizeof(h->info));
  memset(&h->prof, 0, sizeof(h->prof));
  *out = h;  // returned even on failure below so the caller can read hs_last_error, then destroy
  HS_HIP(h, hipSetDevice(params->device));
  HS_HIP(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  for (int i = 0; i < EV_COUNT; ++i) HS_HIP(h, hipEventCreate(&h->ev[i]));
  h->ev_ok = true;
  {
    // lowest priority: the runtime keeps a separate pool of hardware queues per priority level, so
    // the side stream never shares a queue with the main stream (with the default 4 queues and a
    // few more streams in the process -- torch's, RCCL's -- two normal-priority streams can land on
    // the same hardware queue, and the streaming filter would then run AFTER the join instead of
    // beside it); it is also the right order of service
    int least = 0, greatest = 0;
    HS_HIP(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HS_HIP(h, hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, least));
  }
  for (int i = 0; i < EVX_COUNT; ++i)
    HS_HIP(h, hipEventCreateWithFlags(&h->evx[i], hipEventDisableTiming));
  h->evx_ok = true;
  const size_t na = (size_t)h->LK * h->d;
  HS_HIP(h, h->a.reserve(na * 8));
  HS_HIP(h, h->b.reserve((size_t)h->LK * 8));
  HS_HIP(h, h->coords.reserve(HS_ALPHABET_PAD * 8 * 8));
  HS_HIP(h, hipMemsetAsync(h->coords.p, 0, HS_ALPHABET_PAD * 8 * 8, h->stream));
  HS_HIP(h, hipMemcpyAsync(h->a.p, a, na * 8, hipMemcpyHostToDevice, h->stream));
  // the hash kernels read the planes dimension-major: aT[i][f], f = l * K + k
  HS_HIP(h, h->aT.reserve(na * 8));
  HS_HIP(h, hs_launch_transpose_f64(h->a.as<double>(), h->LK, h->d, h->aT.as<double>(), h->stream));
  HS_HIP(h, hipMemcpyAsync(h->b.p, b, (size_t)h->LK * 8, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipMemcpyAsync(h->coords.p, coords ? coords : &HS_AA_COORDS[0][0],
                           (size_t)h->alphabet * 8 * 8, hipMemcpyHostToDevice, h->stream));
  // fp16 coordinate table + row norms of the bucket-join filter
  HS_HIP(h, h->jtab.reserve(512 + 128 + 64));
  HS_HIP(h, hipMemsetAsync(h->jtab.p, 0, 512 + 128 + 64, h->stream));
  HS_HIP(h, hs_launch_jtables(h->coords.as<double>(), h->alphabet, h->jtab.p,
                              reinterpret_cast<float*>(h->jtab.as<char>() + 512),
                              reinterpret_cast<uint32_t*>(h->jtab.as<char>() + 640), h->stream));
  uint32_t unsafe = 1;
  HS_HIP(h, hipMemcpyAsync(&unsafe, h->jtab.as<char>() + 640, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->join_tables_ok = (unsafe == 0);
  // int8 table {x^ packed, |x1|^2, L1(x^)} x 32 at bytes 0..511, scale {s, s^2/2} at 512, flag at 640
  // ... refinement table {x^ 0..3, x^ 4..7, |x|^2, L1s} x 32 at bytes 1024..1535, scale[2..3] = its s, ok
  HS_HIP(h, h->jtab8.reserve(2048));
  HS_HIP(h, hipMemsetAsync(h->jtab8.p, 0, 2048, h->stream));
  // ... the 8-column one-scale table of the wide rows (short k-mers) at bytes 1536..2047, scale[4..6]
  HS_HIP(h, hs_launch_jtables8(h->coords.as<double>(), h->alphabet, h->jtab8.p, h->jtab8.as<float>() + 128,
                               reinterpret_cast<uint32_t*>(h->jtab8.as<char>() + 640),
                               h->jtab8.as<char>() + 1024, h->jtab8.as<char>() + 1536, h->stream));
  // the FP6 join's tables (hs_join6_tables.h); their last word says whether the table has a usable scale
  HS_HIP(h, h->jtab6.reserve(hs_join6_table_bytes()));
  HS_HIP(h, hipMemsetAsync(h->jtab6.p, 0, hs_join6_table_bytes(), h->stream));
  HS_HIP(h, hs_launch_jtables6(h->coords.as<double>(), h->alphabet, h->jtab6.p, h->stream));
  int32_t ok6 = 0;
  HS_HIP(h, hipMemcpyAsync(&ok6, h->jtab6.as<char>() + hs_join6_ok_offset(), 4, hipMemcpyDeviceToHost, h->stream));
  uint32_t unsafe8 = 1;
  float scale8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  HS_HIP(h, hipMemcpyAsync(&unsafe8, h->jtab8.as<char>() + 640, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(scale8, h->jtab8.as<char>() + 512, 32, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->join8_tables_ok = (unsafe8 == 0);
  h->join6_tables_ok = ok6 != 0;
  // Short k-mers: R^2 is not far below the 4-column distance of bucket mates any more (k = 15: the
  // 4-column bound passes 4 % of random pairs), so their rows carry all 8 columns (hs_join8.hip)
  if (getenv("HS_BACKTRACE")) signal(SIGABRT, hs_abort_backtrace);
  h->wide8_ok = h->join8_tables_ok && scale8[6] > 0.f;
  h->wide8 = h->wide8_ok && (int)h->p.k <= 20;  // (hs_set_option(HS_OPT_WIDE_ROWS, 3): never)
  h->join8_scale = (double)scale8[0];
  h->join8_scale_w = (double)scale8[4];
  {  // mean and variance of the 4-column squared distance of two uniformly drawn residues (want_wide)
    const double* ct = coords ? coords : &HS_AA_COORDS[0][0];
    const int A = h->alphabet;
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < A; ++i)
      for (int j = 0; j < A; ++j) {
        double d = 0.0;
        for (int c = 0; c < 4; ++c) d += (ct[i * 8 + c] - ct[j * 8 + c]) * (ct[i * 8 + c] - ct[j * 8 + c]);
        s1 += d;
        s2 += d * d;
      }
    h->pair4_mean = s1 / ((double)A * A);
    h->pair4_var = std::max(0.0, s2 / ((double)A * A) - h->pair4_mean * h->pair4_mean);
  }
  read_knobs(h);
  HS_CHECK(setup_projection(h, true));
  HS_CHECK(warm_up_device_code(h));
  return HS_OK;
}

hs_status hs_set_planes(hs_handle* h, const double* a, const double* b) {
  if (!h || !a || !b) return HS_ERR_INVALID;
  hs_status st = ensure_device(h);
  if (st) return st;
  drop_index(h);  // the tables were keyed by the old family
  const size_t na = (size_t)h->LK * h->d;
  // the previous family may still be read by work queued on the stream: order the copies after it
  HS_HIP(h, hipMemcpyAsync(h->a.p, a, na * 8, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hs_launch_transpose_f64(h->a.as<double>(), h->LK, h->d, h->aT.as<double>(), h->stream));
  HS_HIP(h, hipMemcpyAsync(h->b.p, b, (size_t)h->LK * 8, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));  // a, b are the caller's again
  return setup_projection(h, false);
}

hs_status hs_set_hash_mode(hs_handle* h, int mode, double eps_scale) {
  if (!h || mode < 0 || mode > 2 || !(eps_scale >= 1.0) || !(eps_scale < 1e12)) return HS_ERR_INVALID;
  hs_status st = ensure_device(h);
  if (st) return st;
  h->hash_mode = mode;
  if (eps_scale != h->proj_eps_scale) {
    h->proj_eps_scale = eps_scale;
    HS_HIP(h, hipStreamSynchronize(h->stream));
    if (h->stream2) HS_HIP(h, hipStreamSynchronize(h->stream2));
    return setup_projection(h, false);
  }
  return HS_OK;
}

hs_status hs_set_verify_mode(hs_handle* h, int mode) {
  if (!h || mode < 0 || mode > 3) return HS_ERR_INVALID;
  h->verify_mode = mode;
  return HS_OK;
}

hs_status hs_set_bucket_partition(hs_handle* h, uint32_t part, uint32_t n_parts) {
  if (!h) return HS_ERR_INVALID;
  if (!n_parts || part >= n_parts || n_parts > 65536u)
    return fail(h, HS_ERR_INVALID, "hs_set_bucket_partition: part < n_parts, 1 <= n_parts <= 65536");
  h->bucket_part = part;
  h->bucket_parts = n_parts;
  return HS_OK;
}

hs_status hs_set_option(hs_handle* h, int option, int64_t value) {
  if (!h) return HS_ERR_INVALID;
  Knobs& kn = h->knobs;
  auto flag = [&](bool* dst, bool invert) -> hs_status {
    if (value != 0 && value != 1) return fail(h, HS_ERR_INVALID, "hs_set_option: the option takes 0 or 1");
    *dst = invert ? value == 0 : value == 1;
    return HS_OK;
  };
  switch (option) {
    case HS_OPT_QUERY_BATCH:
      if (value < 0 || value >= (1ll << 27) || value > (int64_t)max_query_batch(h)) break;
      kn.query_batch = (uint32_t)value;
      return HS_OK;
    case HS_OPT_SEG_MODE:
      if (value < 0 || value > 2) break;
      kn.seg_mode = (int)value;
      return HS_OK;
    case HS_OPT_JOIN_RESIDENT:
      if (value < 0 || value > 2) break;
      kn.no_join_r = value == 1;
      kn.force_join_r = value == 2;
      return HS_OK;
    case HS_OPT_RECOGNISE_KMERS: return flag(&kn.no_recognise, true);
    case HS_OPT_BUILD_GROUPING: return flag(&kn.build_sort, false);
    case HS_OPT_WIDE_ROWS: {
      if (value < 0 || value > 3) break;
      kn.force_wide = value == 1;
      kn.no_wide_by_radius = value >= 2;
      // 3: the 4-column rows for short k-mers too -- the index's member records are built for one form
      const bool wide8 = h->wide8_ok && (int)h->p.k <= 20 && value != 3;
      if (wide8 != h->wide8) {
        drop_index(h);
        h->wide8 = wide8;
      }
      return HS_OK;
    }
    case HS_OPT_REFINE8: return flag(&kn.no_refine8, true);
    case HS_OPT_JOIN_F6: return flag(&kn.no_join_f6, true);
    case HS_OPT_JOIN_F6_FORM:
      if (value < -1 || value > 1) break;
      kn.join_f6_form = (int)value;
      return HS_OK;
    case HS_OPT_PSSM_FILTER: return flag(&kn.no_pssm_filter, true);
    case HS_OPT_PSSM_CMP_FILTER: return flag(&kn.no_pssm_cmp_filter, true);
    case HS_OPT_PSSM_TOPK_SAMPLE:
      if (value < 1 || value > 0xffffffffll) break;
      kn.pssm_topk_sample = (uint32_t)value;
      return HS_OK;
    case HS_OPT_PSSM_RANK_SAMPLE:
      if (value < 1 || value > 0xffffffffll) break;
      kn.pssm_rank_sample = (uint32_t)value;
      return HS_OK;
    case HS_OPT_PSSM_NULL_BINS:
      if (value < 64 || value > 8192) break;
      kn.pssm_null_bins = (uint32_t)value;
      return HS_OK;
    case HS_OPT_PSSM_COUNT_CHUNK:
      if (value < 0 || value > (1ll << 20)) break;
      kn.pssm_count_chunk = (uint32_t)value;
      return HS_OK;
    case HS_OPT_SELF_CODES: return flag(&kn.no_self_codes, true);
    case HS_OPT_SORT_HITS: return flag(&kn.sort_hits, false);
    case HS_OPT_SYNC_ITEMS: return flag(&kn.sync_items, false);
    case HS_OPT_JOIN_MIN_Q:
      if (value < 1 || value > (1ll << 30)) break;
      h->join_min_q = (uint32_t)value;
      return HS_OK;
    case HS_OPT_JOIN_MIN_M:
      if (value < 1 || value > (1ll << 30)) break;
      h->join_min_m = (uint32_t)value;
      return HS_OK;
    case HS_OPT_SORT_FROM_BIT:
      if (value < 0 || value > 60) break;
      kn.sort_from_bit = (int)value;
      return HS_OK;
    case HS_OPT_BUILD_SERIAL: return flag(&kn.build_serial, false);
    case HS_OPT_PROBE_RECORDS: return flag(&kn.no_probe_records, true);
    case HS_OPT_JOIN_CHUNK:
      if (value != 0 && (value < 2 || value > 64)) break;
      kn.join_chunk = (uint32_t)value;
      return HS_OK;
    case HS_OPT_SUMMARY_CHUNK:
      if (value < 0 || value > (1ll << 20)) break;
      kn.summary_chunk = (uint32_t)value;
      return HS_OK;
    case HS_OPT_SUMMARY_ROWS:
      if (value < 0 || value >= (1ll << 31)) break;
      kn.summary_rows = (uint32_t)value;
      return HS_OK;
    case HS_OPT_MSF_EDGE_BUDGET:
      if (value < -1) break;
      kn.msf_edge_budget = value;
      return HS_OK;
    case HS_OPT_JOIN_XCD_RUN:
      if (value < -1 || value > 4096 || (value > 0 && (value & (value - 1)))) break;  // a power of two
      kn.join_xcd_run = (int)value;
      return HS_OK;
    default:
      return fail(h, HS_ERR_INVALID, "hs_set_option: unknown option");
  }
  return fail(h, HS_ERR_INVALID, "hs_set_option: value out of range");
}

hs_status hs_wait_event(hs_handle* h, void* hip_event) {
  if (!h || !hip_event) return HS_ERR_INVALID;
  hs_status st = ensure_device(h);
  if (st) return st;
  HS_HIP(h, hipStreamWaitEvent(h->stream, reinterpret_cast<hipEvent_t>(hip_event), 0));
  return HS_OK;
}

void hs_destroy(hs_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->p.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  DevBuf* bufs[] = {&h->a, &h->aT, &h->b, &h->coords, &h->codes, &h->packed_all, &h->qints, &h->qstart,
                    &h->qcount, &h->nslices, &h->slice_off, &h->tq, &h->prov, &h->hit_key,
                    &h->hit_val, &h->hit_key2, &h->hit_val2, &h->counters, &h->temp,
                    &h->io_centers, &h->io_q, &h->io_id, &h->io_table, &h->io_dist, &h->io_cand,
                    &h->io_codes, &h->io_misc, &h->jtab, &h->c16, &h->seg_keys, &h->seg_keys_sorted,
                    &h->seg_vals, &h->sorted_ql, &h->seg_key, &h->seg_cnt, &h->seg_qoff,
                    &h->seg_items, &h->item_off, &h->seg_n, &h->c16s, &h->item_desc,
                    &h->probe_slow, &h->jtab8, &h->c8b, &h->prov2, &h->t_packed, &h->t_rec8, &h->t_rec8w, &h->jtab6, &h->t_rec6, &h->t_pos, &h->dir_base,
                    &h->bucket_work, &h->proj_aq_all, &h->proj_aq_tab, &h->proj_fn, &h->proj_tab, &h->proj_stats,
                    &h->proj_flags[0], &h->proj_flags[1], &h->proj_flags[2], &h->proj_cnt, &h->proj_xq,
                    &h->proj_xmeta, &h->qhits, &h->bs_ints2[0], &h->bs_ints2[1], &h->bs_keys2[0],
                    &h->bs_keys2[1], &h->bs_iota2[0], &h->bs_iota2[1], &h->bs_keys_sorted, &h->bs_rle_unique,
                    &h->bs_rle_counts, &h->bs_small, &h->bs_sort_temp, &h->bs_slow_q, &h->all_codes,
                    &h->subset_ids, &h->qcodes_buf, &h->qembed, &h->seg_res, &h->seg_of, &h->t_rho, &h->rec_codes, &h->qpacked, &h->hit_rank, &h->hit_kv, &h->bs_fptab, &h->bs_blk,
                    &h->bs_dk, &h->bs_hist, &h->bs_rank, &h->mp_pts, &h->mp_codes, &h->mp_ints, &h->mp_frac,
                    &h->mp_vints, &h->mp_valid, &h->mp_rows, &h->mp_q, &h->mp_id, &h->mp_table, &h->mp_dist,
                    &h->mp_cand, &h->mp_radii, &h->io_radii, &h->ann_dist, &h->ann_tq, &h->ann_touched,
                    &h->ann_sorted, &h->ann_cnt, &h->cc_parent, &h->cc_cnt, &h->cc_label,
                    &h->db_deg, &h->db_anchor, &h->db_cnt, &h->msf_comp, &h->msf_best_d, &h->msf_best_pair,
                    &h->msf_out_pair, &h->msf_out_d, &h->msf_s_pair, &h->msf_s_d, &h->msf_cnt, &h->msf_kept, &h->dt_core, &h->dt_thr,
                    &h->dt_next, &h->dt_cnt, &h->knn_cnt, &h->knn_off, &h->knn_cur, &h->knn_total, &h->knn_io_count, &h->pt_tused, &h->pt_parts,
                    &h->pr_keys, &h->pr_off, &h->pr_state, &h->pr_resolved, &h->pr_tscan, &h->pr_unres, &h->pr_rank, &h->pr_out,
                    &h->pc_m, &h->pc_id, &h->pc_m2, &h->pc_id2, &h->pc_start, &h->pc_nitem, &h->pc_off, &h->pc_rows, &h->pc_out,
                    &h->pw_u, &h->pw_counts, &h->pw_out,
                    &h->pcm_xq, &h->pcm_yq, &h->pcm_xpar, &h->pcm_ypar, &h->pcm_y,
                    &h->sq_key, &h->sq_idx, &h->sq_skey, &h->sq_sidx, &h->sq_head, &h->sq_excl, &h->sq_part, &h->sq_acc,
                    &h->sq_fin, &h->sq_chk, &h->sq_in, &h->sq_out,
                    &h->pf_sidx, &h->pf_start, &h->pf_rows, &h->pf_keep, &h->pf_pos, &h->pf_in,
                    &h->pch_state, &h->pch_rows,
                    &h->sm_size, &h->sm_tmp, &h->sm_row_of, &h->sm_off_of,
                    &h->sm_row_label, &h->sm_row_off, &h->sm_member, &h->sm_d2, &h->sm_err, &h->sm_counts,
                    &h->sm_io_label, &h->sm_io_a, &h->sm_io_b, &h->sm_io_counts, &h->sm_io_f64, &h->sm_io_f64b};
  for (DevBuf* bf : bufs) bf->release();
  h->sj_host.release();
  h->t_dirjump.release();
  h->t_dirrec.release();
  h->part_work.release();
  h->t_giant.release();
  for (int l = 0; l < HS_MAX_L; ++l) {
    h->t_dirkey[l].release();
    h->t_dirstart[l].release();
    h->t_dirtuple[l].release();
    h->t_ids[l].release();
  }
  if (h->pin_cnt) (void)hipHostFree(h->pin_cnt);
  if (h->ev_ok)
    for (int i = 0; i < EV_COUNT; ++i) (void)hipEventDestroy(h->ev[i]);
  if (h->evx_ok)
    for (int i = 0; i < EVX_COUNT; ++i) (void)hipEventDestroy(h->evx[i]);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// ------------------------------------------------------------------------------ embed / hash
hs_status hs_embed_codes(hs_handle* h, const uint8_t* codes, uint64_t n, double* out) {
  if (!h || (n && (!codes || !out))) return HS_ERR_INVALID;
  if (!n) return HS_OK;
  for (uint64_t i = 0; i < n * h->p.k; ++i)
    if (codes[i] >= h->alphabet) return fail(h, HS_ERR_INVALID, "residue code outside the alphabet");
  hs_status st = ensure_device(h);
  if (st) return st;
  const size_t out_bytes = (size_t)n * h->d * 8;
  HS_HIP(h, h->io_codes.reserve((size_t)n * h->p.k));
  HS_HIP(h, h->io_misc.reserve(out_bytes));
  HS_HIP(h, hipMemcpyAsync(h->io_codes.p, codes, (size_t)n * h->p.k, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hs_launch_embed(h->io_codes.as<uint8_t>(), n, (int)h->p.k, h->coords.as<double>(),
                            h->io_misc.as<double>(), h->stream));
  HS_HIP(h, hipMemcpyAsync(out, h->io_misc.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

hs_status hs_hash_codes(hs_handle* h, const uint8_t* codes, uint64_t n, int32_t* buckets) {
  if (!h || (n && (!codes || !buckets))) return HS_ERR_INVALID;
  if (!n) return HS_OK;
  for (uint64_t i = 0; i < n * h->p.k; ++i)
    if (codes[i] >= h->alphabet) return fail(h, HS_ERR_INVALID, "residue code outside the alphabet");
  hs_status st = ensure_device(h);
  if (st) return st;
  const size_t out_bytes = (size_t)n * h->LK * 4;
  HS_HIP(h, h->io_codes.reserve((size_t)n * h->p.k));
  HS_HIP(h, h->io_misc.reserve(out_bytes));
  HS_HIP(h, hipMemcpyAsync(h->io_codes.p, codes, (size_t)n * h->p.k, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  HS_CHECK(hash_dispatch(h, h->io_codes.as<uint8_t>(), nullptr, n, -1, h->io_misc.as<int32_t>(), h->LK, 2,
                         h->stream));
  HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  HS_HIP(h, hipMemcpyAsync(buckets, h->io_misc.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  memset(&h->prof, 0, sizeof(h->prof));
  h->prof.ms_hash = h->prof.ms_total = ev_ms(h, 0, 1);
  return hash_account(h, n, h->LK, 2);
}

hs_status hs_hash_points(hs_handle* h, const double* points, uint64_t n, int32_t* buckets) {
  if (!h || (n && (!points || !buckets))) return HS_ERR_INVALID;
  if (!n) return HS_OK;
  hs_status st = ensure_device(h);
  if (st) return st;
  const size_t in_bytes = (size_t)n * h->d * 8, out_bytes = (size_t)n * h->LK * 4;
  HS_HIP(h, h->io_centers.reserve(in_bytes));
  HS_HIP(h, h->io_misc.reserve(out_bytes));
  HS_HIP(h, hipMemcpyAsync(h->io_centers.p, points, in_bytes, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  HS_CHECK(hash_dispatch(h, nullptr, h->io_centers.as<double>(), n, -1, h->io_misc.as<int32_t>(), h->LK, 2,
                         h->stream));
  HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  HS_HIP(h, hipMemcpyAsync(buckets, h->io_misc.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  memset(&h->prof, 0, sizeof(h->prof));
  h->prof.ms_hash = h->prof.ms_total = ev_ms(h, 0, 1);
  return hash_account(h, n, h->LK, 2);
}

// bits of a sorted position inside one table (segment keys: hs_launch_seg_keys)
static inline int seg_shift_of(const hs_handle* h) {
  return std::max(1, bit_width_u32((uint32_t)std::min<uint64_t>(h->n, 0xffffffffull)));
}

// Segments -> work items of jm members x <= 2048 queries: routing (join or streaming), the item
// numbering order (many-query segments first), item offsets.  Workspace reuse: seg_keys = the class flags (two
// to a 64-bit word), seg_res = their scan, seg_vals = order, seg_keys_sorted = item counts in that order (all free
// by now).  max_q_res > 0: segments with at most that many probing queries form the item list's tail, whose bounds
// hs_launch_item_desc leaves in seg_n[2..3] (hs_join8r_kernel's share) from the scan's last word.
// clear_slices: the probes wrote slice counts although every segment is joined (bucket partition): cleared here.
static hs_status cut_items(hs_handle* h, uint32_t nql, uint32_t jm, unsigned long long* d_jstats,
                           uint32_t max_q_res, uint32_t n_probes, bool clear_slices, uint32_t jm_stream = 0) {
  const size_t n1 = (size_t)nql + 1;
  // every segment with a member goes to the join (the default): no probe keeps a slice for the streaming filter
  const bool all_joined = h->join_min_q == 1 && h->join_min_m == 1;
  uint64_t* cls = h->seg_keys.as<uint64_t>();
  HS_HIP(h, h->seg_res.reserve(n1 * 8));
  uint64_t* cls_pos = h->seg_res.as<uint64_t>();
  uint32_t* order = h->seg_vals.as<uint32_t>();
  uint32_t* items_ord = h->seg_keys_sorted.as<uint32_t>();
  HS_HIP(h, hs_launch_seg_route(h->seg_key.as<uint64_t>(), h->seg_cnt.as<uint32_t>(),
                                h->seg_qoff.as<uint32_t>(), h->seg_n.as<uint32_t>(),
                                h->sorted_ql.as<uint32_t>(), h->qcount.as<uint32_t>(), nql,
                                h->join_min_q, h->join_min_m, jm, (int)h->p.L, seg_shift_of(h), max_q_res, 512u,
                                h->seg_items.as<uint32_t>(), cls, d_jstats,
                                all_joined ? nullptr : h->nslices.as<uint32_t>(), h->seg_of.as<uint32_t>(), h->stream,
                                jm_stream));
  if (all_joined && clear_slices) HS_HIP(h, hipMemsetAsync(h->nslices.p, 0, (size_t)n_probes * 4, h->stream));
  HS_HIP(h, hs_exclusive_scan_u64(h->temp.p, h->temp.cap, cls, cls_pos, n1, h->stream));
  HS_HIP(h, hs_launch_seg_order(cls_pos, h->seg_items.as<uint32_t>(), nql, order, items_ord, h->stream));
  HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, items_ord, h->item_off.as<uint32_t>(), n1,
                                  h->stream));
  return HS_OK;
}

// the tables as the probe kernel gets them: without the directory records when the option says so
static hs_tables_dev probe_tabs(const hs_handle* h, const QueryCall& c, uint32_t q_first,
                                const uint32_t* probe_list = nullptr, uint32_t n_list = 0) {
  hs_tables_dev t = h->tabs;
  t.q_first = q_first;
  t.probe_list = probe_list;
  t.n_list = n_list;
  if (h->knobs.no_probe_records)
    for (int l = 0; l < HS_MAX_L; ++l) t.t[l].dir_rec = nullptr;
  t.part = c.self_first == HS_NO_SELF ? h->bucket_part : 0u;  // (searches only, not the self-joins)
  t.n_parts = c.self_first == HS_NO_SELF ? h->bucket_parts : 1u;
  t.probe_valid = c.pre_valid;
  return t;
}

// ---- KLSH pre-grouping ------------------------------------------------------
hs_status hs_klsh_draw_planes(uint32_t feat, uint32_t bits, double sigma, double* w, double* b,
                              double* t) {
  if (!feat || !bits || bits > 64 || !w || !b || !t) return HS_ERR_INVALID;
  // KLSH's members in declaration order (lsh.hpp:37-49): three distributions, then the engine,
  // default-seeded; the constructor body draws t, b, then the feat normals of each bit (:28-37)
  std::normal_distribution<double> normal(0.0, sigma * sigma);  // sigma^2 as the std deviation, :22
  std::uniform_real_distribution<double> uniform_1(-1.0, 1.0);
  std::uniform_real_distribution<double> uniform_pi(0.0, 2.0 * M_PI);
  std::default_random_engine generator;
  for (uint32_t i = 0; i < bits; ++i) {
    t[i] = uniform_1(generator);
    b[i] = uniform_pi(generator);
    for (uint32_t j = 0; j < feat; ++j) w[(size_t)i * feat + j] = normal(generator);
  }
  return HS_OK;
}

hs_status hs_klsh_codes(int device, const uint8_t* classes, uint64_t n_residues,
                        const uint64_t* seq_start, uint64_t n_seq, const double* w, const double* b,
                        const double* t, uint32_t bits, uint64_t* codes, uint64_t* uncertain, char* err,
                        uint32_t err_cap) {
  auto say = [&](hs_status st, const std::string& msg) {
    if (err && err_cap) {
      strncpy(err, msg.c_str(), err_cap - 1);
      err[err_cap - 1] = 0;
    }
    return st;
  };
  if ((n_seq && (!seq_start || !codes)) || (n_residues && !classes) || !w || !b || !t || !bits || bits > 64)
    return say(HS_ERR_INVALID, "bad argument");
  if (!n_seq) return HS_OK;
  for (uint64_t s = 0; s < n_seq; ++s)
    if (seq_start[s] > seq_start[s + 1] || seq_start[s + 1] > n_residues)
      return say(HS_ERR_INVALID, "seq_start must be ascending and end within n_residues");
  for (uint64_t i = 0; i < n_residues; ++i)
    if (classes[i] >= HS_KLSH_CLASSES) return say(HS_ERR_INVALID, "residue class outside 0..7");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
    return say(HS_ERR_NO_DEVICE, "no usable gfx950 device");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return say(HS_ERR_NO_DEVICE, "no usable gfx950 device");
#define HS_KL(expr)                                                                          \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return say(e_ == hipErrorOutOfMemory ? HS_ERR_NOMEM : HS_ERR_HIP,                      \
                 std::string(#expr) + ": " + hipGetErrorString(e_));                         \
  } while (0)
  HS_KL(hipSetDevice(device));
  DevBuf d_cls, d_start, d_w, d_b, d_t, d_codes, d_unc;
  struct Guard {
    DevBuf* bufs[7];
    ~Guard() { for (DevBuf* x : bufs) x->release(); }
  } guard = {{&d_cls, &d_start, &d_w, &d_b, &d_t, &d_codes, &d_unc}};
  HS_KL(d_cls.reserve(std::max<size_t>(16, (size_t)n_residues)));
  HS_KL(d_start.reserve(((size_t)n_seq + 1) * 8));
  HS_KL(d_w.reserve((size_t)bits * HS_KLSH_FEATURES * 8));
  HS_KL(d_b.reserve((size_t)bits * 8));
  HS_KL(d_t.reserve((size_t)bits * 8));
  HS_KL(d_codes.reserve((size_t)n_seq * 8));
  HS_KL(d_unc.reserve((size_t)n_seq * 8));
  if (n_residues) HS_KL(hipMemcpy(d_cls.p, classes, (size_t)n_residues, hipMemcpyHostToDevice));
  HS_KL(hipMemcpy(d_start.p, seq_start, ((size_t)n_seq + 1) * 8, hipMemcpyHostToDevice));
  HS_KL(hipMemcpy(d_w.p, w, (size_t)bits * HS_KLSH_FEATURES * 8, hipMemcpyHostToDevice));
  HS_KL(hipMemcpy(d_b.p, b, (size_t)bits * 8, hipMemcpyHostToDevice));
  HS_KL(hipMemcpy(d_t.p, t, (size_t)bits * 8, hipMemcpyHostToDevice));
  HS_KL(hs_launch_klsh(d_cls.as<uint8_t>(), d_start.as<uint64_t>(), n_seq, d_w.as<double>(),
                       d_b.as<double>(), d_t.as<double>(), bits, d_codes.as<uint64_t>(),
                       d_unc.as<uint64_t>(), nullptr));
  HS_KL(hipDeviceSynchronize());
  HS_KL(hipMemcpy(codes, d_codes.p, (size_t)n_seq * 8, hipMemcpyDeviceToHost));
  if (uncertain) HS_KL(hipMemcpy(uncertain, d_unc.p, (size_t)n_seq * 8, hipMemcpyDeviceToHost));
#undef HS_KL
  return HS_OK;
}

// ------------------------------------------------------------------------------------- query
// Where a batch's ordered hits go (run_query's output arrays from its running total on) when the
// batch orders them itself (hs_launch_hit_order); ordered = true on return if it did.
struct BatchOut {
  uint32_t *q = nullptr, *id = nullptr, *table = nullptr;
  double* dist = nullptr;
  uint64_t room = 0;   // entries left in the arrays
  bool ordered = false;
};

// Wide int8 rows (all 8 coordinate columns) for this call?  Always for short k-mers (the index's
// member records are wide then).  For k = 21..25 when the radius is large for the k-mer length: the
// 4-column squared distance of two random k-mers is ~ N(k m, k v) (m, v: one residue pair), and once
// R^2 comes within 3 standard deviations of its mean the 4-column bound passes > 1e-3 of the bucket
// mates -- the survivor path, not the matrix pipe, then sets the pace (k = 25, R = 50: 1 % pass).
static bool want_wide(const hs_handle* h, double R) {
  if (h->wide8) return true;
  if (!h->wide8_ok || h->p.k > 25 || h->knobs.no_wide_by_radius) return false;
  if (h->knobs.force_wide) return true;
  const double k = (double)h->p.k, sd = sqrt(k * h->pair4_var);
  return R * R > k * h->pair4_mean - 3.0 * sd;
}

// The wide rows' member records for k = 21..25 (16 bytes per entry and table), built on first use
static hs_status ensure_rec8w(hs_handle* h) {
  if (h->wide8 || h->rec8w_ready) return HS_OK;
  const size_t n = h->n;
  const int L = (int)h->p.L;
  HS_HIP(h, h->t_rec8w.reserve(((size_t)L * n + HS_JM_WAVE) * 16));
  for (int l = 0; l < L; ++l)
    HS_HIP(h, hs_launch_gather_rec8(h->packed_all.as<uint4>(), h->tabs.t[l].ids, (uint32_t)n, (int)h->p.k, 1,
                                    h->jtab8.p, h->jtab8.as<char>() + 1536, h->jtab8.as<float>() + 128,
                                    nullptr, h->t_rec8w.as<uint4>() + (size_t)l * n, nullptr, h->stream));
  h->rec8w_ready = true;
  return HS_OK;
}

// The FP6 join's member records, built on the first batch that can use them.  false: no room for them (the
// error is cleared; the index keeps the int8 join)
static bool ensure_rec6(hs_handle* h) {
  if (h->rec6_state) return h->rec6_state > 0;
#ifdef HS_TEST_HOOKS
  if (h->knobs.test_rec6_no_room) {
    h->rec6_state = -1;
    return false;
  }
#endif
  const size_t n = h->n;
  const int L = (int)h->p.L;
  if (h->t_rec6.reserve(((size_t)L * n + HS_JM_WAVE) * 16) != hipSuccess) {
    (void)hipGetLastError();
    h->rec6_state = -1;
    return false;
  }
  // (the pad behind the last entry is read by nobody: the kernel clamps a member index to its segment)
  for (int l = 0; l < L; ++l)
    if (hs_launch_gather_rec6(h->packed_all.as<uint4>(), h->tabs.t[l].ids, (uint32_t)n, (int)h->p.k, h->jtab6.p,
                              h->t_rec6.as<uint4>() + (size_t)l * n, h->stream) != hipSuccess) {
      (void)hipGetLastError();
      h->rec6_state = -1;
      return false;
    }
  h->rec6_state = 1;
  return true;
}

// May a self-join at radius R run from the residue codes alone (the plan's self_codes)?  Only when
// nothing on its way can need the embedded centres: the int8 join and its thin-segment filter must
// apply, and no query row may be unrepresentable -- for a k-mer of the coordinate table the one way
// is -gamma overflowing its 13 base-127 digits, bounded here from R and the scale alone.
static bool self_codes_ok(const hs_handle* h, double R) {
  const bool wide = want_wide(h, R);
  const double r2 = R * R, s = wide ? h->join8_scale_w : h->join8_scale, k = (double)h->p.k;
  if (!h->join8_tables_ok || h->p.k > 50 || h->verify_mode == 1 || h->verify_mode == 3 || !(r2 < 30000.0))
    return false;
  // (segments routed away from the join go to the streaming filter, which works from the centres)
  if (h->join_min_q > 1 || h->join_min_m > 1 || h->knobs.no_self_codes) return false;
  // -gamma <= s^2 R^2 / 2 + L1(c^)/2 + 3, L1(c^) <= 127 * 4 k (127 * 8 k with wide rows)
  return s > 0.0 && 0.5 * s * s * r2 + (wide ? 508.0 : 254.0) * k + 3.0 < 127.0 * 127.0 * 13.0;
}

// How a batch runs, decided by plan_batch before its first launch from the handle's switches, the call
// and the batch history.  demote() alone changes it afterwards, when a query row is unsafe.
struct BatchPlan {
  bool can16 = false;       // the fp16 form of the join filter exists (k <= 25): int8's fallback
  bool use_join = false;    // bucket join (fp16 or int8 rows) in front of the exact decision; streaming otherwise
  bool use_i8 = false;      // ... in its int8 form (hs_join8.hip)
  int wide = 0;             // ... over all 8 coordinate columns (want_wide)
  bool refine = false;      // the int8 join's survivors pass an 8-column bound: hs_refine_codes_kernel when the
                            // queries are k-mers (b.qcodes), hs_refine8_kernel (int8 rows) otherwise
  bool self_codes = false;  // self-join whose per-query quantities all come from the indexed codes
  bool ext_codes = false;   // queries given as codes that never become centres
  bool seg_sparse = false;  // probes grouped by a sort of the probes, not a counting sort over the buckets
  bool parted = false;      // bucket partition: only this part's probes are fingerprinted and grouped
  bool all_joined = false;  // every segment goes to the join (HS_OPT_JOIN_MIN_Q / _M at 1)
  bool no_slices = false;   // ... so the probes write no slice counts and the slice offsets stay the reset's zeros
  bool use_r = false;       // segments with few probing queries through hs_join8r_kernel
  bool f6 = false;          // the other segments through hs_join6x_kernel (FP6 rows) instead of hs_join8x_kernel
  uint32_t jm = HS_JM_BLOCK;  // members per join work item
  uint32_t jm_stream = 0;     // ... of the segments outside the resident kernel's class, where it differs (f6 on
                              // hs_join6w_kernel: 192); 0: jm
  bool async_items = false;   // the item count stays on the device; the descriptors are sized by item_cap
  uint32_t item_cap = 0;
  bool order_here = false;    // the batch orders its hits per query itself (no sort afterwards)
  int xcd_run = -1;           // chunks per XCD-local run of join items (-1: by the query tiles' size)
  bool resident_stale = false;  // the history's resident share was measured on a batch of another size
};

// Precedence, first rule first: the filter form (verify mode, k, radius, the tables' representability), then
// what follows from it (wide rows, refinement, queries from codes, item size, the resident kernel), then the
// grouping -- a bucket partition always sorts its probes (the counting sort needs the rank of every probe,
// which the part's owned-probe list never writes), HS_OPT_SEG_MODE next, the bucket : probe ratio last.
static BatchPlan plan_batch(const hs_handle* h, const QueryCall& c, uint32_t nq, bool allow_async, bool ordered_out) {
  BatchPlan p;
  const BatchHistory& m = h->hist;
  const int k = (int)h->p.k;
  const double r2 = c.R * c.R;
  // fp16 form: k <= 25 only; int8 form (hs_join8.hip): k <= 50 (6 or 8 k-steps for two packed words)
  p.can16 = h->join_tables_ok && k <= 25;
  const bool can8 = h->join8_tables_ok && k <= 50 && h->verify_mode != 3;
  p.use_join = h->verify_mode != 1 && r2 < 30000.0 && (p.can16 || can8);
  p.use_i8 = p.use_join && can8;
  p.wide = (p.use_i8 && want_wide(h, c.R)) ? 1 : 0;
  // (wide rows already hold all 8 columns: nothing to refine)
  p.refine = p.use_i8 && !p.wide && !h->knobs.no_refine8;
  // Self-join (the queries are the indexed k-mers self_first + q_base ..): every per-query quantity
  // comes from the residue codes and the tables -- no embedded centres, no hashing, no directory
  // search (a k-mer probes the bucket it sits in).  Needs the int8 join with its thin-segment filter,
  // the only filters that work without per-query distance tables.  Queries given as codes likewise.
  const bool codes_ok = p.use_i8 && self_codes_ok(h, c.R);
  p.self_codes = codes_ok && c.self_first != HS_NO_SELF;
  p.ext_codes = codes_ok && c.codes;
  // how the probes are grouped by bucket in front of the join: a counting sort over the bucket slots,
  // or -- when those far outnumber the probes -- a sort of the probes
  // (measured at the configs[2] shape, 10^6 queries x 32 tables against 1.3e8 bucket slots -- a ratio of 4:
  // 11.3 ms for the whole probe + segment chain with the sort, 15.0 with the counting sort)
  p.parted = p.use_join && h->bucket_parts > 1 && c.self_first == HS_NO_SELF;  // (searches only)
  p.seg_sparse = p.parted || (h->knobs.seg_mode ? h->knobs.seg_mode == 1 : (uint64_t)h->nb_total > 2ull * nq * h->p.L);
  p.all_joined = h->join_min_q == 1 && h->join_min_m == 1;
  // (a bucket partition's list of owned probes is made by a kernel that writes the slice counts of all of them)
  p.no_slices = p.use_join && p.all_joined && !p.parted;
  // work items: one wave's 128 members for the wave-independent int8 join, 512 otherwise
  p.jm = p.use_i8 ? hs_join8_members_per_item(k, p.wide) : HS_JM_BLOCK;
  // k <= 25 with 4-column rows: segments probed by at most HS_JR_MAXQ queries of the batch go to the
  // query-resident kernel (hs_join8r_kernel), as the tail of the item list
  p.resident_stale = p.use_join && m.resident_nq && (nq > 2 * m.resident_nq || 2 * nq < m.resident_nq);
  const double share = p.resident_stale ? -1.0 : m.resident_share;
  p.use_r = p.use_i8 && !p.wide && k <= 25 && h->alphabet <= HS_JR_MAX_ALPHABET && !h->knobs.no_join_r &&
            (h->knobs.force_join_r || share < 0.0 || share >= 0.5 || m.resident_age >= 64);
  // Queries that are k-mers, k = 21..25, 4-column rows: the FP6 form of the query-streaming kernel (its bound is a
  // table over residue PAIRS, so centres that are no k-mers have none).  query_batch builds the member records.
  p.f6 = (p.self_codes || p.ext_codes) && !p.wide && k >= 21 && k <= 25 && h->alphabet <= 32 && h->PW == 1 &&
         h->join6_tables_ok && !h->knobs.no_join_f6 && h->rec6_state >= 0;
  // ... on items of 192 members (hs_join6w_kernel) unless HS_OPT_JOIN_F6_FORM says 0
  p.jm_stream = (p.f6 && h->knobs.join_f6_form != 0) ? hs_join6_wide_item() : 0u;
  // No host round trip when the int8 join takes every segment and the previous batch left a
  // capacity hint: the item count stays on the device (item_off[nqs]); join legality and the
  // capacity are checked with the batch's final read-back, a violation repeats the batch the
  // slow way.  Otherwise one round trip: join legality, item count, streaming slices.
  p.async_items = allow_async && p.use_i8 && p.all_joined && m.item_cap_hint && !h->knobs.sync_items;
  p.item_cap = p.async_items ? m.item_cap_hint : 0;
  // the batch orders its hits itself (bucket by query, no sort, no host count); not tried again at a
  // radius at which the previous batch had a query with too many hits for it (the attempt costs 10 % of
  // such a batch -- k = 15 at the C2 sizes, 545 hits per query)
  p.order_here = ordered_out && !h->knobs.sort_hits && !(m.order_failed && !c.radii && m.order_failed_R == c.R);
  p.xcd_run = h->knobs.join_xcd_run;
  return p;
}

// One batch's queries and the device arrays and counts the stages hand on to each other.
struct Batch {
  uint32_t nq = 0, q_base = 0, nql = 0;
  uint32_t nqs = 0;                  // probes the grouping works on (bucket partition: the ones that found a bucket)
  double r2 = 0.0;                   // R * R (motif_both_points.cpp:204)
  const double* centers = nullptr;   // the call's centres, or the embedded query codes
  uint64_t* d_cand = nullptr;
  const uint8_t* qcodes = nullptr;   // from-codes batches: the codes every per-query quantity comes from
  const uint32_t* owned = nullptr;   // bucket partition: the probes of this part, ascending (device)
  uint32_t n_owned = 0;
  uint32_t n_items = 0, n_slices = 1;
  const double* radii = nullptr;     // the batch's slice of the call's per-query radii (device), or null: r2 for all
};

// Bytes reserved per query row, in c16 and (in segment order) c16s: the widest fp16 row (208 halves), or the 128
// bytes of a k <= 25 int8 row with the FP6 row behind it
static size_t qrow_room() { return std::max<size_t>(208 * 2, 128 + (size_t)hs_join6_row_bytes()); }

// The join filter's query rows, on stream s: from the codes, int8 from the centres, or fp16
static hipError_t launch_qrows(hs_handle* h, const BatchPlan& p, const Batch& b, hipStream_t s) {
  const int k = (int)h->p.k;
  uint32_t* const d_unsafe = h->counters.as<uint32_t>() + 8;
  if (p.f6) {  // FP6 rows behind the int8 rows' place; the int8 rows only where the resident kernel reads them
    hipError_t e = hs_launch_qprep6_codes(b.qcodes, b.nq, k, b.r2, h->jtab6.p, h->c16.as<char>() + (size_t)b.nq * 128,
                                          s, b.radii);
    if (e != hipSuccess || !p.use_r) return e;
  }
  if (p.self_codes || p.ext_codes)  // (no second row: these batches' survivors are refined from the codes)
    return hs_launch_qprep8_codes(b.qcodes, b.nq, k, p.wide, b.r2, h->coords.as<double>(), h->jtab8.p,
                                  h->jtab8.as<char>() + 1024, h->jtab8.as<char>() + 1536, h->jtab8.as<float>() + 128,
                                  h->c16.p, nullptr, s, b.radii);
  if (p.use_i8)
    return hs_launch_qprep8(b.centers, b.nq, k, p.wide, b.r2, h->jtab8.as<float>() + 128, h->c16.p, d_unsafe,
                            p.refine ? h->c8b.p : nullptr, s, b.radii);
  return hs_launch_qprep(b.centers, b.nq, k, b.r2, h->c16.p, d_unsafe, s, b.radii);
}

// Where the FP6 rows of a batch sit in segment order: behind the room of its int8 rows in c16s.  (The join reads
// a whole 32-row tile at a segment's ragged end too: at most 31 rows past the last, inside the 64 spare rows.)
static char* c6t_of(hs_handle* h, const Batch& b) { return h->c16s.as<char>() + ((size_t)b.nql + 64) * 128; }

// The query rows gathered into segment order (c16s)
static hipError_t gather_qrows(hs_handle* h, const BatchPlan& p, const Batch& b) {
  if (p.f6) {
    hipError_t e = hs_launch_gather_c6t(h->c16.as<char>() + (size_t)b.nq * 128, h->sorted_ql.as<uint32_t>(),
                                        h->seg_qoff.as<uint32_t>(), h->seg_of.as<uint32_t>(), b.nqs, (int)h->p.L,
                                        c6t_of(h, b), h->stream);
    if (e != hipSuccess || !p.use_r) return e;
  }
  if (p.use_i8)
    return hs_launch_gather_c8t(h->c16.p, h->sorted_ql.as<uint32_t>(), h->seg_qoff.as<uint32_t>(),
                                h->seg_of.as<uint32_t>(), b.nqs, (int)h->p.L, (int)h->p.k, p.wide, h->c16s.p, h->stream);
  return hs_launch_gather_c16(h->c16.p, h->sorted_ql.as<uint32_t>(), b.nqs, (int)h->p.L, h->c16s.p, h->stream);
}

// The probe of the batch's (query, table) pairs (bucket partition: the part's listed ones).  With a join
// ahead it also numbers each probe's bucket, and ranks it inside for the counting sort (hs_launch_seg_group).
static hipError_t launch_probe(hs_handle* h, const QueryCall& c, const BatchPlan& p, const Batch& b) {
  uint32_t* const qbucket = p.use_join ? h->seg_keys.as<uint32_t>() : nullptr;
  uint32_t* const bucket_count = p.use_join && !p.seg_sparse ? h->bucket_work.as<uint32_t>() : nullptr;
  uint32_t* const qrank = bucket_count ? qbucket + ((size_t)b.nql + 1) : nullptr;
  unsigned long long* const d_cand_total = reinterpret_cast<unsigned long long*>(h->counters.as<uint32_t>() + 2);
  uint32_t* const nslices = (p.use_join && p.no_slices) ? nullptr : h->nslices.as<uint32_t>();
  if (p.self_codes)
    return hs_launch_self_probe(h->tabs, c.self_first + b.q_base, b.nq, (int)h->p.L, h->qstart.as<uint32_t>(),
                                h->qcount.as<uint32_t>(), nslices, b.d_cand, d_cand_total,
                                h->dir_base.as<uint32_t>(), h->nb_total, bucket_count, qbucket, qrank, h->stream);
  return hs_launch_probe(probe_tabs(h, c, b.q_base, b.owned, b.n_owned), h->qints.as<int32_t>(), b.nq, (int)h->p.K,
                         (int)h->p.L, h->key_seed, h->qstart.as<uint32_t>(), h->qcount.as<uint32_t>(),
                         nslices, b.d_cand, d_cand_total, h->probe_slow.as<uint32_t>(),
                         h->dir_base.as<uint32_t>(), h->nb_total, bucket_count, qbucket, qrank, h->stream);
}

// Work items of the plan's size from the segments, the resident kernel's class as their tail
static hs_status cut_plan_items(hs_handle* h, const BatchPlan& p, const Batch& b) {
  unsigned long long* const d_jstats = reinterpret_cast<unsigned long long*>(h->counters.as<uint32_t>() + 10);
  return cut_items(h, b.nqs, p.jm, d_jstats, p.use_r ? HS_JR_MAXQ : 0u, b.nql, !p.no_slices, p.jm_stream);
}

// Where every probe's slices start in the streaming filter's grid (every segment joined -- the default --:
// all slice counts are zero, and so is their scan: the batch's reset left it so when no probe wrote a count)
static hipError_t slice_offsets(hs_handle* h, const BatchPlan& p, const Batch& b) {
  if (p.use_join && p.no_slices) return hipSuccess;
  if (p.use_join && p.all_joined) return hipMemsetAsync(h->slice_off.p, 0, ((size_t)b.nql + 1) * 4, h->stream);
  return hs_exclusive_scan_u32(h->temp.p, h->temp.cap, h->nslices.as<uint32_t>(), h->slice_off.as<uint32_t>(),
                               (size_t)b.nql + 1, h->stream);
}

// Stage 1: the queries.  Given as codes (hs_query_codes): a checked copy first (a code outside the alphabet
// is reported with the batch's counters and replaced by 0, so no kernel indexes a table with it).  When
// every filter on the way works from codes (self_codes_ok) no embedded centre exists at any point: 25 bytes
// per query instead of 1600 -- hash, query rows and the exact decision all read the table rows the DB's
// k-mers read.  Otherwise the codes are embedded here, on the device, and the batch runs as for any other
// centres.  The join filter's query rows depend on the queries only: quantised on the side stream while
// the main stream hashes and probes (both passes stream the same 8d bytes per query).
static hs_status prepare_queries(hs_handle* h, const QueryCall& c, const BatchPlan& p, Batch& b) {
  const int k = (int)h->p.k;
  if (p.wide) HS_CHECK(ensure_rec8w(h));
  if (p.self_codes) b.qcodes = h->codes.as<uint8_t>() + ((uint64_t)c.self_first + b.q_base) * k;
  if (c.codes) {
    HS_HIP(h, h->qcodes_buf.reserve(std::max<size_t>(16, (size_t)b.nq * k)));
    HS_HIP(h, hs_launch_check_codes(c.codes, (uint64_t)b.nq * k, h->alphabet, h->qcodes_buf.as<uint8_t>(),
                                    h->counters.as<uint32_t>() + HS_CNT_BAD_QUERY_CODE, h->stream));
    if (p.ext_codes) {
      b.qcodes = h->qcodes_buf.as<uint8_t>();
    } else {
      HS_HIP(h, h->qembed.reserve(std::max<size_t>(16, (size_t)b.nq * h->d * 8)));
      HS_HIP(h, hs_launch_embed(h->qcodes_buf.as<uint8_t>(), b.nq, k, h->coords.as<double>(),
                                h->qembed.as<double>(), h->stream));
      b.centers = h->qembed.as<double>();
    }
  }
  if (p.use_join) {
    HS_HIP(h, h->c16.reserve((size_t)b.nq * qrow_room()));
    if (p.refine && !b.qcodes) HS_HIP(h, h->c8b.reserve((size_t)b.nq * hs_join8_row_bytes(k, p.wide)));
    HS_HIP(h, hipEventRecord(h->evx[EV_FORK], h->stream));
    HS_HIP(h, hipStreamWaitEvent(h->stream2, h->evx[EV_FORK], 0));
    HS_HIP(h, launch_qrows(h, p, b, h->stream2));
    HS_HIP(h, hipEventRecord(h->evx[EV_JOIN], h->stream2));
  }
  return HS_OK;
}

// Stage 2: hash and probe.  Bucket partition: the part's own probes (by their bucket ints alone) are listed
// first, and only those -- 1 / n_parts of the batch -- pay for a fingerprint and a walk of the directory.
static hs_status hash_and_probe(hs_handle* h, const QueryCall& c, const BatchPlan& p, Batch& b) {
  const size_t n1 = (size_t)b.nql + 1;
  HS_HIP(h, h->qints.reserve((size_t)b.nq * h->LK * 4));
  HS_HIP(h, h->qstart.reserve(((size_t)b.nql + HS_QRANGE_PAD) * 4));
  HS_HIP(h, h->qcount.reserve(((size_t)b.nql + HS_QRANGE_PAD) * 4));
  for (DevBuf* d : {&h->nslices, &h->probe_slow, &h->slice_off}) HS_HIP(h, d->reserve(n1 * 4));
  HS_HIP(h, h->temp.reserve(hs_scan_u32_temp(n1) + 256));
  if (c.pre_ints)
    HS_HIP(h, hipMemcpyAsync(h->qints.p, c.pre_ints, (size_t)b.nq * h->LK * 4, hipMemcpyDeviceToDevice, h->stream));
  else if (p.ext_codes)
    HS_CHECK(hash_dispatch(h, b.qcodes, nullptr, b.nq, -1, h->qints.as<int32_t>(), h->LK, HS_PROJ_SET_BATCH, h->stream));
  else if (!p.self_codes)
    HS_CHECK(hash_dispatch(h, nullptr, b.centers, b.nq, -1, h->qints.as<int32_t>(), h->LK, HS_PROJ_SET_BATCH, h->stream));
  HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  if (p.use_join) {
    HS_HIP(h, h->seg_keys.reserve(n1 * 8));
    // (the sort of the probes needs no ranks and no pass over the bucket slots: hs_launch_seg_group_sparse)
    HS_HIP(h, h->bucket_work.reserve(4 * (p.seg_sparse ? n1 : (size_t)h->nb_total + 2) * 4));
  }
  if (p.parted) {
    HS_HIP(h, h->part_work.reserve(5 * n1 * 4));
    uint32_t* const pw = h->part_work.as<uint32_t>();
    HS_HIP(h, hs_launch_part_owned(probe_tabs(h, c, b.q_base), h->qints.as<int32_t>(), b.nq, (int)h->p.K,
                                   (int)h->p.L, h->nb_total, pw, h->qstart.as<uint32_t>(), h->qcount.as<uint32_t>(),
                                   h->nslices.as<uint32_t>(), b.d_cand, h->seg_keys.as<uint32_t>(), h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, pw, pw + n1, n1, h->stream));
    HS_HIP(h, hs_launch_flagged_list(pw, pw + n1, b.nql, pw + 4 * n1, h->stream));
    HS_HIP(h, hipMemcpyAsync(&b.n_owned, pw + n1 + b.nql, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    b.owned = pw + 4 * n1;
  }
  HS_HIP(h, launch_probe(h, c, p, b));
  return HS_OK;
}

// Stage 3: the probes grouped by bucket into segments, the segments cut into work items, the query rows
// gathered in segment order.  Bucket partition: only the part's probes that found a bucket are grouped.
static hs_status group_segments(hs_handle* h, const BatchPlan& p, Batch& b) {
  if (!p.use_join) return HS_OK;
  const size_t n1 = (size_t)b.nql + 1;
  HS_HIP(h, h->c16s.reserve(((size_t)b.nql + 64) * qrow_room()));
  for (DevBuf* d : {&h->seg_keys, &h->seg_keys_sorted, &h->seg_key}) HS_HIP(h, d->reserve(n1 * 8));
  for (DevBuf* d : {&h->seg_vals, &h->sorted_ql, &h->seg_cnt, &h->seg_qoff, &h->seg_items, &h->item_off, &h->seg_of})
    HS_HIP(h, d->reserve(n1 * 4));
  HS_HIP(h, h->seg_n.reserve(64));
  HS_HIP(h, h->temp.reserve(std::max(hs_scan_u32_temp(n1), hs_scan_u32_temp((size_t)h->nb_total + 2)) + 256));
  // (the query rows of the join filter were quantised on the side stream, beside hash and probe)
  HS_HIP(h, hipStreamWaitEvent(h->stream, h->evx[EV_JOIN], 0));
  const int L = (int)h->p.L, seg_shift = seg_shift_of(h);
  if (p.seg_sparse) {
    HS_HIP(h, h->temp.reserve(std::max(hs_sort_pairs_u32_u32_temp(b.nql), hs_scan_u32_temp(n1)) + 256));
    const uint32_t* keys_in = h->seg_keys.as<uint32_t>();
    const uint32_t* probes_in = nullptr;
    if (p.parted) {
      uint32_t* const pw = h->part_work.as<uint32_t>();
      uint32_t n_found = 0;
      if (b.n_owned) {
        HS_HIP(h, hs_launch_found_probes(h->seg_keys.as<uint32_t>(), b.n_owned, h->nb_total, h->temp.p, h->temp.cap,
                                         pw, pw + n1, pw + 2 * n1, pw + 3 * n1, h->stream, b.owned));
        HS_HIP(h, hipMemcpyAsync(&n_found, pw + n1 + b.n_owned, 4, hipMemcpyDeviceToHost, h->stream));
      }
      HS_HIP(h, hipStreamSynchronize(h->stream));
      if (n_found) {  // (none at all: the batch goes on as one of probes that found nothing)
        b.nqs = n_found;
        keys_in = pw + 2 * n1;
        probes_in = pw + 3 * n1;
      }
    }
    HS_HIP(h, hs_launch_seg_group_sparse(h->tabs, h->dir_base.as<uint32_t>(), L, seg_shift, h->nb_total, h->temp.p,
                                         h->temp.cap, keys_in, h->seg_keys.as<uint32_t>() + n1,
                                         h->seg_vals.as<uint32_t>(), h->bucket_work.as<uint32_t>(), b.nqs,
                                         h->sorted_ql.as<uint32_t>(), h->seg_key.as<uint64_t>(),
                                         h->seg_cnt.as<uint32_t>(), h->seg_n.as<uint32_t>(), h->seg_of.as<uint32_t>(),
                                         h->stream, probes_in));
  } else {
    HS_HIP(h, hs_launch_seg_group(h->tabs, h->dir_base.as<uint32_t>(), L, seg_shift, h->nb_total,
                                  h->bucket_work.as<uint32_t>(),
                                  h->bucket_work.as<uint32_t>() + (((size_t)h->nb_total + 3) & ~(size_t)1),
                                  h->temp.p, h->temp.cap, h->seg_keys.as<uint32_t>(), h->seg_keys.as<uint32_t>() + n1,
                                  b.nql, h->sorted_ql.as<uint32_t>(), h->seg_key.as<uint64_t>(),
                                  h->seg_cnt.as<uint32_t>(), h->seg_n.as<uint32_t>(), h->seg_of.as<uint32_t>(),
                                  h->stream));
  }
  HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, h->seg_cnt.as<uint32_t>(), h->seg_qoff.as<uint32_t>(),
                                  (size_t)b.nqs + 1, h->stream));
  HS_CHECK(cut_plan_items(h, p, b));
  HS_HIP(h, gather_qrows(h, p, b));
  return HS_OK;
}

// A query row the plan's form cannot carry (found by the item read-back): the batch goes on one form down --
// int8 -> fp16 (the query rows again; the items again if their size changes), fp16 -> the streaming filter
// (the probes again, without the join's outputs, and their slices) -- re-issuing only what the new form needs.
static hs_status demote(hs_handle* h, const QueryCall& c, BatchPlan& p, Batch& b, uint32_t unsafe) {
  if (p.self_codes || p.ext_codes) return fail(h, HS_ERR_STATE, "queries from codes: a query row marked unsafe");
  uint32_t* const d_cnt = h->counters.as<uint32_t>();
  if (p.use_i8) {
    p.use_i8 = p.refine = false;
    if (p.can16) {
      HS_HIP(h, hipMemsetAsync(d_cnt + 8, 0, 4, h->stream));
      HS_HIP(h, launch_qrows(h, p, b, h->stream));
      HS_HIP(h, gather_qrows(h, p, b));
      HS_HIP(h, hipMemcpyAsync(&unsafe, d_cnt + 8, 4, hipMemcpyDeviceToHost, h->stream));
      if (p.jm != HS_JM_BLOCK) {  // the fp16 kernel works on 512-member items: cut the segments again
        p.jm = HS_JM_BLOCK;
        p.jm_stream = 0;
        p.use_r = false;
        HS_HIP(h, hipMemsetAsync(d_cnt + 10, 0, 16, h->stream));
        HS_CHECK(cut_plan_items(h, p, b));
        HS_HIP(h, hipMemcpyAsync(&b.n_items, h->item_off.as<uint32_t>() + b.nqs, 4, hipMemcpyDeviceToHost,
                                 h->stream));
      }
      HS_HIP(h, hipStreamSynchronize(h->stream));
    }
  }
  if (unsafe) {
    p.use_join = false;
    b.n_items = 0;
    b.owned = nullptr;  // (every probe again)
    b.n_owned = 0;
    HS_HIP(h, hipMemsetAsync(d_cnt + 2, 0, 8, h->stream));
    HS_HIP(h, hipMemsetAsync(h->probe_slow.p, 0, 4, h->stream));  // (the list of the probes left to the slow kernel)
    HS_HIP(h, launch_probe(h, c, p, b));
    HS_HIP(h, slice_offsets(h, p, b));
    b.n_slices = 1;
  }
  return HS_OK;
}

// Stage 4: the item count, join legality and the streaming slices, in one round trip -- or none when the
// plan leaves the item count on the device -- then the work item descriptors.
static hs_status read_items(hs_handle* h, const QueryCall& c, BatchPlan& p, Batch& b) {
  HS_HIP(h, slice_offsets(h, p, b));
  uint32_t unsafe = 0;
  if (p.async_items) {
    b.n_items = p.item_cap;
    b.n_slices = 0;
  } else {
    if (p.use_join) {
      HS_HIP(h, hipMemcpyAsync(&unsafe, h->counters.as<uint32_t>() + 8, 4, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipMemcpyAsync(&b.n_items, h->item_off.as<uint32_t>() + b.nqs, 4, hipMemcpyDeviceToHost, h->stream));
    }
    HS_HIP(h, hipMemcpyAsync(&b.n_slices, h->slice_off.as<uint32_t>() + b.nql, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  if (unsafe) HS_CHECK(demote(h, c, p, b, unsafe));
  if (b.n_items) {
    HS_HIP(h, h->item_desc.reserve((size_t)b.n_items * 32));
    HS_HIP(h, hs_launch_item_desc(h->tabs, h->seg_key.as<uint64_t>(), h->seg_cnt.as<uint32_t>(),
                                  h->seg_qoff.as<uint32_t>(), h->item_off.as<uint32_t>(), b.nqs,
                                  h->sorted_ql.as<uint32_t>(), h->qcount.as<uint32_t>(), b.n_items, p.jm,
                                  seg_shift_of(h), h->seg_vals.as<uint32_t>(), h->PW,
                                  p.async_items ? h->item_off.as<uint32_t>() + b.nqs : nullptr,
                                  h->seg_res.as<uint64_t>(), h->seg_n.as<uint32_t>() + 2,
                                  h->counters.as<uint32_t>() + HS_CNT_SPLIT, h->item_desc.as<uint4>(), h->stream,
                                  p.jm_stream));
  }
  // segments routed away from the join (HS_OPT_JOIN_MIN_Q / _M; none by default) go through the streaming
  // filter and its per-query distance tables, on the side stream beside the join
  if (b.n_slices) {
    HS_HIP(h, h->tq.reserve((size_t)b.nq * h->p.k * HS_TROW * 4));
    if (!b.n_items)
      HS_HIP(h, hs_launch_qtables(b.centers, b.nq, (int)h->p.k, h->coords.as<double>(), h->alphabet,
                                  h->tq.as<float>(), h->stream));
  }
  return HS_OK;
}

// Stage 5: the filters, into one survivor list of prov_cap entries: the join (int8: the query-streaming kernel
// over the head of the item list, the query-resident one over its tail; fp16), and the streaming filter for
// the probes' slices -- beside the join on the side stream when both have work.
static hs_status launch_filters(hs_handle* h, const BatchPlan& p, const Batch& b, uint32_t prov_cap, bool again) {
  const int k = (int)h->p.k, L = (int)h->p.L;
  const float r2_hi = filter_bound(b.r2);
  uint32_t* const d_cnt = h->counters.as<uint32_t>();
  const int n_blocks = h->n_cu * 8, join_blocks = h->n_cu * h->join_blocks_per_cu;
  const bool side = b.n_items && b.n_slices;
  auto verify = [&](hipStream_t s) {
    return hs_launch_verify(h->tabs, h->qstart.as<uint32_t>(), h->qcount.as<uint32_t>(), h->slice_off.as<uint32_t>(),
                            b.nql, h->tq.as<float>(), k, L, r2_hi, d_cnt, prov_cap, h->prov.as<uint2>(), n_blocks, s,
                            b.radii);
  };
  if (side) {
    HS_HIP(h, hipEventRecord(h->evx[EV_FORK], h->stream));
    HS_HIP(h, hipStreamWaitEvent(h->stream2, h->evx[EV_FORK], 0));
    if (!again)  // (the streaming filter's query tables: beside the join too, once)
      HS_HIP(h, hs_launch_qtables(b.centers, b.nq, k, h->coords.as<double>(), h->alphabet, h->tq.as<float>(),
                                  h->stream2));
    HS_HIP(h, verify(h->stream2));
    HS_HIP(h, hipEventRecord(h->evx[EV_JOIN], h->stream2));
  }
  HS_HIP(h, hipEventRecord(h->ev[11], h->stream));  // the join kernel alone: ev[11] .. ev[10]
  if (b.n_items && p.use_i8) {
    // (split == the item count when no segment qualifies for the resident kernel or use_r is off)
    const uint32_t* const d_split = h->seg_n.as<uint32_t>() + 2;
    const uint4* const rec8 = (p.wide && !h->wide8) ? h->t_rec8w.as<uint4>() : h->t_rec8.as<uint4>();
    const void* const rows = p.wide ? (const void*)(h->jtab8.as<char>() + 1536) : (const void*)h->jtab8.p;
    // XCD-local runs of items where the batch's query tiles do not stay in every XCD's L2 anyway
    // (d_cnt + 40 .. 47: the per-XCD chunk counters)
    const uint64_t tile_bytes = (uint64_t)b.nqs * (uint64_t)hs_join8_row_bytes(k, p.wide);
    const uint32_t xcd_run = p.xcd_run >= 0 ? (uint32_t)p.xcd_run : (tile_bytes > (64ull << 20) ? 128u : 0u);
    const uint32_t* const d_n_items =
        p.use_r ? d_split : (p.async_items ? h->item_off.as<uint32_t>() + b.nqs : nullptr);
    if (p.f6) {
      uint32_t G = hs_join8_chunk_items(b.n_items, join_blocks, h->hist.pairs_per_item, h->knobs.join_chunk);
      // items of 192 members take 1.5 times as long, and what is lost at the kernel's end is paid in chunks: half
      // the items per chunk (bench.py's default workload: 8 -> 4 took 2 % off the kernel; 2 added 20 %)
      if (p.jm_stream && !h->knobs.join_chunk) G = std::max(2u, (G + 1u) / 2u);
      HS_HIP(h, hs_launch_join6x(h->item_desc.as<uint4>(), b.n_items, h->tabs.t[0].packed, h->t_rec6.as<uint4>(),
                                 c6t_of(h, b), h->jtab6.p, d_cnt, prov_cap, h->prov.as<uint2>(), d_cnt + 32,
                                 join_blocks, d_n_items, G, xcd_run, h->stream, p.jm_stream ? 1 : 0));
    } else
      HS_HIP(h, hs_launch_join8w(h->item_desc.as<uint4>(), b.n_items, h->tabs.t[0].packed, rec8, h->c16s.p, rows, k,
                                 p.wide, d_cnt, prov_cap, h->prov.as<uint2>(), d_cnt + 32, join_blocks, d_n_items,
                                 h->hist.pairs_per_item, xcd_run, h->stream, h->knobs.join_chunk));
    if (p.use_r)
      HS_HIP(h, hs_launch_join8r(h->item_desc.as<uint4>(), b.n_items, d_split, h->tabs.t[0].packed,
                                 h->t_rho.as<uint32_t>(), h->c16s.p, rows, h->alphabet, d_cnt, prov_cap,
                                 h->prov.as<uint2>(), d_cnt + 33, join_blocks, h->hist.pairs_per_item, h->stream));
  } else if (b.n_items) {
    HS_HIP(h, hs_launch_join(h->item_desc.as<uint4>(), b.n_items, h->tabs.t[0].packed, h->sorted_ql.as<uint32_t>(),
                             h->c16s.p, h->jtab.p, reinterpret_cast<const float*>(h->jtab.as<char>() + 512), k, d_cnt,
                             prov_cap, h->prov.as<uint2>(), join_blocks, h->stream));
  }
  HS_HIP(h, hipEventRecord(h->ev[10], h->stream));
  if (side)
    HS_HIP(h, hipStreamWaitEvent(h->stream, h->evx[EV_JOIN], 0));
  else if (b.n_slices)
    HS_HIP(h, verify(h->stream));
  return HS_OK;
}

// Stage 6: the exact decision on the survivors (after the int8 join's 8-column refinement), and the hits
// ordered per query into the caller's arrays when the plan says so.
static hs_status finalize_hits(hs_handle* h, const QueryCall& c, const BatchPlan& p, const Batch& b,
                               uint32_t prov_cap, uint32_t hit_cap, bool again, BatchOut* bout) {
  const int k = (int)h->p.k, L = (int)h->p.L;
  uint32_t* const d_cnt = h->counters.as<uint32_t>();
  const uint2* fin_list = h->prov.as<uint2>();
  const uint32_t* fin_count = d_cnt;
  const uint4* d_qpacked = nullptr;
  if (b.qcodes && k <= 75) {  // the queries are k-mers: packed like the members, for the refinement and the exact pass
    HS_HIP(h, h->qpacked.reserve(std::max<size_t>(16, (size_t)b.nq * h->PW * 16)));
    HS_HIP(h, hs_launch_pack(b.qcodes, b.nq, k, h->alphabet, h->qpacked.as<uint4>(), d_cnt + HS_CNT_BAD_QUERY_CODE,
                             h->stream));
    d_qpacked = h->qpacked.as<uint4>();
  }
  if (p.refine && b.n_items) {
    HS_HIP(h, h->prov2.reserve((size_t)prov_cap * 8));
    if (again) HS_HIP(h, hipMemsetAsync(d_cnt + 4, 0, 4, h->stream));  // (first pass: the batch's reset)
    if (b.qcodes)  // (p.refine: the int8 join, k <= 50.  No second query row on this path: launch_qrows)
      HS_HIP(h, hs_launch_refine_codes(h->tabs, h->prov.as<uint2>(), d_cnt, prov_cap, h->sorted_ql.as<uint32_t>(),
                                       d_qpacked, h->coords.as<double>(), h->alphabet, k, L, b.r2, b.radii,
                                       h->qstart.as<uint32_t>(), h->qcount.as<uint32_t>(), h->prov2.as<uint2>(),
                                       d_cnt + 4, h->stream));
    else
      HS_HIP(h, hs_launch_refine8(h->tabs, h->prov.as<uint2>(), d_cnt, prov_cap, h->sorted_ql.as<uint32_t>(), h->c16.p,
                                  h->c8b.p, h->jtab8.as<char>() + 1024, h->jtab8.as<float>() + 128, k, L,
                                  h->qstart.as<uint32_t>(), h->qcount.as<uint32_t>(), h->prov2.as<uint2>(), d_cnt + 4,
                                  h->stream));
    fin_list = h->prov2.as<uint2>();
    fin_count = d_cnt + 4;
  }
  uint32_t* const qcnt = p.order_here ? h->qhits.as<uint32_t>() : nullptr;
  HS_HIP(h, hs_launch_finalize(h->tabs, h->codes.as<uint8_t>(), b.centers, b.qcodes, h->coords.as<double>(),
                               h->qstart.as<uint32_t>(), h->qcount.as<uint32_t>(), fin_list, fin_count, prov_cap,
                               h->sorted_ql.as<uint32_t>(), k, L, b.r2, c.sqrt_test ? c.R : (double)NAN, b.q_base,
                               c.self_first, d_cnt + 1, hit_cap, h->hit_key.as<uint64_t>(), h->hit_val.as<uint64_t>(),
                               qcnt, h->alphabet, d_qpacked, p.order_here ? h->hit_rank.as<uint32_t>() : nullptr,
                               h->stream, b.radii));
  if (p.order_here) {
    const size_t n1q = (size_t)b.nq + 1;
    uint32_t* const qoff = qcnt + n1q;
    HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, qcnt, qoff, n1q, h->stream));
    HS_HIP(h, hs_launch_hit_order(h->hit_key.as<uint64_t>(), h->hit_val.as<uint64_t>(), d_cnt + 1, hit_cap, b.q_base,
                                  b.nq, qoff, h->hit_rank.as<uint32_t>(), h->hit_kv.p, d_cnt + 20, qoff + 2 * n1q,
                                  bout->q, bout->id, bout->table, bout->dist, bout->room, h->n_cu, h->stream));
  }
  return HS_OK;
}

// One pass of a search batch's filters and exact decision; the counters and what the accounting and the
// history need read back behind them.
static hs_status search_pass(hs_handle* h, const QueryCall& c, const BatchPlan& p, Batch& b, uint32_t prov_cap,
                             uint32_t hit_cap, bool again, BatchOut* bout) {
  uint32_t* const d_cnt = h->counters.as<uint32_t>();
  if (p.order_here) {
    const size_t n1q = (size_t)b.nq + 1;
    HS_HIP(h, h->qhits.reserve((6 * n1q + 8) * 4));
    // per-query hit counts, offsets, fill, and behind them the lists of the queries a block orders
    if (again) {  // (first pass: the batch's reset)
      HS_HIP(h, hipMemsetAsync(h->qhits.p, 0, (3 * n1q + 8) * 4, h->stream));
      HS_HIP(h, hipMemsetAsync(d_cnt + 20, 0, 4, h->stream));  // the "too many hits" flag
    }
    HS_HIP(h, h->hit_kv.reserve((size_t)hit_cap * 16));
    HS_HIP(h, h->hit_rank.reserve((size_t)hit_cap * 4));
    HS_HIP(h, h->temp.reserve(hs_scan_u32_temp(n1q) + 256));
  }
  HS_HIP(h, hipEventRecord(h->ev[3], h->stream));
  if (again) HS_HIP(h, hipMemsetAsync(d_cnt + 32, 0, 64, h->stream));  // the item counters again
  HS_CHECK(launch_filters(h, p, b, prov_cap, again));
  HS_HIP(h, hipEventRecord(h->ev[4], h->stream));
  HS_CHECK(finalize_hits(h, c, p, b, prov_cap, hit_cap, again, bout));
  HS_HIP(h, hipEventRecord(h->ev[5], h->stream));
  // ONE copy of the whole block: [0] survivors [1] hits [2..3] candidates ... [10..13] join statistics [20] order
  // fallback, [HS_CNT_PROJ] the projection of the queries, [HS_CNT_SPLIT] first item of the few-query class and
  // the items -- under async_items the real item count -- both written there by their kernels
  HS_HIP(h, hipMemcpyAsync(h->pin_cnt, d_cnt, HS_CNT_WORDS * 4, hipMemcpyDeviceToHost, h->stream));
  return HS_OK;
}

// Brute force: every query against every indexed k-mer (packed_all) through the streaming filter's tables
static hs_status brute_batch(hs_handle* h, const QueryCall& c, uint32_t nq, uint32_t q_base, uint32_t* n_hits) {
  const int k = (int)h->p.k;
  const double r2 = c.R * c.R;  // motif_both_points.cpp:204
  const float r2_hi = filter_bound(r2);
  uint32_t* const d_cnt = h->counters.as<uint32_t>();
  HS_HIP(h, hipMemsetAsync(d_cnt, 0, 256, h->stream));
  HS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  HS_HIP(h, h->tq.reserve((size_t)nq * k * HS_TROW * 4));
  HS_HIP(h, hs_launch_qtables(c.centers, nq, k, h->coords.as<double>(), h->alphabet, h->tq.as<float>(), h->stream));
  HS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  HS_CHECK(filter_passes(h, nq, 0, false, n_hits, [&](uint32_t prov_cap, uint32_t hit_cap, bool again) -> hs_status {
    HS_HIP(h, hipEventRecord(h->ev[3], h->stream));
    if (again) HS_HIP(h, hipMemsetAsync(d_cnt + 32, 0, 64, h->stream));
    HS_HIP(h, hs_launch_bruteforce(h->packed_all.as<uint4>(), (uint32_t)h->n, h->tq.as<float>(), nq, k, r2_hi, d_cnt,
                                   prov_cap, h->prov.as<uint2>(), nullptr, nullptr, h->n_cu * 8, h->stream, c.radii));
    HS_HIP(h, hipEventRecord(h->ev[4], h->stream));
    HS_HIP(h, hs_launch_bf_finalize(h->codes.as<uint8_t>(), c.centers, h->coords.as<double>(), h->prov.as<uint2>(),
                                    d_cnt, prov_cap, k, c.R, q_base, d_cnt + 1, hit_cap, h->hit_key.as<uint64_t>(),
                                    h->hit_val.as<uint64_t>(), h->stream, c.radii));
    HS_HIP(h, hipEventRecord(h->ev[5], h->stream));
    HS_HIP(h, hipMemcpyAsync(h->pin_cnt, d_cnt, 96, hipMemcpyDeviceToHost, h->stream));
    return HS_OK;
  }));
  h->prof.candidates += (uint64_t)nq * h->n;
  return HS_OK;
}

// Stage 7: a finished search batch's counters into the profile
static void account_batch(hs_handle* h, const BatchPlan& p, Batch& b) {
  const uint32_t* const cnt = h->pin_cnt;
  if (!p.self_codes && use_projection(h)) {
    h->prof.hash_values += (uint64_t)b.nq * h->LK;
    h->prof.hash_flagged += cnt[HS_CNT_PROJ + 1];
  }
  uint64_t cand_total;
  memcpy(&cand_total, cnt + 2, 8);
  h->prof.candidates += cand_total;
  h->prof.join_batches += b.n_items ? 1 : 0;
  h->prof.join_i8_batches += (b.n_items && p.use_i8) ? 1 : 0;
  // (an FP6 batch counts as an int8 one as well, with the same depth-128 row: what is priced is the GEMM)
  h->prof.join_f6_batches += (b.n_items && p.use_i8 && p.f6) ? 1 : 0;
  if (b.n_items && p.use_i8) {
    h->prof.join_row_bytes = (uint32_t)hs_join8_row_bytes((int)h->p.k, p.wide);
    h->prof.join_wide = (uint32_t)p.wide;
  }
  if (p.async_items) b.n_items = cnt[HS_CNT_SPLIT + 1];
  h->prof.join_items += b.n_items;
  if (p.use_i8 && b.n_items && p.use_r && cnt[HS_CNT_SPLIT + 1])
    h->prof.join_items_resident += cnt[HS_CNT_SPLIT + 1] - cnt[HS_CNT_SPLIT];
  if (p.use_i8 && b.n_items && p.f6 && p.jm_stream)  // (the items in front of the resident kernel's class)
    h->prof.join_f6_wide_items += (p.use_r && cnt[HS_CNT_SPLIT + 1]) ? cnt[HS_CNT_SPLIT] : b.n_items;
  if (p.use_join) {
    unsigned long long js[2] = {0, 0};
    memcpy(js, cnt + 10, 16);  // the join statistics (d_cnt + 10), read back with the counters
    h->prof.join_pairs_issued += js[0];
    h->prof.join_pairs += js[1];
  }
}

// What a batch leaves for the next ones (BatchHistory): written here alone, after its counters are back.
static void learn_from_batch(hs_handle* h, const QueryCall& c, const BatchPlan& p, const Batch& b, hs_status st) {
  BatchHistory& m = h->hist;
  if (p.resident_stale) m.resident_share = -1.0;
  if (st != HS_OK) return;
  const uint32_t* const cnt = h->pin_cnt;
  if (p.order_here) {
    m.order_failed = cnt[20] != 0;
    m.order_failed_R = c.radii ? (double)NAN : c.R;
  }
  if (!p.use_i8 || !b.n_items) return;
  m.item_cap_hint = b.n_items + b.n_items / 4 + 4096;
  ++m.resident_age;
  if (p.use_r && cnt[HS_CNT_SPLIT + 1]) {
    m.resident_age = 0;
    m.resident_nq = b.nq;
    m.resident_share = (double)(cnt[HS_CNT_SPLIT + 1] - cnt[HS_CNT_SPLIT]) / (double)cnt[HS_CNT_SPLIT + 1];
  }
  unsigned long long issued = 0;
  memcpy(&issued, cnt + 10, 8);
  m.pairs_per_item = (double)issued / (double)b.n_items;
}

// Everything of a batch that starts from zero and whose place and size are known before its first kernel, in ONE
// launch at its head (they were a dozen fills of 5 us each, most of them 4 bytes long): the counters, the slow
// probes' list, the closing word of the slice counts, and with a join ahead the segment counts, the bucket
// counters of the counting sort, and the slice offsets where no probe writes a count; the per-query hit counts
// where the batch orders its hits.  The stages reserve the same buffers again (no-ops).  What a later pass of
// the same batch needs cleared again (`again`, demote, the HS_SYNC_ITEMS retry through here) is re-issued there.
static hs_status reset_batch(hs_handle* h, const BatchPlan& p, const Batch& b) {
  const size_t n1 = (size_t)b.nql + 1, n1q = (size_t)b.nq + 1;
  hs_zero_ranges z{};
  auto add = [&](void* ptr, uint64_t words) {
    z.p[z.n] = static_cast<uint32_t*>(ptr);
    z.words[z.n++] = words;
  };
  for (DevBuf* d : {&h->nslices, &h->probe_slow, &h->slice_off}) HS_HIP(h, d->reserve(n1 * 4));
  add(h->counters.p, 64);  // incl. the join's item counter (d_cnt + 32)
  add(h->probe_slow.p, 1);
  add(h->nslices.as<uint32_t>() + b.nql, 1);
  if (p.use_join) {
    HS_HIP(h, h->seg_cnt.reserve(n1 * 4));
    add(h->seg_cnt.p, n1);
    if (p.no_slices) add(h->slice_off.p, n1);
    if (!p.seg_sparse) {
      HS_HIP(h, h->bucket_work.reserve(4 * ((size_t)h->nb_total + 2) * 4));
      add(h->bucket_work.p, (uint64_t)h->nb_total + 2);
    }
  }
  if (p.order_here) {
    HS_HIP(h, h->qhits.reserve((6 * n1q + 8) * 4));
    add(h->qhits.p, 3 * n1q + 8);
  }
  static_assert(HS_ZERO_RANGES >= 7, "reset_batch lists up to 7 ranges");
  HS_HIP(h, hs_launch_zero_ranges(z, h->stream));
  return HS_OK;
}

// One batch of a call: brute force, or the search stages in order.  A batch that left its item count on the
// device and found it too small runs once more with the count read back first.
static hs_status query_batch(hs_handle* h, const QueryCall& c, uint32_t nq, uint32_t q_base, uint64_t* d_cand,
                             uint32_t* n_hits, BatchOut* bout) {
  if (c.brute) return brute_batch(h, c, nq, q_base, n_hits);
  for (bool allow_async = true;; allow_async = false) {
    BatchPlan p = plan_batch(h, c, nq, allow_async, bout != nullptr);
    if (p.f6 && !ensure_rec6(h)) {  // the int8 kernel takes the batch, on ITS items: 128 members, not 192
      p.f6 = false;
      p.jm_stream = 0;
    }
    const uint32_t nql = nq * (uint32_t)h->p.L;
    Batch b{nq, q_base, nql, nql, c.R * c.R, c.centers, d_cand};
    b.radii = c.radii;
    HS_HIP(h, hipEventRecord(h->ev[0], h->stream));  // (the reset counts as part of the batch's first phase)
    HS_CHECK(reset_batch(h, p, b));
    HS_CHECK(prepare_queries(h, c, p, b));
    HS_CHECK(hash_and_probe(h, c, p, b));
    HS_CHECK(group_segments(h, p, b));
    HS_CHECK(read_items(h, c, p, b));
    HS_HIP(h, hipEventRecord(h->ev[2], h->stream));
    const hs_status st = filter_passes(h, nq, p.item_cap, b.n_items != 0, n_hits,
                                       [&](uint32_t prov_cap, uint32_t hit_cap, bool again) {
                                         return search_pass(h, c, p, b, prov_cap, hit_cap, again, bout);
                                       });
    if (st == HS_SYNC_ITEMS) {
      ++h->prof.join_async_retries;  // (measurements can exclude such a call: its join ran twice)
      continue;
    }
    if (st == HS_OK) {
      account_batch(h, p, b);
      if (bout) bout->ordered = p.order_here && !h->pin_cnt[20];
    }
    learn_from_batch(h, c, p, b, st);
    return st;
  }
}

static hs_status mp_query(hs_handle* h, const QueryCall& c, uint64_t nq, uint32_t* d_hit_q, uint32_t* d_hit_id,
                          uint32_t* d_hit_table, double* d_hit_dist, uint64_t cap, uint64_t* n_hits, uint64_t* d_cand);

// hs_annotate: n hits -- a batch's (key, value) pairs, or with d_key == null the four arrays of a merged list --
// into the handle's nearest-centre state (annot_begin has prepared it), on the handle's stream
static hs_status annot_reduce(hs_handle* h, const uint64_t* d_key, const uint64_t* d_val, const uint32_t* d_q,
                              const uint32_t* d_id, const uint32_t* d_table, const double* d_dist, uint64_t n) {
  HS_HIP(h, hs_launch_annot_reduce(d_key, d_val, d_q, d_id, d_table, d_dist, (uint32_t)n, h->ann_dist.as<uint64_t>(),
                                   h->ann_tq.as<uint32_t>(), (uint32_t)h->n, h->ann_touched.as<uint32_t>(),
                                   h->ann_cnt.as<uint32_t>(), h->stream));
  return HS_OK;
}

// The one place a batch's hits leave for a sink other than LIST: the nh (key, value) pairs finalize_hits left in
// hit_key / hit_val, on the handle's stream.  The kernels below are launched from here and nowhere else (annot_reduce
// once more by mp_query, on a chunk's merged list: its probe rows run with the LIST sink).  The rule for every
// sink: it sees each batch's hits exactly once, and only after the batch succeeded.  run_query keeps it --
// a batch cut in halves (HS_SPLIT_BATCH) has `continue`d before handing anything on, and its halves bring each hit
// once -- and hit_key holds each ordered pair once (the first-seen rule across the tables has run; the tests pin
// n_edges == len(self_join)).  DB_DEGREE depends on it: it is NOT idempotent, a pair counted twice is a wrong
// degree.  The other three would forgive a repeat (union, min and the nearest-centre steps are idempotent).
// MSF_COLLECT: step 1 over the batch, its pairs with a < b appended to the kept list.  The list grows to hold them: the
// batch brings at most nh entries on top of those counted so far (read back here: the stream is idle between
// batches), never beyond the call's budget.  A list that cannot hold its pairs is not an error: the kernel stops
// appending, the counter keeps running, and hs_msf goes on without the list.
static hs_status msf_grow_kept(hs_handle* h, uint32_t nh) {
  uint64_t* const cnt = h->msf_cnt.as<uint64_t>();
  uint64_t kept = 0;
  HS_HIP(h, hipMemcpyAsync(&kept, cnt + 2, 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  const uint64_t budget = h->msf_kept_budget, have = h->msf_kept.cap / 16;
  const uint64_t need = std::min<uint64_t>(budget, kept + nh);
  if (need > have && kept <= have && !h->msf_kept_failed) {
    DevBuf bigger;
    const uint64_t entries = std::min<uint64_t>(budget, std::max<uint64_t>(need, 2 * have));
    if (bigger.reserve((size_t)entries * 16) != hipSuccess) {
      (void)hipGetLastError();
      h->msf_kept_failed = true;
    } else {
      hipError_t e = hipSuccess;
      if (kept) e = hipMemcpyAsync(bigger.p, h->msf_kept.p, (size_t)kept * 16, hipMemcpyDeviceToDevice, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      if (e != hipSuccess) bigger.release();  // (DevBuf has no destructor)
      HS_HIP(h, e);
      h->msf_kept.release();
      h->msf_kept = bigger;
    }
  }
  return HS_OK;
}

static hs_status msf_collect_batch(hs_handle* h, const QueryCall& c, uint32_t nh) {
  if (!nh) return HS_OK;
  HS_CHECK(msf_grow_kept(h, nh));
  uint64_t* const cnt = h->msf_cnt.as<uint64_t>();
  const uint64_t budget = h->msf_kept_budget;
  HS_HIP(h, hs_launch_msf_min_d_hits(h->hit_key.as<uint64_t>(), h->hit_val.as<uint64_t>(), nh, c.self_first,
                                     h->msf_comp.as<uint32_t>(), h->msf_best_d.as<uint64_t>(), (uint32_t)h->n, cnt,
                                     h->msf_kept.p, std::min<uint64_t>(budget, h->msf_kept.cap / 16), h->stream));
  return HS_OK;
}

// hs_density.hip's core pass over one batch: its queries are the k-mers [first, first + count), and ALL hits of such a
// k-mer lie in this batch's nh (run_query batches by query and hands a batch on once, whole), each ordered pair once.
// The pairs are counted (and, collecting, kept with their raw distance); then at most min_pts - 1 threshold rounds,
// the count of k-mers still open read back after each (the stream is idle between batches) and zero ending them.
static hs_status dt_core_batch(hs_handle* h, const QueryCall& c, uint32_t nh, uint32_t first, uint32_t count) {
  uint64_t* const cnt = h->msf_cnt.as<uint64_t>();
  const uint32_t n = (uint32_t)h->n;
  const bool collect = c.sink.kind == HitSink::DT_CORE_COLLECT;
  if (collect && nh) HS_CHECK(msf_grow_kept(h, nh));
  HS_HIP(h, hs_launch_dt_pairs(h->hit_key.as<uint64_t>(), h->hit_val.as<uint64_t>(), nh, c.self_first, n, cnt,
                               collect ? h->msf_kept.p : nullptr,
                               std::min<uint64_t>(h->msf_kept_budget, h->msf_kept.cap / 16), h->stream));
  for (uint32_t round = 1; round < c.sink.min_pts; ++round) {
    HS_HIP(h, hipMemsetAsync(cnt + 6, 0, 8, h->stream));
    HS_HIP(h, hs_launch_dt_round(h->hit_key.as<uint64_t>(), h->hit_val.as<uint64_t>(), nh, c.self_first, n, first, count,
                                 c.sink.min_pts, h->dt_core.as<uint64_t>(), h->dt_thr.as<uint64_t>(),
                                 h->dt_next.as<uint64_t>(), h->dt_cnt.as<uint32_t>(), cnt, h->stream));
    uint64_t open = 0;
    HS_HIP(h, hipMemcpyAsync(&open, cnt + 6, 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    if (!open) break;
  }
  return HS_OK;
}

// hs_knn.hip over n hits -- a batch's (key, value) pairs, or with d_key == null the four arrays of a merged list --
// whose queries are [first, first + count) of the call: ALL hits of such a query are among them, each once (a batch
// and a multi-probe chunk are ranges of queries, handed on whole), so their rows are final.  hit_key2 / hit_val2 take
// the hits grouped by query: only a batch that sorts its hit LIST uses them (sort_batch_hits), and a merged list has
// left them.  On the handle's stream.
static hs_status topk_reduce(hs_handle* h, const QueryCall& c, const uint64_t* d_key, const uint64_t* d_val,
                             const uint32_t* d_q, const uint32_t* d_id, const uint32_t* d_table, const double* d_dist,
                             uint64_t n, uint32_t first, uint32_t count) {
  if (!count) return HS_OK;
  if (n >= (1ull << 32)) return fail(h, HS_ERR_CAPACITY, "more than 2^32 - 1 hits in one batch");
  const size_t words = ((size_t)count + 1) * 4;
  HS_HIP(h, h->knn_cnt.reserve(words));
  HS_HIP(h, h->knn_off.reserve(words));
  HS_HIP(h, h->knn_cur.reserve(words));
  HS_HIP(h, h->hit_key2.reserve(std::max<size_t>(16, (size_t)n * 8)));
  HS_HIP(h, h->hit_val2.reserve(std::max<size_t>(16, (size_t)n * 8)));
  HS_HIP(h, h->temp.reserve(hs_knn_temp(count) + 256));
  const HitSink& k = c.sink;
  HS_HIP(h, hs_launch_knn_batch(d_key, d_val, d_q, d_id, d_table, d_dist, (uint32_t)n, c.self_first, first, count,
                                h->knn_cnt.as<uint32_t>(), h->knn_off.as<uint32_t>(), h->knn_cur.as<uint32_t>(),
                                h->temp.p, h->temp.cap, h->hit_key2.as<uint64_t>(), h->hit_val2.as<uint64_t>(),
                                h->knn_total.as<uint64_t>(), k.topk, k.row0, k.nn_id, k.nn_table, k.nn_dist, k.nn_count,
                                h->stream));
  return HS_OK;
}

// hs_seqmatch.hip's passes over n sorted-to-be elements whose keys are in sq_key and indices in sq_idx: sort, run heads,
// scan, the number of runs read back, then the runs reduced into rows row0 ... of the list `dst` (grown to hold them;
// keep: its first row0 rows stay).  The source is a batch's hits (the five arrays) or the rows of `src`.
static hs_status seq_rows_reduce(hs_handle* h, const SeqMatchCall& sm, uint32_t n, const uint64_t* d_key,
                                 const uint64_t* d_val, const uint32_t* d_q, const uint32_t* d_id, const double* d_dist,
                                 const DevBuf* src, DevBuf* dst, uint64_t row0, uint32_t* n_rows) {
  HS_HIP(h, h->sq_skey.reserve((size_t)n * 8));
  HS_HIP(h, h->sq_sidx.reserve((size_t)n * 4));
  HS_HIP(h, h->sq_head.reserve(((size_t)n + 1) * 4));
  HS_HIP(h, h->sq_excl.reserve(((size_t)n + 1) * 4));
  HS_HIP(h, h->sq_part.reserve(hs_sm_part_bytes(n)));
  HS_HIP(h, h->temp.reserve(std::max(hs_sort_pairs_u64_u32_temp(n), hs_scan_u32_temp((size_t)n + 1)) + 256));
  HS_HIP(h, hs_sort_pairs_u64_u32(h->temp.p, h->temp.cap, h->sq_key.as<uint64_t>(), h->sq_skey.as<uint64_t>(),
                                  h->sq_idx.as<uint32_t>(), h->sq_sidx.as<uint32_t>(), n, 0,
                                  std::max(1, sm.wg + sm.ws + sm.wd), h->stream));
  HS_HIP(h, hs_launch_sm_head(h->sq_skey.as<uint64_t>(), n, h->sq_head.as<uint32_t>(), h->stream));
  HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, h->sq_head.as<uint32_t>(), h->sq_excl.as<uint32_t>(),
                                  (size_t)n + 1, h->stream));
  uint32_t rows = 0;
  HS_HIP(h, hipMemcpyAsync(&rows, h->sq_excl.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (!rows || rows > n) return fail(h, HS_ERR_HIP, "hs_seq_match: the run count of a batch is out of range");
  const uint64_t have = dst->cap / 40, need = row0 + rows;
  if (need > have) {  // by doubling; the rows kept move to the new list's arrays
    DevBuf bigger;
    const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(need, 2 * have), 1024);
    HS_HIP(h, bigger.reserve((size_t)cap * 40));
    hipError_t e = hipSuccess;
    static const int at[6] = {0, 8, 16, 24, 32, 36}, width[6] = {8, 8, 8, 8, 4, 4};
    for (int a = 0; a < 6 && row0 && e == hipSuccess; ++a)
      e = hipMemcpyAsync(static_cast<char*>(bigger.p) + cap * at[a], static_cast<char*>(dst->p) + have * at[a],
                         (size_t)row0 * width[a], hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) bigger.release();  // (DevBuf has no destructor)
    HS_HIP(h, e);
    dst->release();
    *dst = bigger;
  }
  HS_HIP(h, hs_launch_sm_reduce(h->sq_skey.as<uint64_t>(), h->sq_sidx.as<uint32_t>(), h->sq_excl.as<uint32_t>(),
                                h->sq_head.as<uint32_t>(), n, d_key, d_val, d_q, d_id, d_dist, sm.id_start, sm.ws, sm.wd,
                                src ? src->p : nullptr, src ? src->cap / 40 : 0, dst->p, dst->cap / 40, row0, rows,
                                h->sq_part.p, h->stream));
  *n_rows = rows;
  return HS_OK;
}

// hs_seq_match: n hits -- a batch's (key, value) pairs, or with d_key == null the arrays of a merged list -- reduced to
// rows and appended to the call's list (seq_begin has emptied it), on the handle's stream
static hs_status seq_reduce(hs_handle* h, const QueryCall& c, const uint64_t* d_key, const uint64_t* d_val,
                            const uint32_t* d_q, const uint32_t* d_id, const double* d_dist, uint64_t n) {
  if (!n) return HS_OK;
  if (n >= (1ull << 32)) return fail(h, HS_ERR_CAPACITY, "more than 2^32 - 1 hits in one batch");
  const SeqMatchCall& sm = *c.sink.sm;
  HS_HIP(h, h->sq_key.reserve((size_t)n * 8));
  HS_HIP(h, h->sq_idx.reserve((size_t)n * 4));
  HS_HIP(h, hs_launch_sm_key(d_key, d_val, d_q, d_id, d_dist, (uint32_t)n, sm.q_group, sm.q_off, sm.id_start, sm.n_seq,
                             sm.ws, sm.wd, sm.max_qoff, h->sq_key.as<uint64_t>(), h->sq_idx.as<uint32_t>(), h->stream));
  uint32_t rows = 0;
  HS_CHECK(seq_rows_reduce(h, sm, (uint32_t)n, d_key, d_val, d_q, d_id, d_dist, nullptr, &h->sq_acc, h->sq_rows, &rows));
  h->sq_rows += rows;
  ++h->sq_batches;
  return HS_OK;
}

// first, count: the batch's queries within the call (for a self-join the k-mers c.self_first + first ...)
static hs_status reduce_batch(hs_handle* h, const QueryCall& c, uint32_t nh, uint32_t first, uint32_t count) {
  const uint64_t* const pairs = h->hit_key.as<uint64_t>();
  const uint32_t n = (uint32_t)h->n;
  switch (c.sink.kind) {
    case HitSink::LIST:
      break;
    case HitSink::ANNOTATE:
      return annot_reduce(h, pairs, h->hit_val.as<uint64_t>(), nullptr, nullptr, nullptr, nullptr, nh);
    case HitSink::CC_UNION:
      HS_HIP(h, hs_launch_cc_union(pairs, nh, c.self_first, h->cc_parent.as<uint32_t>(), n, h->cc_cnt.as<uint64_t>(),
                                   h->stream));
      break;
    case HitSink::DB_DEGREE:
      HS_HIP(h, hs_launch_db_degree(pairs, nh, c.self_first, h->db_deg.as<uint32_t>(), n, h->db_cnt.as<uint64_t>(),
                                    h->stream));
      break;
    case HitSink::DB_UNITE:  // the degrees are final (pass 1 ended at a kernel boundary)
      HS_HIP(h, hs_launch_db_unite(pairs, nh, c.self_first, h->db_deg.as<uint32_t>(), c.sink.min_pts,
                                   h->cc_parent.as<uint32_t>(), h->db_anchor.as<uint32_t>(), n, h->stream));
      break;
    case HitSink::MSF_MIN_D:
      HS_HIP(h, hs_launch_msf_min_d_hits(pairs, h->hit_val.as<uint64_t>(), nh, c.self_first, h->msf_comp.as<uint32_t>(),
                                         h->msf_best_d.as<uint64_t>(), n, h->msf_cnt.as<uint64_t>(), nullptr, 0,
                                         h->stream));
      break;
    case HitSink::MSF_MIN_PAIR:  // the slots' distances are final (step 1 ended at a kernel boundary)
      HS_HIP(h, hs_launch_msf_min_pair_hits(pairs, h->hit_val.as<uint64_t>(), nh, c.self_first,
                                            h->msf_comp.as<uint32_t>(), h->msf_best_d.as<uint64_t>(),
                                            h->msf_best_pair.as<uint64_t>(), n, h->stream));
      break;
    case HitSink::MSF_COLLECT:
      return msf_collect_batch(h, c, nh);
    case HitSink::DT_CORE:
    case HitSink::DT_CORE_COLLECT:
      return dt_core_batch(h, c, nh, c.self_first + first, count);
    case HitSink::DT_MIN_D:
      HS_HIP(h, hs_launch_dt_min_d_hits(pairs, h->hit_val.as<uint64_t>(), nh, c.self_first, h->dt_core.as<uint64_t>(),
                                        h->msf_comp.as<uint32_t>(), h->msf_best_d.as<uint64_t>(), n,
                                        h->msf_cnt.as<uint64_t>(), h->stream));
      break;
    case HitSink::DT_MIN_PAIR:
      HS_HIP(h, hs_launch_dt_min_pair_hits(pairs, h->hit_val.as<uint64_t>(), nh, c.self_first,
                                           h->dt_core.as<uint64_t>(), h->msf_comp.as<uint32_t>(),
                                           h->msf_best_d.as<uint64_t>(), h->msf_best_pair.as<uint64_t>(), n, h->stream));
      break;
    case HitSink::TOPK:
      return topk_reduce(h, c, pairs, h->hit_val.as<uint64_t>(), nullptr, nullptr, nullptr, nullptr, nh, first, count);
    case HitSink::SEQ_MATCH:
      return seq_reduce(h, c, pairs, h->hit_val.as<uint64_t>(), nullptr, nullptr, nullptr, nh);
  }
  return HS_OK;
}

// Centres that are k-mers (every 8 doubles a row of the coordinate table, bit for bit -- what the
// reference's centres files hold) run from their residue codes, as hs_query_codes's do: the same
// results from k bytes per query where the point rows are 64 k.  One small kernel and one wait per call; the flag
// comes back into pinned memory.
static hs_status recognise_kmers(hs_handle* h, QueryCall& c, uint64_t nq) {
  if (!c.centers || c.codes || !nq || !h->n || c.brute || h->knobs.no_recognise || h->p.k > 75) return HS_OK;
  const size_t cb = ((size_t)nq * h->p.k + 15) & ~(size_t)15;
  HS_HIP(h, h->rec_codes.reserve(cb + 16));
  uint32_t* const d_bad = reinterpret_cast<uint32_t*>(h->rec_codes.as<uint8_t>() + cb);
  HS_HIP(h, hipMemsetAsync(d_bad, 0, 4, h->stream));
  HS_HIP(h, hs_launch_recognise_kmers(c.centers, nq, h->p.k, h->coords.as<double>(), h->alphabet,
                                      h->rec_codes.as<uint8_t>(), d_bad, h->stream));
  // (the flag lands in pinned memory, in the last word of the block a pass's counters land in: a copy into
  // pageable memory costs tens of us)
  HS_CHECK(ensure_pin_cnt(h));
  volatile uint32_t* const bad = h->pin_cnt + (HS_CNT_WORDS - 1);
  *bad = 1;
  HS_HIP(h, hipMemcpyAsync(h->pin_cnt + (HS_CNT_WORDS - 1), d_bad, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (!*bad) {
    c.codes = h->rec_codes.as<uint8_t>();
    c.centers = nullptr;
    h->prof.queries_recognised = nq;
  }
  return HS_OK;
}

// Queries per batch of a call of nq queries
static uint32_t choose_query_batch(const hs_handle* h, const QueryCall& c, uint64_t nq) {
  // bounds the workspace, which grows with nq * L (2^17 at L >= 8; with few
  // tables -- the one-table indexes of Clustering() -- larger batches, fewer fixed costs)
  uint32_t QB = std::max(1u << 17, std::min(1u << 20, (1u << 20) / h->p.L));
  if (nq > QB && !c.brute && !h->knobs.query_batch) {
    // More queries than one such batch: as many per batch as a third of the free HBM carries, up to 2^20.
    // The pairs of a batch are (bucket members) x (queries probing the bucket), so the join's operand reuse
    // grows with the batch: at 10^8 k-mers x 32 tables a segment sees ~19 of 125 k queries, ~150 of 10^6.
    // Workspace per query: L x (K + 5 + 18 + 4) words of probe / segment arrays, L x 416 B of gathered
    // query rows + 32 B per work item (~ 1 per probe at worst), its own rows, 16 x 48 B of survivor lists.
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const size_t per_q = (size_t)h->p.L * (4 * ((size_t)h->p.K + 27) + 416 + 64) + 416 + 3 * (size_t)h->d + 768;
      const size_t fit = free_b / 3 / per_q;
      QB = (uint32_t)std::max<size_t>(QB, std::min<size_t>((size_t)1 << 20, fit));
    }
  }
  // hs_set_option(HS_OPT_QUERY_BATCH) / HS_QUERY_BATCH (multi-probe: in queries, each 1 + T probe rows here)
  if (h->knobs.query_batch) QB = (uint32_t)std::min<uint64_t>((uint64_t)h->knobs.query_batch * (c.pre_ints ? h->mp_T + 1 : 1), 1u << 30);
  return std::min(QB, max_query_batch(h));
}

// (brute force, a query with very many hits, HS_SORT_HITS) A batch that did not order its nh hits itself: the order
// of the reference's output by a radix sort on (query, table of first sight, id) -- q_bits bits of query number --
// and, where they fit, the hits into out's arrays
static hs_status sort_batch_hits(hs_handle* h, uint32_t nh, int q_bits, const BatchOut& out) {
  HS_HIP(h, h->hit_key2.reserve((size_t)nh * 8));
  HS_HIP(h, h->hit_val2.reserve((size_t)nh * 8));
  HS_HIP(h, h->temp.reserve(hs_sort_pairs_u64_u64_temp(nh) + 256));
  HS_HIP(h, hipEventRecord(h->ev[6], h->stream));
  HS_HIP(h, hs_sort_pairs_u64_u64(h->temp.p, h->temp.cap, h->hit_key.as<uint64_t>(), h->hit_key2.as<uint64_t>(),
                                  h->hit_val.as<uint64_t>(), h->hit_val2.as<uint64_t>(), nh, 37 + q_bits, h->stream));
  if (nh <= out.room)
    HS_HIP(h, hs_launch_unpack_hits(h->hit_key2.as<uint64_t>(), h->hit_val2.as<uint64_t>(), nh, out.q, out.id,
                                    out.table, out.dist, h->stream));
  HS_HIP(h, hipEventRecord(h->ev[7], h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->prof.ms_finalize += ev_ms(h, 6, 7);
  return HS_OK;
}

static hs_status run_query(hs_handle* h, QueryCall c, uint64_t nq, uint32_t* d_hit_q, uint32_t* d_hit_id,
                           uint32_t* d_hit_table, double* d_hit_dist, uint64_t cap, uint64_t* n_hits, uint64_t* d_cand) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  if (nq >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nq must be < 2^27 per call");
  // (a self-join that runs from the residue codes passes no centres)
  if (nq && !c.centers && !c.codes && !(c.self_first != HS_NO_SELF && self_codes_ok(h, c.R))) return HS_ERR_INVALID;
  if (cap && (c.sink.kind != HitSink::LIST || !d_hit_q || !d_hit_id || !d_hit_dist)) return HS_ERR_INVALID;
  if (!(c.R == c.R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  hs_status st = ensure_device(h);
  if (st) return st;
  if (h->mp_T && !c.brute && c.self_first == HS_NO_SELF && !c.pre_ints)
    return mp_query(h, c, nq, d_hit_q, d_hit_id, d_hit_table, d_hit_dist, cap, n_hits, d_cand);
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  HS_CHECK(recognise_kmers(h, c, nq));
  uint64_t total = 0;
  if (nq && h->n && !(c.brute && c.R < 0 && !c.radii)) {
    uint32_t QB = choose_query_batch(h, c, nq);
    uint32_t nqb = 0;
    for (uint64_t q0 = 0; q0 < nq; q0 += nqb) {
      nqb = (uint32_t)std::min<uint64_t>(QB, nq - q0);
      uint32_t nh = 0;
      const uint64_t at = std::min<uint64_t>(total, cap);
      BatchOut bout{d_hit_q + at, d_hit_id + at, d_hit_table ? d_hit_table + at : nullptr, d_hit_dist + at, cap - at};
      QueryCall bc = c;
      bc.centers = c.centers ? c.centers + q0 * h->d : nullptr;
      bc.codes = c.codes ? c.codes + q0 * h->p.k : nullptr;
      bc.pre_ints = c.pre_ints ? c.pre_ints + q0 * h->LK : nullptr;
      bc.pre_valid = c.pre_valid ? c.pre_valid + q0 * h->p.L : nullptr;
      bc.radii = c.radii ? c.radii + q0 : nullptr;
      st = query_batch(h, bc, nqb, (uint32_t)q0, d_cand ? d_cand + q0 * h->p.L : nullptr, &nh, cap ? &bout : nullptr);
      if (st == HS_SPLIT_BATCH) {
        // more filter survivors than the 32-bit list counter holds (a radius near the typical
        // distance of bucket mates): the same queries again in batches half the size
        if (nqb == 1) return fail(h, HS_ERR_CAPACITY, "the filter survivors of one query exceed 2^32");
        QB = (nqb + 1) / 2;
        nqb = 0;
        continue;
      }
      if (st) return st;
      // the batch came through whole (a split one has `continue`d above): its hits go on, once (reduce_batch)
      if (c.sink.kind != HitSink::LIST) {
        HS_CHECK(reduce_batch(h, c, nh, (uint32_t)q0, nqb));
        total += nh;
        continue;
      }
      if (nh && !bout.ordered) HS_CHECK(sort_batch_hits(h, nh, bit_width_u32((uint32_t)(q0 + nqb)), bout));
      total += nh;
    }
  } else if (d_cand && nq && !c.brute) {
    HS_HIP(h, hipMemsetAsync(d_cand, 0, (size_t)nq * h->p.L * 8, h->stream));
  }
  HS_HIP(h, hipEventRecord(h->ev[9], h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->prof.ms_total = ev_ms(h, 8, 9);
  h->prof.hits = total;
  *n_hits = total;
  if (total > cap && c.sink.kind == HitSink::LIST) return fail(h, HS_ERR_CAPACITY, "hit buffers too small; see *n_hits");
  return HS_OK;
}

// The profile of a call made of several run_query calls (multi-probe, the self-joins): the sum of its chunks' (the
// shape fields of the last one)
static void add_profile(hs_profile& a, const hs_profile& b) {
  a.ms_hash += b.ms_hash;
  a.ms_sort += b.ms_sort;
  a.ms_gather += b.ms_gather;
  a.ms_probe += b.ms_probe;
  a.ms_verify += b.ms_verify;
  a.ms_finalize += b.ms_finalize;
  a.ms_total += b.ms_total;
  a.candidates += b.candidates;
  a.provisional += b.provisional;
  a.verify_launches += b.verify_launches;
  a.join_batches += b.join_batches;
  a.ms_join += b.ms_join;
  a.join_items += b.join_items;
  a.join_pairs += b.join_pairs;
  a.join_pairs_issued += b.join_pairs_issued;
  a.join_i8_batches += b.join_i8_batches;
  a.join_f6_batches += b.join_f6_batches;
  a.join_f6_wide_items += b.join_f6_wide_items;
  a.hash_values += b.hash_values;
  a.hash_flagged += b.hash_flagged;
  a.join_row_bytes = b.join_row_bytes;
  a.join_wide = b.join_wide;
  a.join_items_resident += b.join_items_resident;
  a.join_async_retries += b.join_async_retries;
  a.queries_recognised += b.queries_recognised;
}

// The 1 + T probes of every (query, table) of n points (device): exact projections, then the probe sets, into
// mp_vints / mp_valid at slot q sq + l sl + t st.  On the handle's stream.
static hs_status mp_probes(hs_handle* h, const double* d_pts, uint64_t n, uint64_t sq, uint32_t sl, uint32_t st) {
  const uint32_t P = h->mp_T + 1;
  HS_HIP(h, h->mp_ints.reserve(std::max<size_t>(16, (size_t)n * h->LK * 4)));
  HS_HIP(h, h->mp_frac.reserve(std::max<size_t>(16, (size_t)n * h->LK * 8)));
  HS_HIP(h, h->mp_vints.reserve(std::max<size_t>(16, (size_t)n * P * h->LK * 4)));
  HS_HIP(h, h->mp_valid.reserve(std::max<size_t>(16, (size_t)n * P * h->p.L)));
  HS_HIP(h, hs_launch_mp_hash(d_pts, n, (int)h->p.k, h->aT.as<double>(), h->LK, h->b.as<double>(), h->p.W,
                              h->mp_ints.as<int32_t>(), h->mp_frac.as<double>(), h->stream));
  HS_HIP(h, hs_launch_mp_probe_sets(h->mp_ints.as<int32_t>(), h->mp_frac.as<double>(), n, (int)h->p.K, (int)h->p.L,
                                    (int)h->mp_T, h->mp_vints.as<int32_t>(), h->mp_valid.as<uint8_t>(), sq, sl, st,
                                    h->stream));
  return HS_OK;
}

// A search with T extra probes per table.  The queries run in chunks; in a chunk every query becomes 1 + T
// probe rows (row q P + t: probe t of every table), which the one-probe search below takes like queries of their
// own -- bucket ints given, empty probes flagged -- so every filter, grouping and partition applies unchanged.  A
// row reports an id at the smallest table whose probe t holds it; the rows' hits, mapped back to their query,
// keep per (query, id) the smallest table (hs_merge_first_table_dev): the first-seen rule over all (table, probe)
// pairs, in the order (query, table, id).
static hs_status mp_query(hs_handle* h, const QueryCall& c, uint64_t nq, uint32_t* d_hit_q, uint32_t* d_hit_id,
                          uint32_t* d_hit_table, double* d_hit_dist, uint64_t cap, uint64_t* n_hits, uint64_t* d_cand) {
  const uint32_t P = h->mp_T + 1, L = h->p.L;
  const int k = (int)h->p.k, d = h->d;
  hs_profile acc = {};
  uint64_t total = 0;
  const uint64_t NC = std::max<uint64_t>(1, (1u << 19) / P);  // queries per chunk: 2^19 probe rows
  uint64_t nc = 0;
  for (uint64_t q0 = 0; q0 < nq; q0 += nc) {
    nc = std::min(NC, nq - q0);
    const uint64_t nv = nc * P;
    HS_HIP(h, hipEventRecord(h->ev[0], h->stream));
    const double* pts = c.centers ? c.centers + q0 * d : nullptr;
    if (c.codes) {
      // (a checked copy: the embedding indexes the coordinate table; the search below reports bad codes itself)
      HS_HIP(h, h->mp_codes.reserve((size_t)nc * k + 16));
      HS_HIP(h, h->mp_pts.reserve((size_t)nc * d * 8));
      uint32_t* const d_bad = reinterpret_cast<uint32_t*>(h->mp_codes.as<uint8_t>() + (((size_t)nc * k + 3) & ~(size_t)3));
      HS_HIP(h, hs_launch_check_codes(c.codes + q0 * k, (uint64_t)nc * k, h->alphabet, h->mp_codes.as<uint8_t>(), d_bad,
                                      h->stream));
      HS_HIP(h, hs_launch_embed(h->mp_codes.as<uint8_t>(), nc, k, h->coords.as<double>(), h->mp_pts.as<double>(),
                                h->stream));
      pts = h->mp_pts.as<double>();
    }
    HS_CHECK(mp_probes(h, pts, nc, (uint64_t)P * L, 1, L));
    HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
    QueryCall vc = c;
    vc.sink = HitSink();  // (the probe rows' hits come back as a list: a row's table is final only once merged)
    if (c.codes) {
      HS_HIP(h, h->mp_rows.reserve((size_t)nv * k));
      HS_HIP(h, hs_launch_mp_repeat_u8(c.codes + q0 * k, nv, (uint32_t)k, P, h->mp_rows.as<uint8_t>(), h->stream));
      vc.codes = h->mp_rows.as<uint8_t>();
    } else {
      HS_HIP(h, h->mp_rows.reserve((size_t)nv * d * 8));
      HS_HIP(h, hs_launch_mp_repeat_f64(c.centers + q0 * d, nv, (uint32_t)d, P, h->mp_rows.as<double>(), h->stream));
      vc.centers = h->mp_rows.as<double>();
    }
    if (c.radii) {  // probe row q P + t searches at its query's radius
      HS_HIP(h, h->mp_radii.reserve(nv * 8));
      HS_HIP(h, hs_launch_mp_repeat_f64(c.radii + q0, nv, 1u, P, h->mp_radii.as<double>(), h->stream));
      vc.radii = h->mp_radii.as<double>();
    }
    vc.pre_ints = h->mp_vints.as<int32_t>();
    vc.pre_valid = h->mp_valid.as<uint8_t>();
    HS_HIP(h, hipStreamSynchronize(h->stream));
    const float ms_probes = ev_ms(h, 0, 1);
    if (d_cand) HS_HIP(h, h->mp_cand.reserve((size_t)nv * L * 8));
    uint64_t nh = 0;
    h->mp_room = std::max<uint64_t>(h->mp_room, 1u << 16);
    for (;;) {
      HS_HIP(h, h->mp_q.reserve(h->mp_room * 4));
      HS_HIP(h, h->mp_id.reserve(h->mp_room * 4));
      HS_HIP(h, h->mp_table.reserve(h->mp_room * 4));
      HS_HIP(h, h->mp_dist.reserve(h->mp_room * 8));
      const hs_status st = run_query(h, vc, nv, h->mp_q.as<uint32_t>(), h->mp_id.as<uint32_t>(),
                                     h->mp_table.as<uint32_t>(), h->mp_dist.as<double>(), h->mp_room, &nh,
                                     d_cand ? h->mp_cand.as<uint64_t>() : nullptr);
      if (st == HS_ERR_CAPACITY && nh > h->mp_room) {
        h->mp_room = nh + nh / 4;
        continue;
      }
      if (st) return st;
      break;
    }
    add_profile(acc, h->prof);
    acc.ms_hash += ms_probes;
    acc.ms_total += ms_probes;
    HS_HIP(h, hs_launch_mp_map_q(h->mp_q.as<uint32_t>(), nh, P, (uint32_t)q0, h->stream));
    uint64_t kept = 0;
    HS_CHECK(hs_merge_first_table_dev(h, h->mp_q.as<uint32_t>(), h->mp_id.as<uint32_t>(), h->mp_table.as<uint32_t>(),
                                      h->mp_dist.as<double>(), nh, &kept));
    if (c.sink.kind == HitSink::ANNOTATE) {  // the chunk's merged list -- bounded by the chunk -- is reduced where it lies
      HS_CHECK(annot_reduce(h, nullptr, nullptr, h->mp_q.as<uint32_t>(), h->mp_id.as<uint32_t>(),
                            h->mp_table.as<uint32_t>(), h->mp_dist.as<double>(), kept));
    } else if (c.sink.kind == HitSink::TOPK) {  // ... and selected: the chunk is a range of queries, its list whole
      HS_CHECK(topk_reduce(h, c, nullptr, nullptr, h->mp_q.as<uint32_t>(), h->mp_id.as<uint32_t>(),
                           h->mp_table.as<uint32_t>(), h->mp_dist.as<double>(), kept, (uint32_t)q0, (uint32_t)nc));
    } else if (c.sink.kind == HitSink::SEQ_MATCH) {  // ... and reduced to rows: one (q, id) once, as a batch brings it
      HS_CHECK(seq_reduce(h, c, nullptr, nullptr, h->mp_q.as<uint32_t>(), h->mp_id.as<uint32_t>(),
                          h->mp_dist.as<double>(), kept));
    } else if (kept && total + kept <= cap) {
      HS_HIP(h, hipMemcpyAsync(d_hit_q + total, h->mp_q.p, kept * 4, hipMemcpyDeviceToDevice, h->stream));
      HS_HIP(h, hipMemcpyAsync(d_hit_id + total, h->mp_id.p, kept * 4, hipMemcpyDeviceToDevice, h->stream));
      if (d_hit_table)
        HS_HIP(h, hipMemcpyAsync(d_hit_table + total, h->mp_table.p, kept * 4, hipMemcpyDeviceToDevice, h->stream));
      HS_HIP(h, hipMemcpyAsync(d_hit_dist + total, h->mp_dist.p, kept * 8, hipMemcpyDeviceToDevice, h->stream));
    }
    total += kept;
    if (d_cand) HS_HIP(h, hs_launch_mp_cand(h->mp_cand.as<uint64_t>(), nc, L, P, d_cand + q0 * L, h->stream));
  }
  HS_HIP(h, hipStreamSynchronize(h->stream));
  acc.hits = total;
  h->prof = acc;
  *n_hits = total;
  if (total > cap && c.sink.kind == HitSink::LIST) return fail(h, HS_ERR_CAPACITY, "hit buffers too small; see *n_hits");
  return HS_OK;
}

hs_status hs_set_multiprobe(hs_handle* h, uint32_t extra_probes) {
  if (!h) return HS_ERR_INVALID;
  if (extra_probes > 63) return fail(h, HS_ERR_INVALID, "hs_set_multiprobe: at most 63 extra probes");
  uint64_t sets = 1;  // 3^K - 1 valid perturbation sets exist
  for (uint32_t j = 0; j < h->p.K && sets <= 64; ++j) sets *= 3;
  if (sets - 1 < extra_probes)
    return fail(h, HS_ERR_INVALID, "hs_set_multiprobe: more extra probes than the 3^K - 1 perturbation sets of K");
  h->mp_T = extra_probes;
  return HS_OK;
}

hs_status hs_probe_buckets(hs_handle* h, const double* centers, uint64_t nq, int32_t* buckets, uint8_t* valid) {
  if (!h || (nq && (!centers || !buckets || !valid))) return HS_ERR_INVALID;
  if (!nq) return HS_OK;
  if (nq >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nq must be < 2^27 per call");
  hs_status st = ensure_device(h);
  if (st) return st;
  const uint32_t P = h->mp_T + 1, L = h->p.L;
  const size_t in_bytes = (size_t)nq * h->d * 8;
  HS_HIP(h, h->io_centers.reserve(in_bytes));
  HS_HIP(h, hipMemcpyAsync(h->io_centers.p, centers, in_bytes, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  HS_CHECK(mp_probes(h, h->io_centers.as<double>(), nq, (uint64_t)L * P, P, 1));
  HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  HS_HIP(h, hipMemcpyAsync(buckets, h->mp_vints.p, (size_t)nq * L * P * h->p.K * 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(valid, h->mp_valid.p, (size_t)nq * L * P, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  memset(&h->prof, 0, sizeof(h->prof));
  h->prof.ms_hash = h->prof.ms_total = ev_ms(h, 0, 1);
  return HS_OK;
}

hs_status hs_query_dev(hs_handle* h, const double* d_centers, uint64_t nq, double R,
                       uint32_t* d_hit_q, uint32_t* d_hit_id, uint32_t* d_hit_table,
                       double* d_hit_dist, uint64_t cap, uint64_t* n_hits, uint64_t* d_cand) {
  return run_query(h, {d_centers, nullptr, R}, nq, d_hit_q, d_hit_id, d_hit_table, d_hit_dist, cap, n_hits, d_cand);
}

hs_status hs_query_codes_dev(hs_handle* h, const uint8_t* d_qcodes, uint64_t nq, double R,
                             uint32_t* d_hit_q, uint32_t* d_hit_id, uint32_t* d_hit_table,
                             double* d_hit_dist, uint64_t cap, uint64_t* n_hits, uint64_t* d_cand) {
  if (nq && !d_qcodes) return HS_ERR_INVALID;
  return run_query(h, {nullptr, d_qcodes, R}, nq, d_hit_q, d_hit_id, d_hit_table, d_hit_dist, cap, n_hits, d_cand);
}

// What a radii call's plan is decided from: the largest |radii[q]| (0 for none); false: one of them is a NaN
static bool radii_max_host(const double* radii, uint64_t nq, double* out) {
  double m = 0.0;
  for (uint64_t q = 0; q < nq; ++q) {
    if (!(radii[q] == radii[q])) return false;
    m = std::max(m, fabs(radii[q]));
  }
  *out = m;
  return true;
}

// Host queries onto the device, on the handle's stream: centres (8d bytes per query over PCIe) or codes (k bytes)
// into io_centers / io_codes and, where given, the radii into io_radii; the call's pointers set to them
static hs_status stage_queries(hs_handle* h, const double* centers, const uint8_t* qcodes, const double* radii,
                               uint64_t nq, QueryCall* call) {
  const size_t cbytes = qcodes ? 0 : (size_t)nq * h->d * 8, kbytes = qcodes ? (size_t)nq * h->p.k : 0;
  HS_HIP(h, h->io_centers.reserve(std::max<size_t>(16, cbytes)));
  HS_HIP(h, h->io_codes.reserve(std::max<size_t>(16, kbytes)));
  if (cbytes) HS_HIP(h, hipMemcpyAsync(h->io_centers.p, centers, cbytes, hipMemcpyHostToDevice, h->stream));
  if (kbytes) HS_HIP(h, hipMemcpyAsync(h->io_codes.p, qcodes, kbytes, hipMemcpyHostToDevice, h->stream));
  call->centers = qcodes ? nullptr : h->io_centers.as<double>();
  call->codes = qcodes ? h->io_codes.as<uint8_t>() : nullptr;
  if (radii) {
    HS_HIP(h, h->io_radii.reserve(std::max<size_t>(16, (size_t)nq * 8)));
    if (nq) HS_HIP(h, hipMemcpyAsync(h->io_radii.p, radii, (size_t)nq * 8, hipMemcpyHostToDevice, h->stream));
    call->radii = h->io_radii.as<double>();
  }
  return HS_OK;
}

// radii != null: every query at its own radius (hs_query_radii, hs_bruteforce_radii), R unused
static hs_status host_query(hs_handle* h, const double* centers, const uint8_t* qcodes, uint64_t nq, double R,
                            bool brute, uint32_t* hit_q, uint32_t* hit_id, uint32_t* hit_table, double* hit_dist,
                            uint64_t cap, uint64_t* n_hits, uint64_t* cand, const double* radii = nullptr) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  if (nq && !centers && !qcodes) return HS_ERR_INVALID;
  if (radii && !radii_max_host(radii, nq, &R)) {
    *n_hits = 0;
    return fail(h, HS_ERR_INVALID, "a radius is NaN");
  }
  hs_status st = ensure_device(h);
  if (st) return st;
  HS_HIP(h, h->io_q.reserve(std::max<size_t>(16, cap * 4)));
  HS_HIP(h, h->io_id.reserve(std::max<size_t>(16, cap * 4)));
  HS_HIP(h, h->io_table.reserve(std::max<size_t>(16, cap * 4)));
  HS_HIP(h, h->io_dist.reserve(std::max<size_t>(16, cap * 8)));
  if (cand) HS_HIP(h, h->io_cand.reserve(std::max<size_t>(16, (size_t)nq * h->p.L * 8)));
  QueryCall call{nullptr, nullptr, R, brute};
  HS_CHECK(stage_queries(h, centers, qcodes, radii, nq, &call));
  st = run_query(h, call, nq, h->io_q.as<uint32_t>(), h->io_id.as<uint32_t>(), h->io_table.as<uint32_t>(),
                 h->io_dist.as<double>(), cap, n_hits, cand ? h->io_cand.as<uint64_t>() : nullptr);
  if (st != HS_OK) return st;
  const uint64_t nh = *n_hits;
  if (nh) {
    HS_HIP(h, hipMemcpyAsync(hit_q, h->io_q.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(hit_id, h->io_id.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
    if (hit_table)
      HS_HIP(h, hipMemcpyAsync(hit_table, h->io_table.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(hit_dist, h->io_dist.p, nh * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (cand && nq)
    HS_HIP(h, hipMemcpyAsync(cand, h->io_cand.p, (size_t)nq * h->p.L * 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

hs_status hs_query(hs_handle* h, const double* centers, uint64_t nq, double R, uint32_t* hit_q,
                   uint32_t* hit_id, uint32_t* hit_table, double* hit_dist, uint64_t cap,
                   uint64_t* n_hits, uint64_t* cand) {
  return host_query(h, centers, nullptr, nq, R, false, hit_q, hit_id, hit_table, hit_dist, cap, n_hits, cand);
}

hs_status hs_query_codes(hs_handle* h, const uint8_t* qcodes, uint64_t nq, double R, uint32_t* hit_q,
                         uint32_t* hit_id, uint32_t* hit_table, double* hit_dist, uint64_t cap,
                         uint64_t* n_hits, uint64_t* cand) {
  if (nq && !qcodes) return HS_ERR_INVALID;
  return host_query(h, nullptr, qcodes, nq, R, false, hit_q, hit_id, hit_table, hit_dist, cap, n_hits, cand);
}

hs_status hs_query_radii(hs_handle* h, const double* centers, const uint8_t* qcodes, uint64_t nq, const double* radii,
                         uint32_t* hit_q, uint32_t* hit_id, uint32_t* hit_table, double* hit_dist, uint64_t cap,
                         uint64_t* n_hits, uint64_t* cand) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  if ((centers != nullptr) == (qcodes != nullptr))
    return fail(h, HS_ERR_INVALID, "hs_query_radii: exactly one of centers and qcodes must be given");
  if (nq && !radii) return fail(h, HS_ERR_INVALID, "hs_query_radii: radii is null");
  static const double none = 0.0;  // (nq = 0: the array may be null)
  return host_query(h, centers, qcodes, nq, 0.0, false, hit_q, hit_id, hit_table, hit_dist, cap, n_hits, cand,
                    radii ? radii : &none);
}

hs_status hs_bruteforce_radii(hs_handle* h, const double* centers, uint64_t nq, const double* radii, uint32_t* hit_q,
                              uint32_t* hit_id, double* hit_dist, uint64_t cap, uint64_t* n_hits) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  if (nq && (!centers || !radii)) return fail(h, HS_ERR_INVALID, "hs_bruteforce_radii: centers or radii is null");
  static const double none = 0.0;
  return host_query(h, centers, nullptr, nq, 0.0, true, hit_q, hit_id, nullptr, hit_dist, cap, n_hits, nullptr,
                    radii ? radii : &none);
}

// Radii on the device stay where they are; what the plan needs of them -- the largest |radius|, and whether one is
// a NaN (HS_ERR_INVALID) -- comes from one small reduction and one read-back per call, before anything is written.
static hs_status radii_max_dev(hs_handle* h, const double* d_radii, uint64_t nq, double* out) {
  unsigned long long red[2] = {0ull, 0ull};
  HS_HIP(h, h->io_radii.reserve(16));
  HS_HIP(h, hipMemsetAsync(h->io_radii.p, 0, 16, h->stream));
  HS_HIP(h, hs_launch_radii_max(d_radii, nq, h->io_radii.as<unsigned long long>(), h->stream));
  HS_HIP(h, hipMemcpyAsync(red, h->io_radii.p, 16, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (red[1]) return fail(h, HS_ERR_INVALID, "a radius is NaN");
  memcpy(out, &red[0], 8);
  return HS_OK;
}

hs_status hs_query_radii_dev(hs_handle* h, const double* d_centers, const uint8_t* d_qcodes, uint64_t nq,
                             const double* d_radii, uint32_t* d_hit_q, uint32_t* d_hit_id, uint32_t* d_hit_table,
                             double* d_hit_dist, uint64_t cap, uint64_t* n_hits, uint64_t* d_cand) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  if ((d_centers != nullptr) == (d_qcodes != nullptr))
    return fail(h, HS_ERR_INVALID, "hs_query_radii_dev: exactly one of d_centers and d_qcodes must be given");
  if (nq && !d_radii) return fail(h, HS_ERR_INVALID, "hs_query_radii_dev: d_radii is null");
  if (nq >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nq must be < 2^27 per call");
  hs_status st = ensure_device(h);
  if (st) return st;
  QueryCall call{d_centers, d_qcodes, 0.0};
  HS_HIP(h, h->io_radii.reserve(16));
  if (nq) HS_CHECK(radii_max_dev(h, d_radii, nq, &call.R));
  call.radii = nq ? d_radii : h->io_radii.as<double>();  // (nq = 0: no kernel reads the array)
  return run_query(h, call, nq, d_hit_q, d_hit_id, d_hit_table, d_hit_dist, cap, n_hits, d_cand);
}

// ---- hs_annotate: the nearest centre of every DB k-mer (kernels and the rule: hs_annotate.hip) ----
// The handle's state ready for a call: slots sized by the index and empty, no id touched.  The slots come back
// empty from the call that used them (the gather empties what it reads); all n are cleared only when they are new
// or a call ended before its gather.
static hs_status annot_begin(hs_handle* h) {
  const size_t n = std::max<uint64_t>(h->n, 1);
  if (h->ann_dist.cap < n * 8) h->ann_clean = 0;
  HS_HIP(h, h->ann_dist.reserve(n * 8));
  HS_HIP(h, h->ann_tq.reserve(n * 4));
  HS_HIP(h, h->ann_touched.reserve(n * 4));
  HS_HIP(h, h->ann_cnt.reserve(16));
  if (h->ann_open || h->ann_clean < h->n) {
    HS_HIP(h, hipMemsetAsync(h->ann_dist.p, 0xff, n * 8, h->stream));
    h->ann_clean = h->n;
  }
  HS_HIP(h, hipMemsetAsync(h->ann_cnt.p, 0, 16, h->stream));
  h->ann_open = true;
  return HS_OK;
}

// The search with the reduction in place of the hit list; on success *cnt ids were touched and ann_sorted holds
// them ascending.  call: the queries on the device, with radii its R their largest |radius|.
static hs_status annot_search(hs_handle* h, QueryCall call, uint64_t nq, uint32_t* cnt) {
  *cnt = 0;
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  if (nq >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nq must be < 2^27 per call");
  if (!(call.R == call.R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  HS_CHECK(annot_begin(h));
  call.sink.kind = HitSink::ANNOTATE;
  uint64_t n_hits = 0;
  HS_CHECK(run_query(h, call, nq, nullptr, nullptr, nullptr, nullptr, 0, &n_hits, nullptr));
  HS_HIP(h, hipMemcpyAsync(cnt, h->ann_cnt.p, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (*cnt > h->n) return fail(h, HS_ERR_HIP, "hs_annotate: more ids touched than the index holds");
  if (*cnt) {
    HS_HIP(h, h->ann_sorted.reserve((size_t)*cnt * 4));
    HS_HIP(h, h->temp.reserve(hs_sort_keys_u32_temp(*cnt) + 256));
    HS_HIP(h, hs_sort_keys_u32(h->temp.p, h->temp.cap, h->ann_touched.as<uint32_t>(), h->ann_sorted.as<uint32_t>(), *cnt,
                               std::max(1, bit_width_u32((uint32_t)(h->n - 1))), h->stream));
  }
  return HS_OK;
}

// The rows into device arrays (null: the caller's capacity is too small, no rows) and the slots empty again
static hs_status annot_finish(hs_handle* h, uint32_t cnt, uint32_t* d_id, uint32_t* d_q, uint32_t* d_table,
                              double* d_dist) {
  HS_HIP(h, hs_launch_annot_gather(h->ann_sorted.as<uint32_t>(), cnt, h->ann_dist.as<uint64_t>(),
                                   h->ann_tq.as<uint32_t>(), (uint32_t)h->n, d_id, d_q, d_table, d_dist, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->ann_open = false;
  return HS_OK;
}

hs_status hs_annotate_dev(hs_handle* h, const double* d_centers, const uint8_t* d_qcodes, uint64_t nq, double R,
                          const double* d_radii, uint32_t* d_out_id, uint32_t* d_out_q, uint32_t* d_out_table,
                          double* d_out_dist, uint64_t cap, uint64_t* n_out) {
  if (!h || !n_out) return HS_ERR_INVALID;
  *n_out = 0;
  if ((d_centers != nullptr) == (d_qcodes != nullptr))
    return fail(h, HS_ERR_INVALID, "hs_annotate_dev: exactly one of d_centers and d_qcodes must be given");
  if (cap && (!d_out_id || !d_out_q || !d_out_table || !d_out_dist)) return HS_ERR_INVALID;
  hs_status st = ensure_device(h);
  if (st) return st;
  QueryCall call{d_centers, d_qcodes, d_radii ? 0.0 : R};
  if (d_radii && nq && nq < (1ull << 27)) HS_CHECK(radii_max_dev(h, d_radii, nq, &call.R));
  call.radii = nq ? d_radii : nullptr;
  uint32_t cnt = 0;
  HS_CHECK(annot_search(h, call, nq, &cnt));
  *n_out = cnt;
  const bool fits = cnt <= cap;
  HS_CHECK(annot_finish(h, cnt, fits ? d_out_id : nullptr, d_out_q, d_out_table, d_out_dist));
  return fits ? HS_OK : fail(h, HS_ERR_CAPACITY, "annotation buffers too small; see *n_out");
}

hs_status hs_annotate(hs_handle* h, const double* centers, const uint8_t* qcodes, uint64_t nq, double R,
                      const double* radii, uint32_t* out_id, uint32_t* out_q, uint32_t* out_table, double* out_dist,
                      uint64_t cap, uint64_t* n_out) {
  if (!h || !n_out) return HS_ERR_INVALID;
  *n_out = 0;
  if ((centers != nullptr) == (qcodes != nullptr))
    return fail(h, HS_ERR_INVALID, "hs_annotate: exactly one of centers and qcodes must be given");
  if (cap && (!out_id || !out_q || !out_table || !out_dist)) return HS_ERR_INVALID;
  if (nq >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nq must be < 2^27 per call");
  if (radii && !radii_max_host(radii, nq, &R)) return fail(h, HS_ERR_INVALID, "a radius is NaN");
  hs_status st = ensure_device(h);
  if (st) return st;
  QueryCall call{nullptr, nullptr, R};
  HS_CHECK(stage_queries(h, centers, qcodes, nq ? radii : nullptr, nq, &call));
  uint32_t cnt = 0;
  HS_CHECK(annot_search(h, call, nq, &cnt));
  *n_out = cnt;
  if (cnt > cap) {
    HS_CHECK(annot_finish(h, cnt, nullptr, nullptr, nullptr, nullptr));
    return fail(h, HS_ERR_CAPACITY, "annotation buffers too small; see *n_out");
  }
  // the rows are staged on the device at their own size: 16 bytes per annotated k-mer cross PCIe
  HS_HIP(h, h->io_q.reserve(std::max<size_t>(16, (size_t)cnt * 4)));
  HS_HIP(h, h->io_id.reserve(std::max<size_t>(16, (size_t)cnt * 4)));
  HS_HIP(h, h->io_table.reserve(std::max<size_t>(16, (size_t)cnt * 4)));
  HS_HIP(h, h->io_dist.reserve(std::max<size_t>(16, (size_t)cnt * 8)));
  HS_CHECK(annot_finish(h, cnt, h->io_id.as<uint32_t>(), h->io_q.as<uint32_t>(), h->io_table.as<uint32_t>(),
                        h->io_dist.as<double>()));
  if (cnt) {
    HS_HIP(h, hipMemcpyAsync(out_id, h->io_id.p, (size_t)cnt * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_q, h->io_q.p, (size_t)cnt * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_table, h->io_table.p, (size_t)cnt * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_dist, h->io_dist.p, (size_t)cnt * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return HS_OK;
}

// The merge step of the TABLE-partitioned multi-GPU layout (include/hsearch.h): in place on n gathered tuples.
hs_status hs_merge_first_table_dev(hs_handle* h, uint32_t* d_q, uint32_t* d_id, uint32_t* d_table, double* d_dist,
                                   uint64_t n, uint64_t* n_out) {
  if (!h || !n_out) return HS_ERR_INVALID;
  *n_out = 0;
  if (!n) return HS_OK;
  if (!d_q || !d_id || !d_table || !d_dist) return HS_ERR_INVALID;
  if (n >= (1ull << 31)) return fail(h, HS_ERR_INVALID, "more than 2^31 - 1 tuples to merge");
  hs_status st = ensure_device(h);
  if (st) return st;
  const uint32_t n32 = (uint32_t)n;
  HS_HIP(h, h->hit_key.reserve(n * 8));
  HS_HIP(h, h->hit_val.reserve(n * 8));
  HS_HIP(h, h->hit_key2.reserve(n * 8));
  HS_HIP(h, h->hit_val2.reserve(n * 8));
  HS_HIP(h, h->qhits.reserve(2 * (n + 1) * 4));
  HS_HIP(h, h->temp.reserve(std::max(hs_sort_pairs_u64_u64_temp(n), hs_scan_u32_temp(n + 1)) + 256));
  uint64_t *k1 = h->hit_key.as<uint64_t>(), *v1 = h->hit_val.as<uint64_t>();
  uint64_t *k2 = h->hit_key2.as<uint64_t>(), *v2 = h->hit_val2.as<uint64_t>();
  uint32_t* flag = h->qhits.as<uint32_t>();
  uint32_t* pos = flag + (n + 1);
  HS_HIP(h, hs_launch_merge_key1(d_q, d_id, d_table, d_dist, n32, k1, v1, h->stream));
  HS_HIP(h, hs_sort_pairs_u64_u64(h->temp.p, h->temp.cap, k1, k2, v1, v2, n, 64, h->stream));
  HS_HIP(h, hs_launch_merge_flag(k2, n32, flag, h->stream));
  HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, flag, pos, n + 1, h->stream));
  HS_HIP(h, hs_launch_merge_compact(k2, v2, pos, n32, k1, v1, h->stream));
  uint32_t kept = 0;
  HS_HIP(h, hipMemcpyAsync(&kept, pos + n, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (kept) {
    HS_HIP(h, hs_sort_pairs_u64_u64(h->temp.p, h->temp.cap, k1, k2, v1, v2, kept, 64, h->stream));
    HS_HIP(h, hs_launch_unpack_hits(k2, v2, kept, d_q, d_id, d_table, d_dist, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  *n_out = kept;
  return HS_OK;
}

hs_status hs_bruteforce(hs_handle* h, const double* centers, uint64_t nq, double R, uint32_t* hit_q,
                        uint32_t* hit_id, double* hit_dist, uint64_t cap, uint64_t* n_hits) {
  return host_query(h, centers, nullptr, nq, R, true, hit_q, hit_id, nullptr, hit_dist, cap, n_hits, nullptr);
}

// What every self-join entry point asks first: the index built, its own arguments in order (args_ok), the device
// ready, [first, first + count) inside the indexed k-mers
static hs_status self_join_check(hs_handle* h, uint64_t first, uint64_t count, bool args_ok) {
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  if (!args_ok) return HS_ERR_INVALID;
  HS_CHECK(ensure_device(h));
  if (first > h->n || count > h->n - first) return fail(h, HS_ERR_INVALID, "range outside the indexed k-mers");
  return HS_OK;
}

// The self-join of the k-mers [first, first + count) against the index, in chunks of whole run_query batches.  Every
// chunk's QueryCall -- its hits for `sink` -- goes to per_chunk(call, q0, nq), which runs it (run_query) and takes
// what it hands out; the chunks' profiles are added to *acc.
extern "C++" template <class PerChunk>
static hs_status self_join_chunks(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test, HitSink sink,
                                  hs_profile* acc, PerChunk per_chunk) {
  const uint64_t end = first + count;
  const uint32_t CH = 1u << 20;  // queries embedded per chunk (8k doubles each)
  for (uint64_t q0 = first; q0 < end; q0 += CH) {
    const uint64_t nq = std::min<uint64_t>(CH, end - q0);
    // from the residue codes when every filter on the way can (query_batch's self_codes); embedded
    // centres as for any other query otherwise
    const bool from_codes = self_codes_ok(h, R);
    if (!from_codes) {
      HS_HIP(h, h->io_centers.reserve((size_t)nq * h->d * 8));
      HS_HIP(h, hs_launch_embed(h->codes.as<uint8_t>() + q0 * h->p.k, nq, (int)h->p.k, h->coords.as<double>(),
                                h->io_centers.as<double>(), h->stream));
    }
    // (the pair of a k-mer with itself is dropped on the device)
    QueryCall call{from_codes ? nullptr : h->io_centers.as<double>(), nullptr, R, false, (uint32_t)q0, sqrt_test != 0};
    call.sink = sink;
    HS_CHECK(per_chunk(call, q0, nq));
    add_profile(*acc, h->prof);
  }
  return HS_OK;
}

hs_status hs_self_join(hs_handle* h, double R, int sqrt_test, uint32_t* edge_i, uint32_t* edge_j,
                       uint32_t* edge_table, double* edge_dist, uint64_t cap, uint64_t* n_edges) {
  if (!h) return HS_ERR_INVALID;
  return hs_self_join_range(h, 0, h->n, R, sqrt_test, edge_i, edge_j, edge_table, edge_dist, cap,
                            n_edges);
}

hs_status hs_self_join_range(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test,
                             uint32_t* edge_i, uint32_t* edge_j, uint32_t* edge_table,
                             double* edge_dist, uint64_t cap, uint64_t* n_edges) {
  if (!h || !n_edges) return HS_ERR_INVALID;
  *n_edges = 0;
  HS_CHECK(self_join_check(h, first, count, !cap || (edge_i && edge_j && edge_dist)));
  uint64_t total = 0;
  hs_profile acc = {};
  // the handle's I/O buffers (host-pointer queries use them the same way) and a pinned staging
  // area: Clustering() calls this once per table, reallocating 1.6 GB of centres and faulting in
  // fresh host vectors every time cost more than the join itself
  DevBuf &dq = h->io_q, &did = h->io_id, &dt = h->io_table, &dd = h->io_dist;
  const bool sj_timing = h->knobs.cluster_timing;
  auto sj_t0 = std::chrono::steady_clock::now();
  auto sj_lap = [&](const char* what) {
    if (!sj_timing) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "    sj %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - sj_t0).count());
    sj_t0 = now;
  };
  HS_CHECK(self_join_chunks(h, first, count, R, sqrt_test, HitSink(), &acc,
                            [&](const QueryCall& call, uint64_t q0, uint64_t nq) -> hs_status {
    if (call.centers) sj_lap("centers");  // (the chunk was embedded: reserve and launch)
    uint64_t hcap = std::max<uint64_t>(dq.cap / 4, 3 * nq + 1024), nh = 0;
    for (;;) {
      HS_HIP(h, dq.reserve(hcap * 4));
      HS_HIP(h, did.reserve(hcap * 4));
      HS_HIP(h, dt.reserve(hcap * 4));
      HS_HIP(h, dd.reserve(hcap * 8));
      const hs_status st = run_query(h, call, nq, dq.as<uint32_t>(), did.as<uint32_t>(), dt.as<uint32_t>(),
                                     dd.as<double>(), hcap, &nh, nullptr);
      if (st == HS_OK) break;
      if (st != HS_ERR_CAPACITY) return st;
      hcap = nh + nh / 8 + 1024;
    }
    sj_lap("run_query");
    HS_HIP(h, h->sj_host.reserve(std::max<size_t>(64, (nh + nh / 8 + 1024) * 20)));
    sj_lap("host buf");
    double* const hd = h->sj_host.as<double>();                       // [nh] doubles first: aligned
    uint32_t* const hq = reinterpret_cast<uint32_t*>(hd + nh);
    uint32_t* const hid = hq + nh;
    uint32_t* const ht = hid + nh;
    if (nh) {
      HS_HIP(h, hipMemcpyAsync(hd, dd.p, nh * 8, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipMemcpyAsync(hq, dq.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipMemcpyAsync(hid, did.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipMemcpyAsync(ht, dt.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipStreamSynchronize(h->stream));
    }
    sj_lap("d2h");
    for (uint64_t e = 0; e < nh; ++e) {
      const uint64_t i = q0 + hq[e];
      if (i == hid[e]) continue;  // a k-mer is in its own bucket at distance 0
      if (total < cap) {
        edge_i[total] = (uint32_t)i;
        edge_j[total] = hid[e];
        if (edge_table) edge_table[total] = ht[e];
        edge_dist[total] = hd[e];
      }
      ++total;
    }
    return HS_OK;
  }));
  h->prof = acc;
  h->prof.hits = total;
  *n_edges = total;
  if (total > cap) return fail(h, HS_ERR_CAPACITY, "edge buffers too small; see *n_edges");
  return HS_OK;
}

// ---- self-joins reduced on the device (hs_components, hs_degrees, hs_dbscan) ----------------------------
// The self-join of [first, first + count) with every batch's pairs reduced where finalize_hits leaves them, as
// `sink` says: no per-query ordering, no edge arrays, no copies to the host.  The chunks' profiles are added to *acc.
static hs_status reduced_self_join(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test, HitSink sink,
                                   hs_profile* acc) {
  return self_join_chunks(h, first, count, R, sqrt_test, sink, acc, [h](const QueryCall& call, uint64_t, uint64_t nq) {
    uint64_t nh = 0;
    return run_query(h, call, nq, nullptr, nullptr, nullptr, nullptr, 0, &nh, nullptr);
  });
}

// ---- hs_components: connected components of the self-join's graph (kernels and the invariant: hs_components.hip) ----
// reduced_self_join with every batch's pairs united; d_label [n] (device) receives the labels.
static hs_status components_run(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test,
                                uint32_t* d_label, uint64_t* n_components, uint64_t* n_edges) {
  if (!(R == R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  const uint32_t n_all = (uint32_t)h->n;
  HS_HIP(h, h->cc_parent.reserve(std::max<size_t>(16, (size_t)n_all * 4)));
  HS_HIP(h, h->cc_cnt.reserve(16));
  HS_HIP(h, hs_launch_cc_begin(h->cc_parent.as<uint32_t>(), n_all, h->cc_cnt.as<uint64_t>(), h->stream));
  hs_profile acc = {};
  HS_CHECK(reduced_self_join(h, first, count, R, sqrt_test, {HitSink::CC_UNION}, &acc));
  HS_HIP(h, hs_launch_cc_flatten(h->cc_parent.as<uint32_t>(), n_all, d_label, h->cc_cnt.as<uint64_t>(), h->stream));
  uint64_t counts[2] = {0, 0};
  HS_HIP(h, hipMemcpyAsync(counts, h->cc_cnt.p, 16, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->prof = acc;
  h->prof.hits = counts[0];
  *n_components = counts[1];
  if (n_edges) *n_edges = counts[0];
  return HS_OK;
}

static hs_status components_check(hs_handle* h, uint64_t first, uint64_t count, const uint32_t* label,
                                  uint64_t* n_components, uint64_t* n_edges) {
  if (!h || !n_components) return HS_ERR_INVALID;
  *n_components = 0;
  if (n_edges) *n_edges = 0;
  return self_join_check(h, first, count, !h->n || label);
}

hs_status hs_components_range_dev(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test,
                                  uint32_t* d_label, uint64_t* n_components, uint64_t* n_edges) {
  HS_CHECK(components_check(h, first, count, d_label, n_components, n_edges));
  return components_run(h, first, count, R, sqrt_test, d_label, n_components, n_edges);
}

hs_status hs_components_dev(hs_handle* h, double R, int sqrt_test, uint32_t* d_label, uint64_t* n_components,
                            uint64_t* n_edges) {
  if (!h) return HS_ERR_INVALID;
  return hs_components_range_dev(h, 0, h->n, R, sqrt_test, d_label, n_components, n_edges);
}

hs_status hs_components_range(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test, uint32_t* label,
                              uint64_t* n_components, uint64_t* n_edges) {
  HS_CHECK(components_check(h, first, count, label, n_components, n_edges));
  HS_HIP(h, h->cc_label.reserve(std::max<size_t>(16, (size_t)h->n * 4)));
  HS_CHECK(components_run(h, first, count, R, sqrt_test, h->cc_label.as<uint32_t>(), n_components, n_edges));
  if (h->n) {  // 4 bytes per k-mer cross PCIe, whatever the number of edges
    HS_HIP(h, hipMemcpyAsync(label, h->cc_label.p, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return HS_OK;
}

hs_status hs_components(hs_handle* h, double R, int sqrt_test, uint32_t* label, uint64_t* n_components,
                        uint64_t* n_edges) {
  if (!h) return HS_ERR_INVALID;
  return hs_components_range(h, 0, h->n, R, sqrt_test, label, n_components, n_edges);
}

// ---- hs_degrees / hs_dbscan: density clusters of the self-join's graph (kernels and the rule: hs_dbscan.hip) ----
// Pass 1 over [first, first + count) into db_deg and, with min_pts != 0, pass 2 and the labels into d_label (device).
// counts: {ordered pairs, clusters, core, border, noise}.  h->prof accumulates over both passes.
static hs_status dbscan_run(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test, uint32_t min_pts,
                            uint32_t* d_label, uint64_t counts[5]) {
  if (!(R == R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  const uint32_t n_all = (uint32_t)h->n;
  const size_t bytes = std::max<size_t>(16, (size_t)n_all * 4);
  HS_HIP(h, h->db_deg.reserve(bytes));
  HS_HIP(h, h->cc_parent.reserve(bytes));
  HS_HIP(h, h->db_anchor.reserve(bytes));
  HS_HIP(h, h->db_cnt.reserve(64));
  HS_HIP(h, hs_launch_db_begin(h->db_deg.as<uint32_t>(), h->cc_parent.as<uint32_t>(), h->db_anchor.as<uint32_t>(), n_all,
                               h->db_cnt.as<uint64_t>(), h->stream));
  hs_profile acc = {};
  HS_CHECK(reduced_self_join(h, first, count, R, sqrt_test, {HitSink::DB_DEGREE}, &acc));
  if (min_pts) {
    HS_CHECK(reduced_self_join(h, first, count, R, sqrt_test, {HitSink::DB_UNITE, min_pts}, &acc));
    HS_HIP(h, hs_launch_db_finish(h->cc_parent.as<uint32_t>(), h->db_deg.as<uint32_t>(), h->db_anchor.as<uint32_t>(),
                                  min_pts, n_all, d_label, h->db_cnt.as<uint64_t>(), h->stream));
  }
  HS_HIP(h, hipMemcpyAsync(counts, h->db_cnt.p, 40, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->prof = acc;
  h->prof.hits = counts[0];
  return HS_OK;
}

// the n words of db_deg / cc_label to the caller: host memory or, on the handle's stream, device memory
static hs_status dbscan_copy_out(hs_handle* h, uint32_t* dst, const DevBuf& src, bool to_device) {
  if (!h->n || !dst) return HS_OK;
  HS_HIP(h, hipMemcpyAsync(dst, src.p, (size_t)h->n * 4, to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

static hs_status degrees_any(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test, uint32_t* degree,
                             uint64_t* n_edges, bool dev) {
  if (!h) return HS_ERR_INVALID;
  if (n_edges) *n_edges = 0;
  HS_CHECK(self_join_check(h, first, count, !h->n || degree));
  uint64_t counts[5] = {0, 0, 0, 0, 0};
  HS_CHECK(dbscan_run(h, first, count, R, sqrt_test, 0, nullptr, counts));
  HS_CHECK(dbscan_copy_out(h, degree, h->db_deg, dev));
  if (n_edges) *n_edges = counts[0];
  return HS_OK;
}

static hs_status dbscan_any(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* label, uint32_t* degree,
                            hs_dbscan_counts* out, bool dev) {
  if (!h || !out) return HS_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  HS_CHECK(self_join_check(h, 0, h->n, !h->n || label));
  if (!min_pts) return fail(h, HS_ERR_INVALID, "min_pts must be at least 1");
  uint32_t* d_label = label;
  if (!dev) {
    HS_HIP(h, h->cc_label.reserve(std::max<size_t>(16, (size_t)h->n * 4)));
    d_label = h->cc_label.as<uint32_t>();
  }
  uint64_t counts[5] = {0, 0, 0, 0, 0};
  HS_CHECK(dbscan_run(h, 0, h->n, R, sqrt_test, min_pts, d_label, counts));
  if (!dev) HS_CHECK(dbscan_copy_out(h, label, h->cc_label, false));  // 4 (8 with the degrees) bytes per k-mer cross PCIe
  HS_CHECK(dbscan_copy_out(h, degree, h->db_deg, dev));
  out->n_edges = counts[0];
  out->n_clusters = counts[1];
  out->n_core = counts[2];
  out->n_border = counts[3];
  out->n_noise = counts[4];
  return HS_OK;
}

hs_status hs_degrees_range(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test, uint32_t* degree,
                           uint64_t* n_edges) {
  return degrees_any(h, first, count, R, sqrt_test, degree, n_edges, false);
}

hs_status hs_degrees_range_dev(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test,
                               uint32_t* d_degree, uint64_t* n_edges) {
  return degrees_any(h, first, count, R, sqrt_test, d_degree, n_edges, true);
}

hs_status hs_degrees(hs_handle* h, double R, int sqrt_test, uint32_t* degree, uint64_t* n_edges) {
  if (!h) return HS_ERR_INVALID;
  return degrees_any(h, 0, h->n, R, sqrt_test, degree, n_edges, false);
}

hs_status hs_degrees_dev(hs_handle* h, double R, int sqrt_test, uint32_t* d_degree, uint64_t* n_edges) {
  if (!h) return HS_ERR_INVALID;
  return degrees_any(h, 0, h->n, R, sqrt_test, d_degree, n_edges, true);
}

hs_status hs_dbscan(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* label, uint32_t* degree,
                    hs_dbscan_counts* out) {
  return dbscan_any(h, R, sqrt_test, min_pts, label, degree, out, false);
}

hs_status hs_dbscan_dev(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* d_label, uint32_t* d_degree,
                        hs_dbscan_counts* out) {
  return dbscan_any(h, R, sqrt_test, min_pts, d_label, d_degree, out, true);
}

// ---- hs_msf: the minimum spanning forest of the self-join's graph (kernels, the round and the invariant: hs_msf.hip) ----
// The entries hs_msf / hs_density_tree may keep: the option's bytes, or a quarter of what is free now.
static hs_status msf_budget(hs_handle* h, uint64_t* budget) {
  if (h->knobs.msf_edge_budget < 0) {
    size_t free_b = 0, total_b = 0;
    HS_HIP(h, hipMemGetInfo(&free_b, &total_b));
    *budget = free_b / 4 / 16;
  } else {
    *budget = (uint64_t)h->knobs.msf_edge_budget / 16;
  }
  return HS_OK;
}

// The m tree edges in msf_out_pair / msf_out_d ordered by (weight, lo, hi) -- two stable 64-bit radix sorts over all 64
// bits, by pair, then by the weight bits -- and unpacked into the three output arrays (device).
static hs_status msf_sort_unpack(hs_handle* h, uint64_t m, uint32_t* d_lo, uint32_t* d_hi, double* d_dist) {
  if (!m) return HS_OK;
  uint64_t* const op = h->msf_out_pair.as<uint64_t>();
  uint64_t* const od = h->msf_out_d.as<uint64_t>();
  uint64_t* const sp = h->msf_s_pair.as<uint64_t>();
  uint64_t* const sd = h->msf_s_d.as<uint64_t>();
  HS_HIP(h, h->temp.reserve(hs_sort_pairs_u64_u64_temp(m) + 256));
  HS_HIP(h, hs_sort_pairs_u64_u64(h->temp.p, h->temp.cap, op, sp, od, sd, m, 64, h->stream));
  HS_HIP(h, hs_sort_pairs_u64_u64(h->temp.p, h->temp.cap, sd, od, sp, op, m, 64, h->stream));
  HS_HIP(h, hs_launch_msf_unpack(op, od, (uint32_t)m, d_lo, d_hi, d_dist, h->stream));
  return HS_OK;
}

// Boruvka rounds over the pairs of the full self-join: kept in HBM by the first pass when the budget allows, from a
// reduced self-join per pass otherwise.  The m <= n - 1 tree edges, ordered by (dist, lo, hi), go to d_lo / d_hi /
// d_dist (device, room for cap), the labels to d_label (device, may be null).
static hs_status msf_run(hs_handle* h, double R, int sqrt_test, uint32_t* d_lo, uint32_t* d_hi, double* d_dist,
                         uint64_t cap, uint32_t* d_label, hs_msf_info* out) {
  if (!(R == R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  const uint32_t n = (uint32_t)h->n;
  const size_t w4 = std::max<size_t>(16, (size_t)n * 4), w8 = std::max<size_t>(16, (size_t)n * 8);
  HS_HIP(h, h->msf_comp.reserve(w4));
  HS_HIP(h, h->cc_parent.reserve(w4));
  for (DevBuf* bf : {&h->msf_best_d, &h->msf_best_pair, &h->msf_out_pair, &h->msf_out_d, &h->msf_s_pair, &h->msf_s_d})
    HS_HIP(h, bf->reserve(w8));
  HS_HIP(h, h->msf_cnt.reserve(64));
  uint32_t* const comp = h->msf_comp.as<uint32_t>();
  uint32_t* const parent = h->cc_parent.as<uint32_t>();
  uint64_t* const best_d = h->msf_best_d.as<uint64_t>();
  uint64_t* const best_pair = h->msf_best_pair.as<uint64_t>();
  uint64_t* const cnt = h->msf_cnt.as<uint64_t>();
  uint64_t budget = 0;
  HS_CHECK(msf_budget(h, &budget));
  h->msf_kept_budget = budget;
  h->msf_kept_failed = false;
  HS_HIP(h, hs_launch_msf_begin(comp, parent, best_d, best_pair, n, cnt, h->stream));
  hs_profile acc = {};
  HS_CHECK(reduced_self_join(h, 0, n, R, sqrt_test, {budget ? HitSink::MSF_COLLECT : HitSink::MSF_MIN_D}, &acc));
  uint64_t c[5] = {0, 0, 0, 0, 0};
  HS_HIP(h, hipMemcpyAsync(c, cnt, 40, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  const uint64_t n_pairs = c[0];
  const bool resident = budget && !h->msf_kept_failed && c[2] <= std::min<uint64_t>(budget, h->msf_kept.cap / 16);
  const uint64_t n_kept = resident ? c[2] : 0;
  if (!resident) h->msf_kept.release();  // (a list that overflowed is dropped; the call goes on from the self-joins)
  uint32_t rounds = 0;
  for (uint64_t cross = c[1]; cross;) {
    if (rounds == HS_MSF_MAX_ROUNDS)
      return fail(h, HS_ERR_STATE, "hs_msf: pairs still cross components after 34 rounds (internal error)");
    if (resident)
      HS_HIP(h, hs_launch_msf_min_pair_kept(h->msf_kept.p, n_kept, comp, best_d, best_pair, n, h->stream));
    else
      HS_CHECK(reduced_self_join(h, 0, n, R, sqrt_test, {HitSink::MSF_MIN_PAIR}, &acc));
    HS_HIP(h, hs_launch_msf_select(comp, parent, best_d, best_pair, n, h->msf_out_pair.as<uint64_t>(),
                                   h->msf_out_d.as<uint64_t>(), cnt, h->stream));
    ++rounds;
    HS_HIP(h, hipMemsetAsync(cnt, 0, 16, h->stream));
    if (resident)
      HS_HIP(h, hs_launch_msf_min_d_kept(h->msf_kept.p, n_kept, comp, best_d, n, cnt, h->stream));
    else
      HS_CHECK(reduced_self_join(h, 0, n, R, sqrt_test, {HitSink::MSF_MIN_D}, &acc));
    HS_HIP(h, hipMemcpyAsync(&cross, cnt + 1, 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  // the roots counted; the caller's labels are written behind the capacity verdict only
  HS_HIP(h, hs_launch_msf_finish(comp, n, nullptr, cnt, h->stream));
  HS_HIP(h, hipMemcpyAsync(c, cnt, 40, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  const uint64_t m = c[3];
  h->prof = acc;
  h->prof.hits = n_pairs;
  if (m + c[4] != n) return fail(h, HS_ERR_STATE, "hs_msf: tree edges and components do not add up (internal error)");
  out->n_tree_edges = m;
  out->n_components = c[4];
  out->n_graph_edges = n_pairs;
  out->rounds = rounds;
  out->resident = resident ? 1u : 0u;
  if (m > cap) return fail(h, HS_ERR_CAPACITY, "edge buffers too small; see out->n_tree_edges");
  if (d_label && n) HS_HIP(h, hipMemcpyAsync(d_label, comp, (size_t)n * 4, hipMemcpyDeviceToDevice, h->stream));
  HS_CHECK(msf_sort_unpack(h, m, d_lo, d_hi, d_dist));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

static hs_status msf_any(hs_handle* h, double R, int sqrt_test, uint32_t* edge_lo, uint32_t* edge_hi, double* edge_dist,
                         uint64_t cap, uint32_t* label, hs_msf_info* out, bool dev) {
  if (!h || !out) return HS_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  HS_CHECK(self_join_check(h, 0, h->n, !cap || (edge_lo && edge_hi && edge_dist)));
  if (dev) return msf_run(h, R, sqrt_test, edge_lo, edge_hi, edge_dist, cap, label, out);
  // host pointers: through the handle's I/O buffers; 16 bytes per tree edge and 4 per label cross PCIe
  const size_t room = (size_t)std::min<uint64_t>(cap, h->n);
  HS_HIP(h, h->io_q.reserve(std::max<size_t>(16, room * 4)));
  HS_HIP(h, h->io_id.reserve(std::max<size_t>(16, room * 4)));
  HS_HIP(h, h->io_dist.reserve(std::max<size_t>(16, room * 8)));
  if (label) HS_HIP(h, h->cc_label.reserve(std::max<size_t>(16, (size_t)h->n * 4)));
  HS_CHECK(msf_run(h, R, sqrt_test, h->io_q.as<uint32_t>(), h->io_id.as<uint32_t>(), h->io_dist.as<double>(), room,
                   label ? h->cc_label.as<uint32_t>() : nullptr, out));
  const size_t m = (size_t)out->n_tree_edges;
  if (m) {
    HS_HIP(h, hipMemcpyAsync(edge_lo, h->io_q.p, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(edge_hi, h->io_id.p, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(edge_dist, h->io_dist.p, m * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (label && h->n) HS_HIP(h, hipMemcpyAsync(label, h->cc_label.p, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

hs_status hs_msf(hs_handle* h, double R, int sqrt_test, uint32_t* edge_lo, uint32_t* edge_hi, double* edge_dist,
                 uint64_t cap, uint32_t* label, hs_msf_info* out) {
  return msf_any(h, R, sqrt_test, edge_lo, edge_hi, edge_dist, cap, label, out, false);
}

hs_status hs_msf_dev(hs_handle* h, double R, int sqrt_test, uint32_t* d_edge_lo, uint32_t* d_edge_hi,
                     double* d_edge_dist, uint64_t cap, uint32_t* d_label, hs_msf_info* out) {
  return msf_any(h, R, sqrt_test, d_edge_lo, d_edge_hi, d_edge_dist, cap, d_label, out, true);
}

// ---- hs_core_distance / hs_density_tree: DBSCAN* at every radius up to R (kernels, the rule and the state: hs_density.hip) ----
// The core pass: one self-join whose batches settle the core distances of their own k-mers (dt_core_batch); with
// `collect` it also keeps the pairs.  Needs msf_cnt zeroed.  c8: the eight counts afterwards.
static hs_status density_core_pass(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, bool collect,
                                   hs_profile* acc, uint64_t c8[8]) {
  const uint32_t n = (uint32_t)h->n;
  const size_t w4 = std::max<size_t>(16, (size_t)n * 4), w8 = std::max<size_t>(16, (size_t)n * 8);
  for (DevBuf* bf : {&h->dt_core, &h->dt_thr, &h->dt_next}) HS_HIP(h, bf->reserve(w8));
  HS_HIP(h, h->dt_cnt.reserve(w4));
  uint64_t* const cnt = h->msf_cnt.as<uint64_t>();
  HS_HIP(h, hs_launch_dt_begin(h->dt_core.as<uint64_t>(), h->dt_thr.as<uint64_t>(), h->dt_next.as<uint64_t>(),
                               h->dt_cnt.as<uint32_t>(), n, min_pts, h->stream));
  HS_CHECK(reduced_self_join(h, 0, n, R, sqrt_test, {collect ? HitSink::DT_CORE_COLLECT : HitSink::DT_CORE, min_pts},
                             acc));
  HS_HIP(h, hs_launch_dt_core_finish(h->dt_core.as<uint64_t>(), n, cnt, h->stream));
  HS_HIP(h, hipMemcpyAsync(c8, cnt, 64, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

static hs_status core_distance_any(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, double* core,
                                   uint64_t* n_core, uint64_t* n_edges, bool dev) {
  if (!h || !n_core) return HS_ERR_INVALID;
  *n_core = 0;
  if (n_edges) *n_edges = 0;
  HS_CHECK(self_join_check(h, 0, h->n, !h->n || core));
  if (!min_pts) return fail(h, HS_ERR_INVALID, "min_pts must be at least 1");
  if (!(R == R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  HS_HIP(h, h->msf_cnt.reserve(64));
  HS_HIP(h, hipMemsetAsync(h->msf_cnt.p, 0, 64, h->stream));
  hs_profile acc = {};
  uint64_t c8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HS_CHECK(density_core_pass(h, R, sqrt_test, min_pts, false, &acc, c8));
  h->prof = acc;
  h->prof.hits = c8[0];
  if (h->n) {
    HS_HIP(h, hipMemcpyAsync(core, h->dt_core.p, (size_t)h->n * 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                             h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  *n_core = c8[5];
  if (n_edges) *n_edges = c8[0];
  return HS_OK;
}

hs_status hs_core_distance(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, double* core, uint64_t* n_core,
                           uint64_t* n_edges) {
  return core_distance_any(h, R, sqrt_test, min_pts, core, n_core, n_edges, false);
}

hs_status hs_core_distance_dev(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, double* d_core, uint64_t* n_core,
                               uint64_t* n_edges) {
  return core_distance_any(h, R, sqrt_test, min_pts, d_core, n_core, n_edges, true);
}

// ---- hs_query_topk / hs_self_knn: the topk best hits per query (kernels, the rule and the passes: hs_knn.hip) ----

// The sink of a call whose rows go to the four device arrays; the call's hit count zeroed
static hs_status topk_begin(hs_handle* h, uint32_t topk, uint32_t* d_id, uint32_t* d_table, double* d_dist,
                            uint32_t* d_count, HitSink* sink) {
  HS_HIP(h, h->knn_total.reserve(16));
  HS_HIP(h, hipMemsetAsync(h->knn_total.p, 0, 16, h->stream));
  sink->kind = HitSink::TOPK;
  sink->topk = topk;
  sink->nn_id = d_id;
  sink->nn_table = d_table;
  sink->nn_dist = d_dist;
  sink->nn_count = d_count;
  return HS_OK;
}

static hs_status topk_total(hs_handle* h, uint64_t* total) {
  HS_HIP(h, hipMemcpyAsync(total, h->knn_total.p, 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

// The search with the selection in place of the hit list.  call: the queries on the device, with radii its R their
// largest |radius|.  Everything that can be refused from the arguments is refused before the first kernel writes.
static hs_status topk_search(hs_handle* h, QueryCall call, uint64_t nq, uint32_t topk, uint32_t* d_id, uint32_t* d_table,
                             double* d_dist, uint32_t* d_count, uint64_t* n_hits) {
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  if (nq >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nq must be < 2^27 per call");
  if (!(call.R == call.R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  HS_CHECK(topk_begin(h, topk, d_id, d_table, d_dist, d_count, &call.sink));
  // (an empty index runs no batch: nothing would write the rows)
  if (!h->n) HS_HIP(h, hs_launch_knn_fill(nq, topk, d_id, d_table, d_dist, d_count, h->stream));
  uint64_t nh = 0;
  HS_CHECK(run_query(h, call, nq, nullptr, nullptr, nullptr, nullptr, 0, &nh, nullptr));
  HS_CHECK(topk_total(h, n_hits));
  h->prof.hits = *n_hits;
  return HS_OK;
}

static hs_status topk_args(hs_handle* h, const void* centers, const void* qcodes, uint64_t nq, uint32_t topk,
                           const void* nn_id, const void* nn_dist, const void* nn_count, uint64_t* n_hits) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  if ((centers != nullptr) == (qcodes != nullptr))
    return fail(h, HS_ERR_INVALID, "hs_query_topk: exactly one of centers and qcodes must be given");
  if (!topk_ok(topk)) return fail(h, HS_ERR_INVALID, "hs_query_topk: topk must be 1 .. 64");
  if (nq && (!nn_id || !nn_dist || !nn_count)) return HS_ERR_INVALID;
  return HS_OK;
}

hs_status hs_query_topk_dev(hs_handle* h, const double* d_centers, const uint8_t* d_qcodes, uint64_t nq, double R,
                            const double* d_radii, uint32_t topk, uint32_t* d_nn_id, uint32_t* d_nn_table,
                            double* d_nn_dist, uint32_t* d_nn_count, uint64_t* n_hits) {
  HS_CHECK(topk_args(h, d_centers, d_qcodes, nq, topk, d_nn_id, d_nn_dist, d_nn_count, n_hits));
  HS_CHECK(ensure_device(h));
  QueryCall call{d_centers, d_qcodes, d_radii ? 0.0 : R};
  if (d_radii && nq && nq < (1ull << 27)) HS_CHECK(radii_max_dev(h, d_radii, nq, &call.R));
  call.radii = nq ? d_radii : nullptr;
  return topk_search(h, call, nq, topk, d_nn_id, d_nn_table, d_nn_dist, d_nn_count, n_hits);
}

// rows x topk entries and rows counts staged on the device for a host-pointer call (io_id, io_table, io_dist,
// knn_io_count), and their way out
static hs_status topk_stage_out(hs_handle* h, uint64_t rows, uint32_t topk) {
  const size_t e = (size_t)rows * topk;
  HS_HIP(h, h->io_id.reserve(std::max<size_t>(16, e * 4)));
  HS_HIP(h, h->io_table.reserve(std::max<size_t>(16, e * 4)));
  HS_HIP(h, h->io_dist.reserve(std::max<size_t>(16, e * 8)));
  HS_HIP(h, h->knn_io_count.reserve(std::max<size_t>(16, (size_t)rows * 4)));
  return HS_OK;
}

static hs_status topk_copy_out(hs_handle* h, uint64_t rows, uint32_t topk, uint32_t* nn_id, uint32_t* nn_table,
                               double* nn_dist, uint32_t* nn_count) {
  const size_t e = (size_t)rows * topk;
  if (!e) return HS_OK;
  HS_HIP(h, hipMemcpyAsync(nn_id, h->io_id.p, e * 4, hipMemcpyDeviceToHost, h->stream));
  if (nn_table) HS_HIP(h, hipMemcpyAsync(nn_table, h->io_table.p, e * 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(nn_dist, h->io_dist.p, e * 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(nn_count, h->knn_io_count.p, (size_t)rows * 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

hs_status hs_query_topk(hs_handle* h, const double* centers, const uint8_t* qcodes, uint64_t nq, double R,
                        const double* radii, uint32_t topk, uint32_t* nn_id, uint32_t* nn_table, double* nn_dist,
                        uint32_t* nn_count, uint64_t* n_hits) {
  HS_CHECK(topk_args(h, centers, qcodes, nq, topk, nn_id, nn_dist, nn_count, n_hits));
  if (nq >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nq must be < 2^27 per call");
  if (radii && !radii_max_host(radii, nq, &R)) return fail(h, HS_ERR_INVALID, "a radius is NaN");
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  if (!(R == R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  HS_CHECK(ensure_device(h));
  QueryCall call{nullptr, nullptr, R};
  HS_CHECK(stage_queries(h, centers, qcodes, nq ? radii : nullptr, nq, &call));
  HS_CHECK(topk_stage_out(h, nq, topk));
  // the rows are selected on the device: topk x 12 (16 with the tables) + 4 bytes per query cross PCIe
  HS_CHECK(topk_search(h, call, nq, topk, h->io_id.as<uint32_t>(), nn_table ? h->io_table.as<uint32_t>() : nullptr,
                       h->io_dist.as<double>(), h->knn_io_count.as<uint32_t>(), n_hits));
  return topk_copy_out(h, nq, topk, nn_id, nn_table, nn_dist, nn_count);
}

// ---- hs_seq_match: hits per (query group, sequence, diagonal) (kernels, the rule and the passes: hs_seqmatch.hip) ----
struct SeqMatchOut {
  uint32_t *group, *seq;
  int32_t* diag;
  uint32_t* count;
  double* best_dist;
  uint32_t *best_q, *best_id, *lo, *hi;
  bool all() const { return group && seq && diag && count && best_dist && best_q && best_id && lo && hi; }
};

// The whole call on device pointers.  Everything that can be refused from the arguments is refused before the first
// kernel writes: the underlying call's checks, then one small reduction over q_group / q_off / id_start and one
// read-back.  The rows go to `out` where they fit cap.
static hs_status seq_match_run(hs_handle* h, QueryCall call, uint64_t nq, SeqMatchCall sm, const SeqMatchOut& out,
                               uint64_t cap, uint64_t* n_out, uint64_t* n_hits) {
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  if (nq >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nq must be < 2^27 per call");
  if (!(call.R == call.R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  if (!sm.id_start) return fail(h, HS_ERR_INVALID, "hs_seq_match: id_start is null");
  if (!sm.q_group && sm.n_groups != nq)
    return fail(h, HS_ERR_INVALID, "hs_seq_match: without q_group n_groups must equal nq");
  if (sm.n_groups > (1ull << 32) || sm.n_seq > (1ull << 32))
    return fail(h, HS_ERR_INVALID, "hs_seq_match: more than 2^32 groups or sequences");
  uint64_t chk[3] = {0, 0, 0};
  HS_HIP(h, h->sq_chk.reserve(32));
  HS_HIP(h, hipMemsetAsync(h->sq_chk.p, 0, 32, h->stream));
  HS_HIP(h, hs_launch_sm_check(sm.q_group, sm.q_off, nq, sm.n_groups, sm.id_start, sm.n_seq, h->n,
                               h->sq_chk.as<uint64_t>(), h->stream));
  HS_HIP(h, hipMemcpyAsync(chk, h->sq_chk.p, 24, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (chk[0] & 7) return fail(h, HS_ERR_INVALID, "hs_seq_match: id_start must ascend from 0 to the index's k-mers");
  if (chk[0] & 8) return fail(h, HS_ERR_INVALID, "hs_seq_match: a q_group entry is >= n_groups");
  sm.max_qoff = chk[1];
  if (!hs_sm_widths(sm.n_groups, sm.n_seq, chk[2], sm.max_qoff, &sm.wg, &sm.ws, &sm.wd))
    return fail(h, HS_ERR_INVALID, "hs_seq_match: group, sequence and diagonal need more than 64 key bits");
  h->sq_rows = 0;
  h->sq_batches = 0;
  call.sink.kind = HitSink::SEQ_MATCH;
  call.sink.sm = &sm;
  HS_CHECK(run_query(h, call, nq, nullptr, nullptr, nullptr, nullptr, 0, n_hits, nullptr));
  const hs_profile prof = h->prof;
  const DevBuf* rows = &h->sq_acc;
  uint64_t n_rows = h->sq_rows;
  if (h->sq_batches > 1) {  // a row's hits may lie in several batches: the batches' rows reduced once more
    if (n_rows >= (1ull << 32)) return fail(h, HS_ERR_CAPACITY, "hs_seq_match: more than 2^32 - 1 rows before the merge");
    HS_HIP(h, h->sq_idx.reserve((size_t)n_rows * 4));
    HS_HIP(h, h->sq_key.reserve((size_t)n_rows * 8));
    HS_HIP(h, hipMemcpyAsync(h->sq_key.p, h->sq_acc.p, (size_t)n_rows * 8, hipMemcpyDeviceToDevice, h->stream));
    HS_HIP(h, hs_launch_sm_iota((uint32_t)n_rows, h->sq_idx.as<uint32_t>(), h->stream));
    uint32_t merged = 0;
    HS_CHECK(seq_rows_reduce(h, sm, (uint32_t)n_rows, nullptr, nullptr, nullptr, nullptr, nullptr, &h->sq_acc, &h->sq_fin,
                             0, &merged));
    rows = &h->sq_fin;
    n_rows = merged;
  }
  h->prof = prof;
  *n_out = n_rows;
  if (n_rows > cap) return fail(h, HS_ERR_CAPACITY, "row buffers too small; see *n_out");
  uint32_t flag = 0;
  HS_HIP(h, hipMemsetAsync(h->sq_chk.p, 0, 4, h->stream));
  HS_HIP(h, hs_launch_sm_decode(rows->p, rows->cap / 40, (uint32_t)n_rows, sm.ws, sm.wd, sm.max_qoff, out.group, out.seq,
                                out.diag, out.count, out.best_dist, out.best_q, out.best_id, out.lo, out.hi,
                                h->sq_chk.as<uint32_t>(), h->stream));
  HS_HIP(h, hipMemcpyAsync(&flag, h->sq_chk.p, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (flag) return fail(h, HS_ERR_CAPACITY, "hs_seq_match: a row counts more than 2^32 - 1 hits");
  return HS_OK;
}

static hs_status seq_match_args(hs_handle* h, const void* centers, const void* qcodes, const SeqMatchOut& out,
                                uint64_t cap, uint64_t* n_out, uint64_t* n_hits) {
  if (!h || !n_out || !n_hits) return HS_ERR_INVALID;
  *n_out = 0;
  *n_hits = 0;
  if ((centers != nullptr) == (qcodes != nullptr))
    return fail(h, HS_ERR_INVALID, "hs_seq_match: exactly one of centers and qcodes must be given");
  if (cap && !out.all()) return HS_ERR_INVALID;
  return HS_OK;
}

hs_status hs_seq_match_dev(hs_handle* h, const double* d_centers, const uint8_t* d_qcodes, uint64_t nq, double R,
                           const double* d_radii, const uint32_t* d_q_group, uint64_t n_groups, const uint32_t* d_q_off,
                           const uint64_t* d_id_start, uint64_t n_seq, uint32_t* d_out_group, uint32_t* d_out_seq,
                           int32_t* d_out_diag, uint32_t* d_out_count, double* d_out_best_dist, uint32_t* d_out_best_q,
                           uint32_t* d_out_best_id, uint32_t* d_out_lo, uint32_t* d_out_hi, uint64_t cap, uint64_t* n_out,
                           uint64_t* n_hits) {
  const SeqMatchOut out{d_out_group, d_out_seq, d_out_diag, d_out_count, d_out_best_dist,
                        d_out_best_q, d_out_best_id, d_out_lo, d_out_hi};
  HS_CHECK(seq_match_args(h, d_centers, d_qcodes, out, cap, n_out, n_hits));
  HS_CHECK(ensure_device(h));
  QueryCall call{d_centers, d_qcodes, d_radii ? 0.0 : R};
  if (d_radii && nq && nq < (1ull << 27)) HS_CHECK(radii_max_dev(h, d_radii, nq, &call.R));
  call.radii = nq ? d_radii : nullptr;
  SeqMatchCall sm;
  sm.q_group = d_q_group;
  sm.q_off = d_q_off;
  sm.id_start = d_id_start;
  sm.n_groups = n_groups;
  sm.n_seq = n_seq;
  return seq_match_run(h, call, nq, sm, out, cap, n_out, n_hits);
}

hs_status hs_seq_match(hs_handle* h, const double* centers, const uint8_t* qcodes, uint64_t nq, double R,
                       const double* radii, const uint32_t* q_group, uint64_t n_groups, const uint32_t* q_off,
                       const uint64_t* id_start, uint64_t n_seq, uint32_t* out_group, uint32_t* out_seq,
                       int32_t* out_diag, uint32_t* out_count, double* out_best_dist, uint32_t* out_best_q,
                       uint32_t* out_best_id, uint32_t* out_lo, uint32_t* out_hi, uint64_t cap, uint64_t* n_out,
                       uint64_t* n_hits) {
  const SeqMatchOut out{out_group, out_seq, out_diag, out_count, out_best_dist, out_best_q, out_best_id, out_lo, out_hi};
  HS_CHECK(seq_match_args(h, centers, qcodes, out, cap, n_out, n_hits));
  if (nq >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nq must be < 2^27 per call");
  if (radii && !radii_max_host(radii, nq, &R)) return fail(h, HS_ERR_INVALID, "a radius is NaN");
  if (!id_start) return fail(h, HS_ERR_INVALID, "hs_seq_match: id_start is null");
  if (n_seq > (1ull << 32)) return fail(h, HS_ERR_INVALID, "hs_seq_match: more than 2^32 groups or sequences");
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  HS_CHECK(ensure_device(h));
  QueryCall call{nullptr, nullptr, R};
  HS_CHECK(stage_queries(h, centers, qcodes, nq ? radii : nullptr, nq, &call));
  // q_group, q_off and id_start follow the queries to the device (4 + 4 bytes per query, 8 per sequence)
  const size_t gb = ((size_t)nq * 4 + 15) & ~(size_t)15, sb = ((size_t)n_seq + 1) * 8;
  HS_HIP(h, h->sq_in.reserve(sb + 2 * gb + 16));
  char* const in = h->sq_in.as<char>();
  HS_HIP(h, hipMemcpyAsync(in, id_start, sb, hipMemcpyHostToDevice, h->stream));
  if (q_group && nq) HS_HIP(h, hipMemcpyAsync(in + sb, q_group, (size_t)nq * 4, hipMemcpyHostToDevice, h->stream));
  if (q_off && nq) HS_HIP(h, hipMemcpyAsync(in + sb + gb, q_off, (size_t)nq * 4, hipMemcpyHostToDevice, h->stream));
  SeqMatchCall sm;
  sm.id_start = reinterpret_cast<const uint64_t*>(in);
  sm.q_group = q_group ? reinterpret_cast<const uint32_t*>(in + sb) : nullptr;
  sm.q_off = q_off ? reinterpret_cast<const uint32_t*>(in + sb + gb) : nullptr;
  sm.n_groups = n_groups;
  sm.n_seq = n_seq;
  // the rows are staged on the device at the caller's capacity: 40 bytes per row cross PCIe, never the hits
  HS_HIP(h, h->sq_out.reserve(std::max<size_t>(64, (size_t)cap * 40)));
  char* const o = h->sq_out.as<char>();
  uint32_t* const w = reinterpret_cast<uint32_t*>(o + cap * 8);
  const SeqMatchOut dev{w, w + cap, reinterpret_cast<int32_t*>(w + 2 * cap), w + 3 * cap, reinterpret_cast<double*>(o),
                        w + 4 * cap, w + 5 * cap, w + 6 * cap, w + 7 * cap};
  HS_CHECK(seq_match_run(h, call, nq, sm, dev, cap, n_out, n_hits));
  const size_t m = (size_t)*n_out;
  if (m) {
    HS_HIP(h, hipMemcpyAsync(out_group, dev.group, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_seq, dev.seq, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_diag, dev.diag, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_count, dev.count, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_best_dist, dev.best_dist, m * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_best_q, dev.best_q, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_best_id, dev.best_id, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_lo, dev.lo, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_hi, dev.hi, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return HS_OK;
}

// The self-join of [first, first + count) with every batch's pairs selected per k-mer: row t of the device arrays is
// k-mer first + t
static hs_status self_knn_run(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test, uint32_t topk,
                              uint32_t* d_id, uint32_t* d_table, double* d_dist, uint32_t* d_count, uint64_t* n_edges) {
  HitSink sink;
  HS_CHECK(topk_begin(h, topk, d_id, d_table, d_dist, d_count, &sink));
  hs_profile acc = {};
  HS_CHECK(self_join_chunks(h, first, count, R, sqrt_test, sink, &acc,
                            [h, first](const QueryCall& call, uint64_t q0, uint64_t nq) -> hs_status {
    QueryCall cc = call;
    cc.sink.row0 = q0 - first;  // (the chunk's query 0 is k-mer q0)
    uint64_t nh = 0;
    return run_query(h, cc, nq, nullptr, nullptr, nullptr, nullptr, 0, &nh, nullptr);
  }));
  uint64_t total = 0;
  HS_CHECK(topk_total(h, &total));
  h->prof = acc;
  h->prof.hits = total;
  if (n_edges) *n_edges = total;
  return HS_OK;
}

static hs_status self_knn_any(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test, uint32_t topk,
                              uint32_t* nn_id, uint32_t* nn_table, double* nn_dist, uint32_t* nn_count,
                              uint64_t* n_edges, bool dev) {
  if (!h) return HS_ERR_INVALID;
  if (n_edges) *n_edges = 0;
  HS_CHECK(self_join_check(h, first, count, topk_ok(topk) && (!count || (nn_id && nn_dist && nn_count))));
  if (!(R == R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  if (dev) return self_knn_run(h, first, count, R, sqrt_test, topk, nn_id, nn_table, nn_dist, nn_count, n_edges);
  HS_CHECK(topk_stage_out(h, count, topk));
  HS_CHECK(self_knn_run(h, first, count, R, sqrt_test, topk, h->io_id.as<uint32_t>(),
                        nn_table ? h->io_table.as<uint32_t>() : nullptr, h->io_dist.as<double>(),
                        h->knn_io_count.as<uint32_t>(), n_edges));
  return topk_copy_out(h, count, topk, nn_id, nn_table, nn_dist, nn_count);
}

hs_status hs_self_knn(hs_handle* h, double R, int sqrt_test, uint32_t topk, uint32_t* nn_id, uint32_t* nn_table,
                      double* nn_dist, uint32_t* nn_count, uint64_t* n_edges) {
  if (!h) return HS_ERR_INVALID;
  return self_knn_any(h, 0, h->n, R, sqrt_test, topk, nn_id, nn_table, nn_dist, nn_count, n_edges, false);
}

hs_status hs_self_knn_range(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test, uint32_t topk,
                            uint32_t* nn_id, uint32_t* nn_table, double* nn_dist, uint32_t* nn_count,
                            uint64_t* n_edges) {
  return self_knn_any(h, first, count, R, sqrt_test, topk, nn_id, nn_table, nn_dist, nn_count, n_edges, false);
}

hs_status hs_self_knn_dev(hs_handle* h, double R, int sqrt_test, uint32_t topk, uint32_t* d_nn_id, uint32_t* d_nn_table,
                          double* d_nn_dist, uint32_t* d_nn_count, uint64_t* n_edges) {
  if (!h) return HS_ERR_INVALID;
  return self_knn_any(h, 0, h->n, R, sqrt_test, topk, d_nn_id, d_nn_table, d_nn_dist, d_nn_count, n_edges, true);
}

hs_status hs_self_knn_range_dev(hs_handle* h, uint64_t first, uint64_t count, double R, int sqrt_test, uint32_t topk,
                                uint32_t* d_nn_id, uint32_t* d_nn_table, double* d_nn_dist, uint32_t* d_nn_count,
                                uint64_t* n_edges) {
  return self_knn_any(h, first, count, R, sqrt_test, topk, d_nn_id, d_nn_table, d_nn_dist, d_nn_count, n_edges, true);
}

// The core pass, then hs_msf's rounds under the mutual-reachability weight: from the kept list when the core pass could
// keep it, from two reduced self-joins per round otherwise.  The tree edges, ordered by (w, lo, hi), go to d_lo / d_hi /
// d_w (device, room for cap), the labels and core distances to d_label / d_core (device, may be null).
static hs_status density_run(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* d_lo, uint32_t* d_hi,
                             double* d_w, uint64_t cap, uint32_t* d_label, double* d_core, hs_density_info* out) {
  if (!(R == R)) return fail(h, HS_ERR_INVALID, "R is NaN");
  const uint32_t n = (uint32_t)h->n;
  const size_t w4 = std::max<size_t>(16, (size_t)n * 4), w8 = std::max<size_t>(16, (size_t)n * 8);
  HS_HIP(h, h->msf_comp.reserve(w4));
  HS_HIP(h, h->cc_parent.reserve(w4));
  for (DevBuf* bf : {&h->msf_best_d, &h->msf_best_pair, &h->msf_out_pair, &h->msf_out_d, &h->msf_s_pair, &h->msf_s_d})
    HS_HIP(h, bf->reserve(w8));
  HS_HIP(h, h->msf_cnt.reserve(64));
  uint32_t* const comp = h->msf_comp.as<uint32_t>();
  uint32_t* const parent = h->cc_parent.as<uint32_t>();
  uint64_t* const best_d = h->msf_best_d.as<uint64_t>();
  uint64_t* const best_pair = h->msf_best_pair.as<uint64_t>();
  uint64_t* const cnt = h->msf_cnt.as<uint64_t>();
  uint64_t budget = 0;
  HS_CHECK(msf_budget(h, &budget));
  h->msf_kept_budget = budget;
  h->msf_kept_failed = false;
  HS_HIP(h, hs_launch_msf_begin(comp, parent, best_d, best_pair, n, cnt, h->stream));
  hs_profile acc = {};
  uint64_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HS_CHECK(density_core_pass(h, R, sqrt_test, min_pts, budget != 0, &acc, c));
  uint32_t self_joins = 1;
  const uint64_t n_pairs = c[0], n_core = c[5];
  const bool resident = budget && !h->msf_kept_failed && c[2] <= std::min<uint64_t>(budget, h->msf_kept.cap / 16);
  const uint64_t n_kept = resident ? c[2] : 0;
  if (!resident) h->msf_kept.release();  // (a list that overflowed is dropped; the call goes on from the self-joins)
  const uint64_t* const core = h->dt_core.as<uint64_t>();
  // one pass of step 1 (into zeroed pair / cross counts) or step 2 over the pairs
  auto pass = [&](bool min_d) -> hs_status {
    if (min_d) HS_HIP(h, hipMemsetAsync(cnt, 0, 16, h->stream));
    if (resident) {
      if (min_d)
        HS_HIP(h, hs_launch_dt_min_d_kept(h->msf_kept.p, n_kept, core, comp, best_d, n, cnt, h->stream));
      else
        HS_HIP(h, hs_launch_dt_min_pair_kept(h->msf_kept.p, n_kept, core, comp, best_d, best_pair, n, h->stream));
      return HS_OK;
    }
    ++self_joins;
    return reduced_self_join(h, 0, n, R, sqrt_test, {min_d ? HitSink::DT_MIN_D : HitSink::DT_MIN_PAIR}, &acc);
  };
  uint64_t cross = 0;
  HS_CHECK(pass(true));
  HS_HIP(h, hipMemcpyAsync(&cross, cnt + 1, 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  uint32_t rounds = 0;
  while (cross) {
    if (rounds == HS_MSF_MAX_ROUNDS)
      return fail(h, HS_ERR_STATE, "hs_density_tree: pairs still cross components after 34 rounds (internal error)");
    HS_CHECK(pass(false));
    HS_HIP(h, hs_launch_msf_select(comp, parent, best_d, best_pair, n, h->msf_out_pair.as<uint64_t>(),
                                   h->msf_out_d.as<uint64_t>(), cnt, h->stream));
    ++rounds;
    HS_CHECK(pass(true));
    HS_HIP(h, hipMemcpyAsync(&cross, cnt + 1, 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  // the clusters counted; the caller's arrays are written behind the capacity verdict only
  HS_HIP(h, hs_launch_dt_finish(comp, core, n, nullptr, cnt, h->stream));
  HS_HIP(h, hipMemcpyAsync(c, cnt, 64, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  const uint64_t m = c[3];
  h->prof = acc;
  h->prof.hits = n_pairs;
  if (m + c[4] != n_core)
    return fail(h, HS_ERR_STATE, "hs_density_tree: tree edges and clusters do not add up (internal error)");
  out->n_tree_edges = m;
  out->n_clusters = c[4];
  out->n_core = n_core;
  out->n_graph_edges = n_pairs;
  out->rounds = rounds;
  out->resident = resident ? 1u : 0u;
  out->self_joins = self_joins;
  if (m > cap) return fail(h, HS_ERR_CAPACITY, "edge buffers too small; see out->n_tree_edges");
  if (d_label) HS_HIP(h, hs_launch_dt_finish(comp, core, n, d_label, nullptr, h->stream));
  if (d_core && n) HS_HIP(h, hipMemcpyAsync(d_core, core, (size_t)n * 8, hipMemcpyDeviceToDevice, h->stream));
  HS_CHECK(msf_sort_unpack(h, m, d_lo, d_hi, d_w));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

static hs_status density_any(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* edge_lo,
                             uint32_t* edge_hi, double* edge_w, uint64_t cap, uint32_t* label, double* core,
                             hs_density_info* out, bool dev) {
  if (!h || !out) return HS_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  HS_CHECK(self_join_check(h, 0, h->n, !cap || (edge_lo && edge_hi && edge_w)));
  if (!min_pts) return fail(h, HS_ERR_INVALID, "min_pts must be at least 1");
  if (dev) return density_run(h, R, sqrt_test, min_pts, edge_lo, edge_hi, edge_w, cap, label, core, out);
  // host pointers: through the handle's I/O buffers; 16 bytes per tree edge, 4 per label and 8 per core distance cross PCIe
  const size_t room = (size_t)std::min<uint64_t>(cap, h->n);
  HS_HIP(h, h->io_q.reserve(std::max<size_t>(16, room * 4)));
  HS_HIP(h, h->io_id.reserve(std::max<size_t>(16, room * 4)));
  HS_HIP(h, h->io_dist.reserve(std::max<size_t>(16, room * 8)));
  if (label) HS_HIP(h, h->cc_label.reserve(std::max<size_t>(16, (size_t)h->n * 4)));
  HS_CHECK(density_run(h, R, sqrt_test, min_pts, h->io_q.as<uint32_t>(), h->io_id.as<uint32_t>(),
                       h->io_dist.as<double>(), room, label ? h->cc_label.as<uint32_t>() : nullptr, nullptr, out));
  const size_t m = (size_t)out->n_tree_edges;
  if (m) {
    HS_HIP(h, hipMemcpyAsync(edge_lo, h->io_q.p, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(edge_hi, h->io_id.p, m * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(edge_w, h->io_dist.p, m * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (label && h->n) HS_HIP(h, hipMemcpyAsync(label, h->cc_label.p, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->stream));
  if (core && h->n) HS_HIP(h, hipMemcpyAsync(core, h->dt_core.p, (size_t)h->n * 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

hs_status hs_density_tree(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* edge_lo, uint32_t* edge_hi,
                          double* edge_w, uint64_t cap, uint32_t* label, double* core, hs_density_info* out) {
  return density_any(h, R, sqrt_test, min_pts, edge_lo, edge_hi, edge_w, cap, label, core, out, false);
}

hs_status hs_density_tree_dev(hs_handle* h, double R, int sqrt_test, uint32_t min_pts, uint32_t* d_edge_lo,
                              uint32_t* d_edge_hi, double* d_edge_w, uint64_t cap, uint32_t* d_label, double* d_core,
                              hs_density_info* out) {
  return density_any(h, R, sqrt_test, min_pts, d_edge_lo, d_edge_hi, d_edge_w, cap, d_label, d_core, out, true);
}

// ---- hs_cluster_profile / hs_cluster_radii: clusters of a label array summarised (kernels and state: hs_summary.hip) ----
// Steps 1-3: sizes and validation, rows, grouping.  d_label [n] (device).  HS_ERR_INVALID for a label that is neither
// HS_NOISE nor < n, detected on the device and reported before anything else is written.
// value_bits (hs_cluster_pssm_cover_dev; null: none): word 1 of sm_err, which the caller's own check kernel has
// written on the stream, comes back in the same read-back.
static hs_status summary_group(hs_handle* h, const uint32_t* d_label, uint32_t min_size, uint32_t* n_rows,
                               uint32_t* n_kept, uint32_t* value_bits = nullptr) {
  const uint32_t n = (uint32_t)h->n;
  const size_t words = ((size_t)n + 1) * 4;
  HS_HIP(h, h->sm_size.reserve(words));
  HS_HIP(h, h->sm_tmp.reserve(words));
  HS_HIP(h, h->sm_row_of.reserve(words));
  HS_HIP(h, h->sm_off_of.reserve(words));
  HS_HIP(h, h->sm_row_label.reserve(words));
  HS_HIP(h, h->sm_row_off.reserve(words));
  HS_HIP(h, h->sm_member.reserve(words));
  HS_HIP(h, h->sm_err.reserve(16));
  HS_HIP(h, h->temp.reserve(hs_scan_u32_temp((size_t)n + 1) + 256));
  HS_HIP(h, hs_launch_sm_group(d_label, n, min_size, h->sm_size.as<uint32_t>(), h->sm_tmp.as<uint32_t>(),
                               h->sm_row_of.as<uint32_t>(), h->sm_off_of.as<uint32_t>(), h->temp.p, h->temp.cap,
                               h->sm_err.as<uint32_t>(), h->stream));
  uint32_t back[3] = {0, 0, 0};
  HS_HIP(h, hipMemcpyAsync(&back[0], h->sm_err.p, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(&back[1], h->sm_row_of.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(&back[2], h->sm_off_of.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, h->stream));
  if (value_bits)
    HS_HIP(h, hipMemcpyAsync(value_bits, h->sm_err.as<uint32_t>() + 1, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (back[0]) return fail(h, HS_ERR_INVALID, "a label is neither HS_NOISE nor below the number of indexed k-mers");
  if (back[1] > n || back[2] > n) return fail(h, HS_ERR_HIP, "cluster summary: more rows or members than k-mers");
  HS_HIP(h, hs_launch_sm_members(d_label, n, min_size, h->sm_size.as<uint32_t>(), h->sm_row_of.as<uint32_t>(),
                                 h->sm_off_of.as<uint32_t>(), h->sm_row_label.as<uint32_t>(),
                                 h->sm_row_off.as<uint32_t>(), h->sm_member.as<uint32_t>(), h->stream));
  *n_rows = back[1];
  *n_kept = back[2];
  return HS_OK;
}

static hs_status summary_check(hs_handle* h, const uint32_t* label, uint32_t min_size) {
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  if (!min_size) return fail(h, HS_ERR_INVALID, "min_size must be at least 1");
  if (h->n && !label) return fail(h, HS_ERR_INVALID, "label is null");
  return ensure_device(h);
}

static uint32_t summary_chunk(const hs_handle* h) { return h->knobs.summary_chunk ? h->knobs.summary_chunk : 512u; }

hs_status hs_cluster_profile_dev(hs_handle* h, const uint32_t* d_label, uint32_t min_size, uint32_t* d_out_label,
                                 uint32_t* d_out_size, uint32_t* d_counts, double* d_centroid, uint64_t cap,
                                 uint64_t* n_out) {
  if (!h || !n_out) return HS_ERR_INVALID;
  *n_out = 0;
  HS_CHECK(summary_check(h, d_label, min_size));
  if (cap && (!d_out_label || !d_out_size || !d_centroid)) return fail(h, HS_ERR_INVALID, "an output array is null");
  memset(&h->prof, 0, sizeof(h->prof));
  uint32_t n_rows = 0, n_kept = 0;
  HS_CHECK(summary_group(h, d_label, min_size, &n_rows, &n_kept));
  *n_out = n_rows;
  if (n_rows > cap) return fail(h, HS_ERR_CAPACITY, "profile buffers too small; see *n_out");
  const int k = (int)h->p.k;
  const size_t cells = (size_t)k * h->alphabet;
  // rows per batch: the scratch for the counts nobody asked for holds 32 MB whatever the number of rows
  uint32_t batch = h->knobs.summary_rows;
  if (!batch) batch = (uint32_t)std::max<size_t>(1, ((size_t)32 << 20) / (cells * 4));
  if (!d_counts) HS_HIP(h, h->sm_counts.reserve(std::min<size_t>(batch, std::max<uint32_t>(n_rows, 1)) * cells * 4));
  HS_HIP(h, hs_launch_sm_head(h->sm_row_label.as<uint32_t>(), h->sm_row_off.as<uint32_t>(), n_rows, d_out_label,
                              d_out_size, h->stream));
  for (uint32_t r0 = 0; r0 < n_rows; r0 += batch) {
    const uint32_t r1 = (uint32_t)std::min<uint64_t>(n_rows, (uint64_t)r0 + batch);
    uint32_t* const cnt = d_counts ? d_counts + (size_t)r0 * cells : h->sm_counts.as<uint32_t>();
    HS_HIP(h, hs_launch_sm_profile(h->codes.as<uint8_t>(), k, h->alphabet, d_label, h->sm_row_of.as<uint32_t>(),
                                   h->sm_row_off.as<uint32_t>(), h->sm_member.as<uint32_t>(), r0, r1, summary_chunk(h),
                                   n_kept, cnt, h->n_cu, h->stream));
    HS_HIP(h, hs_launch_sm_centroid(cnt, h->coords.as<double>(), k, h->alphabet, h->sm_row_off.as<uint32_t>(), r0, r1,
                                    d_centroid, h->stream));
  }
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

hs_status hs_cluster_radii_dev(hs_handle* h, const uint32_t* d_label, uint32_t min_size, const double* d_centers,
                               uint64_t n_rows_given, double* d_max_d2, double* d_radius, uint32_t* d_medoid) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(summary_check(h, d_label, min_size));
  if (n_rows_given && (!d_centers || !d_max_d2 || !d_radius || !d_medoid))
    return fail(h, HS_ERR_INVALID, "the centres or an output array is null");
  memset(&h->prof, 0, sizeof(h->prof));
  uint32_t n_rows = 0, n_kept = 0;
  HS_CHECK(summary_group(h, d_label, min_size, &n_rows, &n_kept));
  if (n_rows != n_rows_given) return fail(h, HS_ERR_INVALID, "the labels do not give as many rows as there are centres");
  HS_HIP(h, h->sm_d2.reserve(std::max<size_t>(16, (size_t)h->n * 8)));
  HS_HIP(h, hs_launch_sm_radii(h->codes.as<uint8_t>(), (int)h->p.k, h->alphabet, h->coords.as<double>(), d_label,
                               h->sm_row_of.as<uint32_t>(), h->sm_row_off.as<uint32_t>(), h->sm_member.as<uint32_t>(),
                               n_rows, n_kept, summary_chunk(h), d_centers, h->sm_d2.as<uint64_t>(), d_max_d2, d_radius,
                               d_medoid, h->n_cu, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

// the labels of a host-pointer call on the device
static hs_status summary_labels_in(hs_handle* h, const uint32_t* label) {
  HS_HIP(h, h->sm_io_label.reserve(std::max<size_t>(16, (size_t)h->n * 4)));
  if (h->n) HS_HIP(h, hipMemcpyAsync(h->sm_io_label.p, label, (size_t)h->n * 4, hipMemcpyHostToDevice, h->stream));
  return HS_OK;
}

hs_status hs_cluster_profile(hs_handle* h, const uint32_t* label, uint32_t min_size, uint32_t* out_label,
                             uint32_t* out_size, uint32_t* counts, double* centroid, uint64_t cap, uint64_t* n_out) {
  if (!h || !n_out) return HS_ERR_INVALID;
  *n_out = 0;
  HS_CHECK(summary_check(h, label, min_size));
  if (cap && (!out_label || !out_size || !centroid)) return fail(h, HS_ERR_INVALID, "an output array is null");
  HS_CHECK(summary_labels_in(h, label));
  // the device arrays are sized by what the call can return: min(cap, n / min_size) rows
  const uint64_t room = std::min<uint64_t>(cap, h->n / min_size);
  const size_t cells = (size_t)h->p.k * h->alphabet, d = (size_t)h->d;
  HS_HIP(h, h->sm_io_a.reserve(std::max<size_t>(16, room * 4)));
  HS_HIP(h, h->sm_io_b.reserve(std::max<size_t>(16, room * 4)));
  HS_HIP(h, h->sm_io_f64.reserve(std::max<size_t>(16, room * d * 8)));
  if (counts) HS_HIP(h, h->sm_io_counts.reserve(std::max<size_t>(16, room * cells * 4)));
  uint64_t rows = 0;
  const hs_status st = hs_cluster_profile_dev(h, h->sm_io_label.as<uint32_t>(), min_size, h->sm_io_a.as<uint32_t>(),
                                              h->sm_io_b.as<uint32_t>(), counts ? h->sm_io_counts.as<uint32_t>() : nullptr,
                                              h->sm_io_f64.as<double>(), room, &rows);
  *n_out = rows;
  if (st == HS_ERR_CAPACITY && rows <= cap) return fail(h, HS_ERR_HIP, "cluster profile: more rows than n / min_size");
  HS_CHECK(st);
  if (rows) {
    HS_HIP(h, hipMemcpyAsync(out_label, h->sm_io_a.p, rows * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_size, h->sm_io_b.p, rows * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(centroid, h->sm_io_f64.p, rows * d * 8, hipMemcpyDeviceToHost, h->stream));
    if (counts) HS_HIP(h, hipMemcpyAsync(counts, h->sm_io_counts.p, rows * cells * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return HS_OK;
}

hs_status hs_cluster_radii(hs_handle* h, const uint32_t* label, uint32_t min_size, const double* centers,
                           uint64_t n_rows, double* max_d2, double* radius, uint32_t* medoid) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(summary_check(h, label, min_size));
  if (n_rows && (!centers || !max_d2 || !radius || !medoid))
    return fail(h, HS_ERR_INVALID, "the centres or an output array is null");
  if (n_rows > h->n / min_size) return fail(h, HS_ERR_INVALID, "the labels do not give as many rows as there are centres");
  HS_CHECK(summary_labels_in(h, label));
  const size_t d = (size_t)h->d;
  HS_HIP(h, h->io_centers.reserve(std::max<size_t>(16, n_rows * d * 8)));
  HS_HIP(h, h->sm_io_f64.reserve(std::max<size_t>(16, n_rows * 8)));
  HS_HIP(h, h->sm_io_f64b.reserve(std::max<size_t>(16, n_rows * 8)));
  HS_HIP(h, h->sm_io_a.reserve(std::max<size_t>(16, n_rows * 4)));
  if (n_rows) HS_HIP(h, hipMemcpyAsync(h->io_centers.p, centers, n_rows * d * 8, hipMemcpyHostToDevice, h->stream));
  HS_CHECK(hs_cluster_radii_dev(h, h->sm_io_label.as<uint32_t>(), min_size, h->io_centers.as<double>(), n_rows,
                                h->sm_io_f64.as<double>(), h->sm_io_f64b.as<double>(), h->sm_io_a.as<uint32_t>()));
  if (n_rows) {
    HS_HIP(h, hipMemcpyAsync(max_d2, h->sm_io_f64.p, n_rows * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(radius, h->sm_io_f64b.p, n_rows * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(medoid, h->sm_io_a.p, n_rows * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return HS_OK;
}

// ---- hs_cluster_weighted_profile / hs_cluster_pssm_cover: clusters to weighted, searchable profiles (kernels:
// hs_cluster_pssm.hip; the grouping and its state are hs_cluster_profile's) ----
hs_status hs_cluster_weighted_profile_dev(hs_handle* h, const uint32_t* d_label, uint32_t min_size,
                                          uint32_t* d_out_label, uint32_t* d_out_size, uint32_t* d_counts,
                                          uint64_t* d_wcounts, uint64_t* d_wsum, uint32_t* d_distinct, uint64_t cap,
                                          uint64_t* n_out) {
  if (!h || !n_out) return HS_ERR_INVALID;
  *n_out = 0;
  HS_CHECK(summary_check(h, d_label, min_size));
  if (cap && (!d_out_label || !d_out_size || !d_wcounts)) return fail(h, HS_ERR_INVALID, "an output array is null");
  memset(&h->prof, 0, sizeof(h->prof));
  uint32_t n_rows = 0, n_kept = 0;
  HS_CHECK(summary_group(h, d_label, min_size, &n_rows, &n_kept));
  *n_out = n_rows;
  if (n_rows > cap) return fail(h, HS_ERR_CAPACITY, "profile buffers too small; see *n_out");
  const int k = (int)h->p.k;
  const size_t cells = (size_t)k * h->alphabet;
  // rows per batch: the u tables (8 bytes a cell) and, when nobody asked for them, the counts (4) of a batch share the
  // 32 MB of scratch
  uint32_t batch = h->knobs.summary_rows;
  if (!batch) batch = (uint32_t)std::max<size_t>(1, ((size_t)32 << 20) / (cells * (d_counts ? 8 : 12)));
  const size_t held = std::min<size_t>(batch, std::max<uint32_t>(n_rows, 1));
  if (!d_counts) HS_HIP(h, h->sm_counts.reserve(held * cells * 4));
  HS_HIP(h, h->pw_u.reserve(hs_pssm_weights_table_bytes((uint32_t)held, k, h->alphabet)));
  HS_HIP(h, hs_launch_sm_head(h->sm_row_label.as<uint32_t>(), h->sm_row_off.as<uint32_t>(), n_rows, d_out_label,
                              d_out_size, h->stream));
  const uint32_t ch = summary_chunk(h);
  const uint32_t* const row_off = h->sm_row_off.as<uint32_t>();
  for (uint32_t r0 = 0; r0 < n_rows; r0 += batch) {
    const uint32_t r1 = (uint32_t)std::min<uint64_t>(n_rows, (uint64_t)r0 + batch);
    uint32_t* const cnt = d_counts ? d_counts + (size_t)r0 * cells : h->sm_counts.as<uint32_t>();
    HS_HIP(h, hs_launch_sm_profile(h->codes.as<uint8_t>(), k, h->alphabet, d_label, h->sm_row_of.as<uint32_t>(), row_off,
                                   h->sm_member.as<uint32_t>(), r0, r1, ch, n_kept, cnt, h->n_cu, h->stream));
    HS_HIP(h, hs_launch_pssm_weights_table(cnt, r1 - r0, k, h->alphabet, h->pw_u.as<uint64_t>(),
                                           d_distinct ? d_distinct + r0 : nullptr, h->stream));
    HS_HIP(h, hs_launch_cp_weights(h->codes.as<uint8_t>(), k, h->alphabet, d_label, h->sm_row_of.as<uint32_t>(), row_off,
                                   h->sm_member.as<uint32_t>(), r0, r1, ch, n_kept, h->pw_u.as<uint64_t>(),
                                   d_wcounts + (size_t)r0 * cells, h->n_cu, h->stream));
  }
  HS_HIP(h, hs_launch_pssm_weights_sum(d_wcounts, n_rows, k, h->alphabet, d_wsum, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->prof.summary_weight_rows = n_rows;
  if (n_rows) {  // the items of every batch: its member slots in chunks of ch (the rows' offsets are on the device)
    const uint32_t nb = (n_rows + batch - 1) / batch;
    if (nb == 1) {
      h->prof.summary_weight_items = ((uint64_t)n_kept + ch - 1) / ch;
    } else {
      std::vector<uint32_t> edge((size_t)nb + 1, n_kept);
      for (uint32_t b = 0; b < nb; ++b)
        HS_HIP(h, hipMemcpyAsync(&edge[b], row_off + (size_t)b * batch, 4, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipStreamSynchronize(h->stream));
      for (uint32_t b = 0; b < nb; ++b) h->prof.summary_weight_items += ((uint64_t)(edge[b + 1] - edge[b]) + ch - 1) / ch;
    }
  }
  return HS_OK;
}

hs_status hs_cluster_pssm_cover_dev(hs_handle* h, const uint32_t* d_label, uint32_t min_size, const double* d_S,
                                    uint64_t n_rows_given, double* d_min_score, uint32_t* d_argmin) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(summary_check(h, d_label, min_size));
  if (n_rows_given && (!d_S || !d_min_score || !d_argmin))
    return fail(h, HS_ERR_INVALID, "the profiles or an output array is null");
  if (n_rows_given > h->n / min_size)
    return fail(h, HS_ERR_INVALID, "the labels do not give as many rows as there are profiles");
  memset(&h->prof, 0, sizeof(h->prof));
  const size_t cells = (size_t)h->p.k * h->alphabet;
  // the value check of the profiles rides on the grouping's read-back: word 1 of sm_err
  HS_HIP(h, h->sm_err.reserve(16));
  HS_HIP(h, hipMemsetAsync(h->sm_err.as<uint32_t>() + 1, 0, 4, h->stream));
  if (n_rows_given)
    HS_HIP(h, hs_launch_pssm_check(d_S, n_rows_given * cells, nullptr, 0, h->sm_err.as<uint32_t>() + 1, h->stream));
  uint32_t n_rows = 0, n_kept = 0, bad = 0;
  HS_CHECK(summary_group(h, d_label, min_size, &n_rows, &n_kept, &bad));
  if (n_rows != n_rows_given) return fail(h, HS_ERR_INVALID, "the labels do not give as many rows as there are profiles");
  if (bad) return fail(h, HS_ERR_INVALID, "a profile entry is NaN, infinite or beyond 2^100");
  HS_HIP(h, h->sm_d2.reserve(std::max<size_t>(16, (size_t)h->n * 8)));
  HS_HIP(h, hs_launch_cp_cover(h->codes.as<uint8_t>(), (int)h->p.k, h->alphabet, d_S, d_label,
                               h->sm_row_of.as<uint32_t>(), h->sm_row_off.as<uint32_t>(), h->sm_member.as<uint32_t>(),
                               n_rows, n_kept, summary_chunk(h), h->sm_d2.as<uint64_t>(), d_min_score, d_argmin,
                               h->n_cu, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

hs_status hs_cluster_weighted_profile(hs_handle* h, const uint32_t* label, uint32_t min_size, uint32_t* out_label,
                                      uint32_t* out_size, uint32_t* counts, uint64_t* wcounts, uint64_t* wsum,
                                      uint32_t* distinct, uint64_t cap, uint64_t* n_out) {
  if (!h || !n_out) return HS_ERR_INVALID;
  *n_out = 0;
  HS_CHECK(summary_check(h, label, min_size));
  if (cap && (!out_label || !out_size || !wcounts)) return fail(h, HS_ERR_INVALID, "an output array is null");
  HS_CHECK(summary_labels_in(h, label));
  // the device arrays are sized by what the call can return: min(cap, n / min_size) rows; pw_out: wcounts, wsum, distinct
  const uint64_t room = std::min<uint64_t>(cap, h->n / min_size);
  const size_t cells = (size_t)h->p.k * h->alphabet;
  HS_HIP(h, h->sm_io_a.reserve(std::max<size_t>(16, room * 4)));
  HS_HIP(h, h->sm_io_b.reserve(std::max<size_t>(16, room * 4)));
  HS_HIP(h, h->pw_out.reserve(std::max<size_t>(16, room * (cells * 8 + 16))));
  if (counts) HS_HIP(h, h->sm_io_counts.reserve(std::max<size_t>(16, room * cells * 4)));
  uint64_t* const d_wc = h->pw_out.as<uint64_t>();
  uint64_t* const d_ws = d_wc + room * cells;
  uint32_t* const d_di = reinterpret_cast<uint32_t*>(d_ws + room);
  uint64_t rows = 0;
  const hs_status st = hs_cluster_weighted_profile_dev(
      h, h->sm_io_label.as<uint32_t>(), min_size, h->sm_io_a.as<uint32_t>(), h->sm_io_b.as<uint32_t>(),
      counts ? h->sm_io_counts.as<uint32_t>() : nullptr, d_wc, d_ws, d_di, room, &rows);
  *n_out = rows;
  if (st == HS_ERR_CAPACITY && rows <= cap) return fail(h, HS_ERR_HIP, "cluster profile: more rows than n / min_size");
  HS_CHECK(st);
  if (rows) {
    HS_HIP(h, hipMemcpyAsync(out_label, h->sm_io_a.p, rows * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_size, h->sm_io_b.p, rows * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(wcounts, d_wc, rows * cells * 8, hipMemcpyDeviceToHost, h->stream));
    if (wsum) HS_HIP(h, hipMemcpyAsync(wsum, d_ws, rows * 8, hipMemcpyDeviceToHost, h->stream));
    if (distinct) HS_HIP(h, hipMemcpyAsync(distinct, d_di, rows * 4, hipMemcpyDeviceToHost, h->stream));
    if (counts) HS_HIP(h, hipMemcpyAsync(counts, h->sm_io_counts.p, rows * cells * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return HS_OK;
}

hs_status hs_cluster_pssm_cover(hs_handle* h, const uint32_t* label, uint32_t min_size, const double* S, uint64_t n_rows,
                                double* min_score, uint32_t* argmin) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(summary_check(h, label, min_size));
  if (n_rows && (!S || !min_score || !argmin)) return fail(h, HS_ERR_INVALID, "the profiles or an output array is null");
  if (n_rows > h->n / min_size) return fail(h, HS_ERR_INVALID, "the labels do not give as many rows as there are profiles");
  HS_CHECK(summary_labels_in(h, label));
  const size_t cells = (size_t)h->p.k * h->alphabet;
  HS_HIP(h, h->io_centers.reserve(std::max<size_t>(16, n_rows * cells * 8)));
  HS_HIP(h, h->sm_io_f64.reserve(std::max<size_t>(16, n_rows * 8)));
  HS_HIP(h, h->sm_io_a.reserve(std::max<size_t>(16, n_rows * 4)));
  if (n_rows) HS_HIP(h, hipMemcpyAsync(h->io_centers.p, S, n_rows * cells * 8, hipMemcpyHostToDevice, h->stream));
  HS_CHECK(hs_cluster_pssm_cover_dev(h, h->sm_io_label.as<uint32_t>(), min_size, h->io_centers.as<double>(), n_rows,
                                     h->sm_io_f64.as<double>(), h->sm_io_a.as<uint32_t>()));
  if (n_rows) {
    HS_HIP(h, hipMemcpyAsync(min_score, h->sm_io_f64.p, n_rows * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(argmin, h->sm_io_a.p, n_rows * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return HS_OK;
}

hs_status hs_bruteforce_topk(hs_handle* h, const double* centers, uint64_t nq, uint32_t topk,
                             uint32_t* nn_id, double* nn_dist2) {
  if (!h || (nq && (!centers || !nn_id || !nn_dist2)) || topk < 1 || topk > 1024) return HS_ERR_INVALID;
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  hs_status st = ensure_device(h);
  if (st) return st;
  memset(&h->prof, 0, sizeof(h->prof));
  const int k = (int)h->p.k;
  const uint32_t n = (uint32_t)h->n;
  const uint32_t per_q = (n + HS_SLICE - 1) / HS_SLICE;
  const int n_blocks = h->n_cu * 8;
  HS_HIP(h, h->counters.reserve(256));
  uint32_t* d_cnt = h->counters.as<uint32_t>();
  std::vector<uint64_t> keys, vals;
  std::vector<std::pair<double, uint32_t>> cand;
  const uint32_t QB = 4096;  // queries per batch: two scans of the DB per batch
  for (uint64_t q0 = 0; q0 < nq; q0 += QB) {
    const uint32_t nqb = (uint32_t)std::min<uint64_t>(QB, nq - q0);
    for (uint32_t t = 0; t < nqb * topk; ++t) {
      nn_id[q0 * topk + t] = 0xffffffffu;
      nn_dist2[q0 * topk + t] = INFINITY;
    }
    if (!n) continue;
    HS_HIP(h, h->io_centers.reserve((size_t)nqb * h->d * 8));
    HS_HIP(h, h->tq.reserve((size_t)nqb * k * HS_TROW * 4));
    HS_HIP(h, h->io_misc.reserve((size_t)nqb * per_q * 4 + (size_t)nqb * 4));
    float* d_slice_min = h->io_misc.as<float>();
    float* d_thr = d_slice_min + (size_t)nqb * per_q;
    const double* d_centers = h->io_centers.as<double>();
    HS_HIP(h, hipMemcpyAsync(h->io_centers.p, centers + q0 * h->d, (size_t)nqb * h->d * 8,
                             hipMemcpyHostToDevice, h->stream));
    HS_HIP(h, hs_launch_qtables(d_centers, nqb, k, h->coords.as<double>(), h->alphabet,
                                h->tq.as<float>(), h->stream));
    // pass 1: minimum of every 4096-candidate slice; threshold = k-th smallest slice minimum
    HS_HIP(h, hs_launch_bruteforce(h->packed_all.as<uint4>(), n, h->tq.as<float>(), nqb, k, 0.f, d_cnt,
                                   0, nullptr, nullptr, d_slice_min, n_blocks, h->stream));
    HS_HIP(h, hs_launch_kth_min(d_slice_min, nqb, per_q, topk, d_thr, h->stream));
    // pass 2: everything under the per-query threshold, then exact fp64 distances
    uint32_t prov_cap = (uint32_t)std::max<size_t>(h->prov.cap / 8, std::max<size_t>(1u << 20, 64ull * nqb * topk));
    uint32_t n_prov = 0;
    for (;;) {
      HS_HIP(h, h->prov.reserve((size_t)prov_cap * 8));
      HS_HIP(h, hipMemsetAsync(d_cnt, 0, 8, h->stream));
      HS_HIP(h, hs_launch_bruteforce(h->packed_all.as<uint4>(), n, h->tq.as<float>(), nqb, k, 0.f,
                                     d_cnt, prov_cap, h->prov.as<uint2>(), d_thr, nullptr, n_blocks,
                                     h->stream));
      HS_HIP(h, hipMemcpyAsync(&n_prov, d_cnt, 4, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipStreamSynchronize(h->stream));
      if (n_prov <= prov_cap) break;
      prov_cap = n_prov + 1024;
    }
    HS_HIP(h, h->hit_key.reserve(std::max<size_t>(16, (size_t)n_prov * 8)));
    HS_HIP(h, h->hit_val.reserve(std::max<size_t>(16, (size_t)n_prov * 8)));
    HS_HIP(h, hs_launch_topk_exact(h->codes.as<uint8_t>(), d_centers, h->coords.as<double>(),
                                   h->prov.as<uint2>(), d_cnt, prov_cap, k, h->hit_key.as<uint64_t>(),
                                   h->hit_val.as<uint64_t>(), h->stream));
    keys.resize(n_prov);
    vals.resize(n_prov);
    if (n_prov) {
      HS_HIP(h, hipMemcpyAsync(keys.data(), h->hit_key.p, (size_t)n_prov * 8, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipMemcpyAsync(vals.data(), h->hit_val.p, (size_t)n_prov * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HS_HIP(h, hipStreamSynchronize(h->stream));
    // the per-query selection among the few survivors is host work: (d2, id) ascending
    std::vector<std::vector<std::pair<double, uint32_t>>> per(nqb);
    for (uint32_t e = 0; e < n_prov; ++e) {
      double d2;
      memcpy(&d2, &vals[e], 8);
      per[(uint32_t)(keys[e] >> 37)].push_back(std::make_pair(d2, (uint32_t)keys[e]));
    }
    for (uint32_t q = 0; q < nqb; ++q) {
      std::sort(per[q].begin(), per[q].end());
      for (uint32_t t = 0; t < topk && t < per[q].size(); ++t) {
        nn_id[(q0 + q) * topk + t] = per[q][t].second;
        nn_dist2[(q0 + q) * topk + t] = per[q][t].first;
      }
    }
    h->prof.provisional += n_prov;
    h->prof.candidates += 2ull * nqb * n;
  }
  return HS_OK;
}

}  // extern "C"
