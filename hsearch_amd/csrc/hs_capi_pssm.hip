// hs_capi_pssm.hip -- the profile calls of include/hsearch.h: position-specific score matrices (PSSMs) against every
// indexed k-mer.  The handle and filter_passes: hs_handle.h; the kernels and each call's rule: the hs_pssm*.hip named
// at its section.
//   hs_pssm_scan / _dev                  every hit (m, id, score) at the caller's thresholds        (hs_pssm.hip)
//   hs_pssm_seq_scan / _dev              the hits reduced per (profile, sequence)                   (hs_pssm_seq.hip)
//   hs_pssm_family_scan / _dev           the hits reduced per (family, sequence, diagonal)          (hs_pssm_family.hip)
//   hs_pssm_family_chain / _dev          the best gapped chain per (family, sequence)               (hs_pssm_chain.hip)
//   hs_pssm_hit_counts / _dev            the position frequency matrices of the hits                (hs_pssm_counts.hip)
//   hs_pssm_weighted_counts / _dev       ... with position-based sequence weights                   (hs_pssm_weights.hip)
//   hs_pssm_refine_weighted              the refine loop on weighted counts, under either threshold rule
//   hs_pssm_topk / _dev                  the topk best k-mers per profile, no threshold given       (hs_pssm_topk.hip)
//   hs_pssm_rank / _dev                  the threshold that admits a profile's rank best k-mers     (hs_pssm_rank.hip)
//   hs_pssm_refine, hs_pssm_refine_rank  profiles rebuilt from their own hits, iterated
//   hs_pssm_tables                       the filter's tables on the host (no GPU, no handle)
//   hs_pssm_pvalue / _dev, hs_pssm_pvalue_threshold / _dev   null-model p-values of hits and the thresholds of
//                                        p-values; hs_pssm_null_tables, hs_pssm_pvalue_host, hs_pssm_threshold_host: the
//                                        same rule on the host                                      (hs_pssm_null.hip)
//   hs_pssm_compare / _dev               profile against profile at every offset, no index needed; hs_pssm_compare_host,
//                                        _tables, _pass, _columns: the rule, the filter's tables and test, and the column
//                                        transform on the host                                      (hs_pssm_compare.hip)
// What they share, each once:
//   pssm_args_start, pssm_refuse with pssm_host_bad / pssm_rank_bad / pssm_id_start_bad / pssm_dev_check
//                     what a call refuses: from its arguments, and from its values on the host or on the device
//   pssm_stage_in     S and a per-profile array of a host-pointer call on their way up
//   pssm_batch        one batch of profiles through the tables, the FP6 MFMA filter and the exact pass
//   pssm_batch_loop   the call's profiles cut into batches by the call's rule (the fixed stride; group starts,
//                     pssm_family_cut, for hs_pssm_family_scan and hs_pssm_family_chain), a batch halved when its survivors overflow; a step before
//                     each scan and a sink after it.  pssm_call_end closes the call's profile; pssm_batches is the
//                     two together for the calls that scan at thresholds given
//   pssm_row_pass     a batch's hits reduced to (profile, sequence) rows
//   pssm_family_args, pssm_family_refuse, pssm_family_dev_check / pssm_family_host_check, pssm_family_stage
//                     the two family calls' refusals, their cut points, and a host-pointer call's arrays on their way up
//   pssm_refine       the refine loop under either threshold rule
#include <vector>

#include "hs_handle.h"
#include "hs_pssm_tables.h"
#include "hs_pssm_seq.h"
#include "hs_pssm_chain.h"
#include "hs_pssm_family.h"
#include "hs_pssm_counts.h"
#include "hs_pssm_weights.h"
#include "hs_pssm_topk.h"
#include "hs_pssm_rank.h"
#include "hs_pssm_null.h"
#include "hs_pssm_compare.h"

namespace {

// ---- what a call refuses ----------------------------------------------------------------------------------------
// how every *_args function starts; null_text: what to say when an input array is missing (null: none is)
hs_status pssm_args_start(hs_handle* h, uint64_t nm, const char* null_text) {
  if (!h->built) return fail(h, HS_ERR_STATE, "hs_index_build has not been called");
  if (nm >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nm must be < 2^27 per call");
  if (nm && null_text) return fail(h, HS_ERR_INVALID, null_text);
  return HS_OK;
}

// The values a call refuses, as bits (those of hs_pssm_check_kernel and hs_pssm_rank_check_kernel; BAD_ID_START is
// the host's own), and their texts in the order of refusal.  noun: what the per-profile array holds; name: the call.
enum { BAD_S = 1, BAD_T = 2, BAD_RANK = 4, BAD_ID_START = 8 };

hs_status pssm_refuse(hs_handle* h, uint32_t bad, const char* noun, const char* name) {
  if (bad & BAD_S) return fail(h, HS_ERR_INVALID, "a profile entry is NaN, infinite or beyond 2^100");
  if (bad & BAD_T) return fail(h, HS_ERR_INVALID, std::string("a ") + noun + " is NaN or infinite");
  if (bad & BAD_ID_START)
    return fail(h, HS_ERR_INVALID, std::string(name) + ": id_start must ascend from 0 to the index's k-mers");
  if (bad & BAD_RANK) return fail(h, HS_ERR_INVALID, "hs_pssm_rank: a rank is 0 or above the index's k-mers");
  return HS_OK;
}

// host pointers: S [nm][k][alphabet] and a per-profile array of thresholds or floors (v null: none)
uint32_t pssm_host_bad(const hs_handle* h, const double* S, const double* v, uint64_t nm) {
  const size_t ka = (size_t)h->p.k * h->alphabet;
  uint32_t bad = 0;
  for (uint64_t i = 0; i < nm * ka && !bad; ++i)
    if (hs_pssm_bad_value(S[i], HS_PSSM_MAX_ABS)) bad = BAD_S;
  for (uint64_t m = 0; v && m < nm && !bad; ++m)
    if (hs_pssm_bad_value(v[m], 1.7976931348623157e308)) bad = BAD_T;
  return bad;
}

uint32_t pssm_rank_bad(const hs_handle* h, const uint64_t* rank, uint64_t nm, uint64_t* max_rank) {
  *max_rank = 0;
  for (uint64_t m = 0; m < nm; ++m) {
    if (rank[m] < 1 || rank[m] > h->n) return BAD_RANK;
    *max_rank = std::max(*max_rank, rank[m]);
  }
  return 0;
}

uint32_t pssm_id_start_bad(const hs_handle* h, const uint64_t* id_start, uint64_t n_seq) {
  return hs_pssm_seq_id_start_ok(id_start, n_seq) && id_start[n_seq] == h->n ? 0u : (uint32_t)BAD_ID_START;
}

// Device pointers (d_v, d_rank, d_id_start null: none): one small reduction for each kind the call has, into the
// words of sq_chk -- [0..3] hs_sm_check_kernel's, [4] the BAD_* bits, [5] the largest rank -- and one read-back,
// before anything is written; then pssm_refuse.  max_rank may be null.
hs_status pssm_dev_check(hs_handle* h, const double* d_S, const double* d_v, uint64_t nm, const uint64_t* d_rank,
                         const uint64_t* d_id_start, uint64_t n_seq, const char* noun, const char* name,
                         uint64_t* max_rank) {
  uint64_t chk[6] = {0, 0, 0, 0, 0, 0};
  if (nm || d_id_start) {
    HS_HIP(h, h->sq_chk.reserve(64));
    HS_HIP(h, hipMemsetAsync(h->sq_chk.p, 0, 64, h->stream));
    uint64_t* const d_chk = h->sq_chk.as<uint64_t>();
    uint32_t* const d_bits = h->sq_chk.as<uint32_t>() + 8;
    if (nm) HS_HIP(h, hs_launch_pssm_check(d_S, nm * h->p.k * h->alphabet, d_v, d_v ? nm : 0, d_bits, h->stream));
    if (nm && d_rank) HS_HIP(h, hs_launch_pssm_rank_check(d_rank, nm, h->n, d_bits, d_chk + 5, h->stream));
    if (d_id_start) HS_HIP(h, hs_launch_sm_check(nullptr, nullptr, 0, 0, d_id_start, n_seq, h->n, d_chk, h->stream));
    HS_HIP(h, hipMemcpyAsync(chk, h->sq_chk.p, sizeof(chk), hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  if (max_rank) *max_rank = chk[5];
  return pssm_refuse(h, (uint32_t)chk[4] | (chk[0] & 7 ? (uint32_t)BAD_ID_START : 0u), noun, name);
}

// A host-pointer call's S into io_centers and its per-profile array of 8-byte words (v null: none) into vbuf
hs_status pssm_stage_in(hs_handle* h, const double* S, const void* v, uint64_t nm, DevBuf& vbuf) {
  const size_t sb = nm * h->p.k * h->alphabet * 8;
  HS_HIP(h, h->io_centers.reserve(std::max<size_t>(16, sb)));
  if (v) HS_HIP(h, vbuf.reserve(std::max<size_t>(16, nm * 8)));
  if (nm) {
    HS_HIP(h, hipMemcpyAsync(h->io_centers.p, S, sb, hipMemcpyHostToDevice, h->stream));
    if (v) HS_HIP(h, hipMemcpyAsync(vbuf.p, v, nm * 8, hipMemcpyHostToDevice, h->stream));
  }
  return HS_OK;
}

// ---- a batch, and the loop over a call's batches (kernels: hs_pssm.hip) -------------------------------------------
// One batch of mb profiles (d_S, d_t: the batch's first; number m0 of the call) against the whole index: the tables
// and the MFMA filter (or, with the filter off, nothing) and the exact pass, under filter_passes' survivor protocol.
// On success the batch's nh hits lie unordered in hit_key / hit_val.
hs_status pssm_batch(hs_handle* h, const double* d_S, const double* d_t, uint32_t m0, uint32_t mb, bool filt,
                     uint32_t* nh) {
  const int k = (int)h->p.k;
  const uint32_t steps = hs_pssm_steps(h->p.k, (uint32_t)h->alphabet), mb_pad = (mb + 15u) & ~15u;
  uint32_t* const d_cnt = h->counters.as<uint32_t>();
  enum { CNT_DEAD = 23 };  // word of the counter block hs_pssm_prep_kernel counts the dead profiles in
  if (filt) {  // the batch's tables: parameters (seg_vals), tau (tq), B tiles (c16s)
    HS_HIP(h, h->seg_vals.reserve((size_t)mb_pad * hs_pssm_prof_bytes(h->p.k)));
    HS_HIP(h, h->tq.reserve((size_t)mb_pad * 4));
    HS_HIP(h, h->c16s.reserve((size_t)(mb_pad / 16) * hs_pssm_tile_bytes(steps)));
  }
  HS_HIP(h, hipMemsetAsync(d_cnt, 0, 256, h->stream));
  HS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  HS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  HS_CHECK(filter_passes(h, mb, 0, false, nh, [&](uint32_t prov_cap, uint32_t hit_cap, bool again) -> hs_status {
    HS_HIP(h, hipEventRecord(h->ev[3], h->stream));
    if (filt) {
      if (!again)
        HS_HIP(h, hs_launch_pssm_prep(d_S, d_t, mb, h->p.k, (uint32_t)h->alphabet, h->seg_vals.p, h->tq.as<float>(),
                                      h->c16s.p, d_cnt + CNT_DEAD, h->stream));
      HS_HIP(h, hs_launch_pssm_filter(h->packed_all.as<uint4>(), (uint32_t)h->n, k, h->alphabet, h->c16s.p,
                                      h->tq.as<float>(), mb, d_cnt, prov_cap, h->prov.as<uint2>(), h->stream));
    }
    HS_HIP(h, hipEventRecord(h->ev[4], h->stream));
    HS_HIP(h, hs_launch_pssm_exact(h->codes.as<uint8_t>(), d_S, d_t, k, h->alphabet, m0, mb, (uint32_t)h->n,
                                   h->prov.as<uint2>(), d_cnt, prov_cap, !filt, hit_cap, h->hit_key.as<uint64_t>(),
                                   h->hit_val.as<uint64_t>(), h->n_cu, h->stream));
    HS_HIP(h, hipEventRecord(h->ev[5], h->stream));
    HS_HIP(h, hipMemcpyAsync(h->pin_cnt, d_cnt, HS_CNT_WORDS * 4, hipMemcpyDeviceToHost, h->stream));
    return HS_OK;
  }));
  const uint32_t dead = filt ? h->pin_cnt[CNT_DEAD] : 0u;
  h->prof.pssm_dead += dead;
  h->prof.pssm_pairs += (uint64_t)(mb - dead) * h->n;
  h->prof.pssm_survivors += filt ? (uint64_t)h->pin_cnt[0] : (uint64_t)mb * h->n;
  h->prof.pssm_mfma_steps = filt ? steps : 0;
  return HS_OK;
}

// The batch loop of every profile call: profiles 0 .. nm - 1 (nm > 0, against a non-empty index) in batches of MB, or
// of what HS_OPT_QUERY_BATCH says.  cut(m0, size) is the rule for the cut points: how many profiles the batch that
// starts at m0 takes when batches are to hold `size` (at least 1; it may exceed size where the rule cannot cut).
// one_text: the error when a batch the rule cannot cut further overflows.  Per batch of profiles m0 .. m0 + mb - 1:
//   pre(m0, mb, &d_t)  queues what must run before the scan and names the batch's thresholds (its first profile's);
//                      pre_timed: it records ev[10] / ev[11] around that, which go into ms_hash once the batch has
//                      come through (the repeated step of a batch that is halved is not counted)
//   pssm_batch         the scan; when its survivors overflow the counter the same profiles run again -- pre
//                      included -- in batches half the size, as run_query's queries do
//   sink(m0, mb, nh)   queues the work on the batch's nh unordered hits in hit_key / hit_val, ev[6] / ev[7] around it
//                      into ms_finalize; a batch without hits is skipped unless sink_empty
// *total grows by the hits.
template <class Cut, class Pre, class Sink>
hs_status pssm_batch_loop(hs_handle* h, const double* d_S, uint64_t nm, uint32_t MB, bool pre_timed, bool sink_empty,
                          uint64_t* total, Cut&& cut, const char* one_text, Pre&& pre, Sink&& sink) {
  const bool filt = !h->knobs.no_pssm_filter;
  const size_t ka = (size_t)h->p.k * h->alphabet;
  if (h->knobs.query_batch) MB = h->knobs.query_batch;
  uint32_t mb = 0;
  for (uint64_t m0 = 0; m0 < nm; m0 += mb) {
    mb = cut(m0, MB);
    const double* d_t = nullptr;
    HS_CHECK(pre((uint32_t)m0, mb, &d_t));
    uint32_t nh = 0;
    const hs_status st = pssm_batch(h, d_S + m0 * ka, d_t, (uint32_t)m0, mb, filt, &nh);
    if (st == HS_SPLIT_BATCH) {
      if (cut(m0, (mb + 1) / 2) >= mb) return fail(h, HS_ERR_CAPACITY, one_text);  // nowhere left to cut it
      MB = (mb + 1) / 2;
      mb = 0;
      continue;
    }
    if (st) return st;
    if (pre_timed) h->prof.ms_hash += ev_ms(h, 10, 11);
    if (nh || sink_empty) {
      HS_HIP(h, hipEventRecord(h->ev[6], h->stream));
      HS_CHECK(sink((uint32_t)m0, mb, nh));
      HS_HIP(h, hipEventRecord(h->ev[7], h->stream));
      HS_HIP(h, hipStreamSynchronize(h->stream));
      h->prof.ms_finalize += ev_ms(h, 6, 7);
    }
    *total += nh;
  }
  return HS_OK;
}

// ... cut anywhere: batches of MB profiles, the last one shorter (every call but hs_pssm_family_scan)
template <class Pre, class Sink>
hs_status pssm_batch_loop(hs_handle* h, const double* d_S, uint64_t nm, uint32_t MB, bool pre_timed, bool sink_empty,
                          uint64_t* total, Pre&& pre, Sink&& sink) {
  return pssm_batch_loop(
      h, d_S, nm, MB, pre_timed, sink_empty, total,
      [nm](uint64_t m0, uint32_t size) { return (uint32_t)std::min<uint64_t>(size, nm - m0); },
      "the filter survivors of one profile exceed 2^32", pre, sink);
}

// the end of a call whose start recorded ev[8]
hs_status pssm_call_end(hs_handle* h, uint64_t total) {
  HS_HIP(h, hipEventRecord(h->ev[9], h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  h->prof.ms_total = ev_ms(h, 8, 9);
  h->prof.hits = total;
  return HS_OK;
}

// A whole scan at the thresholds d_t: the loop with nothing before a scan, sink(m0, mb, nh) for every batch that has
// hits, and the call's end.  Profiles per batch: 4096 (256 tiles: 1.5 MB of B operands at 4 steps).
template <class Cut, class Sink>
hs_status pssm_batches(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm, uint64_t* n_hits, Cut&& cut,
                       const char* one_text, Sink&& sink) {
  uint64_t total = 0;
  if (nm && h->n)
    HS_CHECK(pssm_batch_loop(h, d_S, nm, 4096u, false, false, &total, cut, one_text,
                             [&](uint32_t m0, uint32_t, const double** t) -> hs_status {
                               *t = d_t + m0;
                               return HS_OK;
                             },
                             sink));
  HS_CHECK(pssm_call_end(h, total));
  *n_hits = total;
  return HS_OK;
}

template <class Sink>
hs_status pssm_batches(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm, uint64_t* n_hits, Sink&& sink) {
  return pssm_batches(
      h, d_S, d_t, nm, n_hits, [nm](uint64_t m0, uint32_t size) { return (uint32_t)std::min<uint64_t>(size, nm - m0); },
      "the filter survivors of one profile exceed 2^32", sink);
}

// the order (m, id) of a batch's nh hits: the 64-bit sort of the hit lists on the key m << 32 | id, into hit_key2 /
// hit_val2
hs_status pssm_sort_hits(hs_handle* h, uint32_t m0, uint32_t mb, uint32_t nh, size_t temp_also) {
  HS_HIP(h, h->hit_key2.reserve((size_t)nh * 8));
  HS_HIP(h, h->hit_val2.reserve((size_t)nh * 8));
  HS_HIP(h, h->temp.reserve(std::max(hs_sort_pairs_u64_u64_temp(nh), temp_also) + 256));
  HS_HIP(h, hs_sort_pairs_u64_u64(h->temp.p, h->temp.cap, h->hit_key.as<uint64_t>(), h->hit_key2.as<uint64_t>(),
                                  h->hit_val.as<uint64_t>(), h->hit_val2.as<uint64_t>(), nh,
                                  32 + bit_width_u32(m0 + mb), h->stream));
  return HS_OK;
}

// ---- hs_pssm_scan: every indexed k-mer against position-specific score matrices (kernels: hs_pssm.hip) ----
// The scan with every array on the device; the callers have checked the arguments and the values.
hs_status pssm_core(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm, uint32_t* d_hit_m,
                    uint32_t* d_hit_id, double* d_hit_score, uint64_t cap, uint64_t* n_hits, uint64_t* d_cnt_out) {
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  if (d_cnt_out && nm) HS_HIP(h, hipMemsetAsync(d_cnt_out, 0, nm * 8, h->stream));
  uint64_t total = 0;
  HS_CHECK(pssm_batches(h, d_S, d_t, nm, n_hits, [&](uint32_t m0, uint32_t mb, uint32_t nh) -> hs_status {
    const uint64_t at = std::min<uint64_t>(total, cap);
    const bool fits = nh <= cap - at;
    const uint64_t *key = h->hit_key.as<uint64_t>(), *val = h->hit_val.as<uint64_t>();
    if (fits) {
      HS_CHECK(pssm_sort_hits(h, m0, mb, nh, 0));
      key = h->hit_key2.as<uint64_t>();
      val = h->hit_val2.as<uint64_t>();
    }
    HS_HIP(h, hs_launch_pssm_emit(key, val, nh, fits, fits ? d_hit_m + at : nullptr, fits ? d_hit_id + at : nullptr,
                                  fits ? d_hit_score + at : nullptr, d_cnt_out, h->stream));
    total += nh;
    return HS_OK;
  }));
  if (*n_hits > cap) return fail(h, HS_ERR_CAPACITY, "hit buffers too small; see *n_hits");
  return HS_OK;
}

hs_status pssm_args(hs_handle* h, const void* S, const void* t, uint64_t nm, const void* hit_m, const void* hit_id,
                    const void* hit_score, uint64_t cap) {
  HS_CHECK(pssm_args_start(h, nm, S && t ? nullptr : "hs_pssm_scan: S or t is null"));
  if (cap && (!hit_m || !hit_id || !hit_score)) return fail(h, HS_ERR_INVALID, "an output array is null");
  return HS_OK;
}

// ---- hs_pssm_seq_scan: the scan's hits reduced per (profile, sequence) (kernels and the passes: hs_pssm_seq.hip) ----
struct PssmSeqOut {
  uint32_t *m = nullptr, *seq = nullptr, *count = nullptr;
  double* best_score = nullptr;
  uint32_t *best_id = nullptr, *lo = nullptr, *hi = nullptr;
  bool all() const { return m && seq && count && best_score && best_id && lo && hi; }
  PssmSeqOut at(uint64_t i) const {
    return PssmSeqOut{m + i, seq + i, count + i, best_score + i, best_id + i, lo + i, hi + i};
  }
  // r rows in 32 r bytes of one buffer: the scores, then the six 32-bit arrays
  static PssmSeqOut in(char* o, size_t r) {
    uint32_t* const w = reinterpret_cast<uint32_t*>(o + r * 8);
    return PssmSeqOut{w, w + r, w + 2 * r, reinterpret_cast<double*>(o), w + 3 * r, w + 4 * r, w + 5 * r};
  }
};

// A batch's nh hits reduced to their (profile, sequence) rows under d_id_start [n_seq + 1]; *n_rows: how many.  out
// given: they follow the `done` rows the call has so far in the caller's arrays of cap rows -- or are only counted
// when they do not fit; out null: they go to pc_rows, laid out by PssmSeqOut::in.  temp_also: bytes of temp the
// caller's next step wants; d_cnt_out, d_seq_cnt_out (either may be null): the profiles' hit and row counts; name:
// the call, for the error text.
hs_status pssm_row_pass(hs_handle* h, uint32_t m0, uint32_t mb, uint32_t nh, const uint64_t* d_id_start, uint64_t n_seq,
                        size_t temp_also, const PssmSeqOut* out, uint64_t done, uint64_t cap, uint64_t* d_cnt_out,
                        uint64_t* d_seq_cnt_out, const char* name, uint32_t* n_rows) {
  HS_CHECK(pssm_sort_hits(h, m0, mb, nh, std::max(hs_scan_u32_temp((size_t)nh + 1), temp_also)));
  const uint64_t *key = h->hit_key2.as<uint64_t>(), *val = h->hit_val2.as<uint64_t>();
  HS_HIP(h, h->sq_sidx.reserve((size_t)nh * 4));  // the sequence of every hit
  HS_HIP(h, h->sq_head.reserve(((size_t)nh + 1) * 4));
  HS_HIP(h, h->sq_excl.reserve(((size_t)nh + 1) * 4));
  HS_HIP(h, hs_launch_pssm_seq_head(key, nh, d_id_start, n_seq, h->sq_sidx.as<uint32_t>(), h->sq_head.as<uint32_t>(),
                                    h->stream));
  HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, h->sq_head.as<uint32_t>(), h->sq_excl.as<uint32_t>(),
                                  (size_t)nh + 1, h->stream));
  uint32_t rows = 0;
  HS_HIP(h, hipMemcpyAsync(&rows, h->sq_excl.as<uint32_t>() + nh, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  if (!rows || rows > nh) return fail(h, HS_ERR_HIP, std::string(name) + ": the row count of a batch is out of range");
  HS_HIP(h, h->sq_skey.reserve(((size_t)rows + 1) * 4));  // where every row's run starts
  HS_HIP(h, h->sq_key.reserve((size_t)rows * 8));         // the rows' best score keys ...
  HS_HIP(h, h->sq_idx.reserve((size_t)rows * 4));         // ... and ids
  HS_HIP(h, h->sq_part.reserve(hs_pssm_seq_part_bytes(nh)));
  bool fits = true;
  PssmSeqOut to;  // (all null when the rows do not fit)
  if (out) {
    const uint64_t at = std::min<uint64_t>(done, cap);
    fits = rows <= cap - at;
    if (fits) to = out->at(at);
  } else {
    HS_HIP(h, h->pc_rows.reserve((size_t)rows * 32));
    to = PssmSeqOut::in(h->pc_rows.as<char>(), rows);
  }
  HS_HIP(h, hs_launch_pssm_seq_rows(key, val, h->sq_sidx.as<uint32_t>(), h->sq_head.as<uint32_t>(),
                                    h->sq_excl.as<uint32_t>(), nh, rows, d_id_start, fits, h->sq_skey.as<uint32_t>(),
                                    h->sq_key.as<uint64_t>(), h->sq_idx.as<uint32_t>(), h->sq_part.p, to.m, to.seq,
                                    to.count, to.best_score, to.best_id, to.lo, to.hi, d_cnt_out, d_seq_cnt_out,
                                    h->stream));
  *n_rows = rows;
  return HS_OK;
}

// The call with every array on the device; the callers have checked the arguments and the values.  A batch's rows are
// final (every hit of a profile lies in its batch) and follow the rows of the batches before it.
hs_status pssm_seq_core(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm, const uint64_t* d_id_start,
                        uint64_t n_seq, const PssmSeqOut& out, uint64_t cap, uint64_t* n_out, uint64_t* n_hits,
                        uint64_t* d_cnt_out, uint64_t* d_seq_cnt_out) {
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  if (d_cnt_out && nm) HS_HIP(h, hipMemsetAsync(d_cnt_out, 0, nm * 8, h->stream));
  if (d_seq_cnt_out && nm) HS_HIP(h, hipMemsetAsync(d_seq_cnt_out, 0, nm * 8, h->stream));
  uint64_t total_rows = 0;
  HS_CHECK(pssm_batches(h, d_S, d_t, nm, n_hits, [&](uint32_t m0, uint32_t mb, uint32_t nh) -> hs_status {
    uint32_t rows = 0;
    HS_CHECK(pssm_row_pass(h, m0, mb, nh, d_id_start, n_seq, 0, &out, total_rows, cap, d_cnt_out, d_seq_cnt_out,
                           "hs_pssm_seq_scan", &rows));
    total_rows += rows;
    return HS_OK;
  }));
  h->prof.pssm_seq_rows = total_rows;
  *n_out = total_rows;
  if (total_rows > cap) return fail(h, HS_ERR_CAPACITY, "row buffers too small; see *n_out");
  return HS_OK;
}

// what both forms refuse from the arguments alone (hs_pssm_scan's refusals first)
hs_status pssm_seq_args(hs_handle* h, const void* S, const void* t, uint64_t nm, const void* id_start, uint64_t n_seq,
                        const PssmSeqOut& out, uint64_t cap) {
  HS_CHECK(pssm_args_start(h, nm, S && t ? nullptr : "hs_pssm_seq_scan: S or t is null"));
  if (cap && !out.all()) return fail(h, HS_ERR_INVALID, "an output array is null");
  if (!id_start) return fail(h, HS_ERR_INVALID, "hs_pssm_seq_scan: id_start is null");
  if (n_seq > (1ull << 32)) return fail(h, HS_ERR_INVALID, "hs_pssm_seq_scan: more than 2^32 sequences");
  if (!n_seq && h->n) return fail(h, HS_ERR_INVALID, "hs_pssm_seq_scan: no sequence owns the index's k-mers");
  return HS_OK;
}

// ---- hs_pssm_family_scan: the scan's hits reduced per (family, sequence, diagonal) (kernels: hs_pssm_family.hip) ----
// What the core needs beside S and t, every array on the device.  cuts: the profile numbers at which a group starts,
// ascending, and nm (null: every profile is its own group).
struct PssmFamily {
  const uint32_t* d_m_group = nullptr;
  uint64_t n_groups = 0;
  const uint32_t* d_m_off = nullptr;
  const uint64_t* d_id_start = nullptr;
  uint64_t n_seq = 0;
  uint32_t min_count = 1;
  const double* d_t_group = nullptr;
  uint64_t max_off = 0;
  int wg = 0, ws = 0, wd = 0;
  const std::vector<uint32_t>* cuts = nullptr;
};

const char* const FAMILY_NAME = "hs_pssm_family_scan";

// the group starts of a checked m_group [nm] (non-decreasing), and nm
std::vector<uint32_t> pssm_family_cuts(const uint32_t* m_group, uint64_t nm) {
  std::vector<uint32_t> cuts;
  for (uint64_t m = 0; m < nm; ++m)
    if (!m || m_group[m] != m_group[m - 1]) cuts.push_back((uint32_t)m);
  cuts.push_back((uint32_t)nm);
  return cuts;
}

// what both forms refuse from the arguments alone (hs_pssm_seq_scan's refusals first); name: the call, for the texts
hs_status pssm_family_args(hs_handle* h, const char* name, const void* S, const void* t, uint64_t nm, bool has_group,
                           uint64_t n_groups, const void* id_start, uint64_t n_seq, uint32_t min_count, bool out_all,
                           uint64_t cap) {
  const std::string at = std::string(name) + ": ";
  const std::string null_text = at + "S or t is null";
  HS_CHECK(pssm_args_start(h, nm, S && t ? nullptr : null_text.c_str()));
  if (cap && !out_all) return fail(h, HS_ERR_INVALID, "an output array is null");
  if (!id_start) return fail(h, HS_ERR_INVALID, at + "id_start is null");
  if (n_seq > (1ull << 32)) return fail(h, HS_ERR_INVALID, at + "more than 2^32 sequences");
  if (!n_seq && h->n) return fail(h, HS_ERR_INVALID, at + "no sequence owns the index's k-mers");
  if (min_count < 1) return fail(h, HS_ERR_INVALID, at + "min_count must be at least 1");
  if (n_groups > (1ull << 32)) return fail(h, HS_ERR_INVALID, at + "more than 2^32 groups");
  if (!has_group && n_groups != nm) return fail(h, HS_ERR_INVALID, at + "without m_group n_groups must equal nm");
  return HS_OK;
}

// the value errors of the family arguments (HS_FAM_BAD_* bits; HS_FAM_BAD_OFF_ORDER only where the caller passes it
// on) and the width rule, after the scan's own refusals
hs_status pssm_family_refuse(hs_handle* h, const char* name, uint32_t bad, uint64_t max_len, PssmFamily* f) {
  const std::string at = std::string(name) + ": ";
  if (bad & HS_FAM_BAD_GROUP_ORDER) return fail(h, HS_ERR_INVALID, at + "m_group must not decrease");
  if (bad & HS_FAM_BAD_GROUP_VALUE) return fail(h, HS_ERR_INVALID, at + "a group is >= n_groups");
  if (bad & HS_FAM_BAD_GROUP_SIZE) return fail(h, HS_ERR_INVALID, at + "a group holds more than 4096 profiles");
  if (bad & HS_FAM_BAD_OFF) return fail(h, HS_ERR_INVALID, at + "an m_off is above 2^31 - 1");
  if (bad & HS_FAM_BAD_T_GROUP) return fail(h, HS_ERR_INVALID, at + "a t_group entry is NaN or infinite");
  if (bad & HS_FAM_BAD_OFF_ORDER) return fail(h, HS_ERR_INVALID, at + "m_off decreases inside a group");
  if (!hs_pssm_family_widths(f->n_groups, f->n_seq, max_len, f->max_off, &f->wg, &f->ws, &f->wd))
    return fail(h, HS_ERR_INVALID, at + "group, sequence and diagonal do not fit a 64-bit key");
  return HS_OK;
}

// the batch at m0 ends at the last group start within `size`, or, where the first group is larger, at that group's end
uint32_t pssm_family_cut(const PssmFamily& f, uint64_t nm, uint64_t m0, uint32_t size) {
  if (!f.cuts) return (uint32_t)std::min<uint64_t>(size, nm - m0);
  const std::vector<uint32_t>& c = *f.cuts;
  auto it = std::upper_bound(c.begin(), c.end(), (uint32_t)std::min<uint64_t>(m0 + size, nm));
  const uint32_t end = *(it - 1);  // (c holds m0 itself, so it - 1 exists)
  return end > m0 ? end - (uint32_t)m0 : *it - (uint32_t)m0;
}

// The call with every array on the device; the callers have checked the arguments and the values.  Batches are cut at
// group starts, so a batch's rows are final and follow the rows of the batches before it.
hs_status pssm_family_core(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm, const PssmFamily& f,
                           const HsFamilyOut& out, uint64_t cap, uint64_t* n_out, uint64_t* n_hits, uint64_t* d_cnt_out,
                           uint64_t* d_grp_rows) {
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  if (d_cnt_out && nm) HS_HIP(h, hipMemsetAsync(d_cnt_out, 0, nm * 8, h->stream));
  if (d_grp_rows && f.n_groups) HS_HIP(h, hipMemsetAsync(d_grp_rows, 0, f.n_groups * 8, h->stream));
  const auto cut = [&](uint64_t m0, uint32_t size) -> uint32_t { return pssm_family_cut(f, nm, m0, size); };
  uint64_t all_rows = 0, kept_rows = 0;
  const int key_bits = std::max(1, f.wg + f.ws + f.wd);
  HS_CHECK(pssm_batches(
      h, d_S, d_t, nm, n_hits, cut, "hs_pssm_family_scan: the filter survivors of one group exceed 2^32",
      [&](uint32_t m0, uint32_t mb, uint32_t nh) -> hs_status {
        HS_CHECK(pssm_sort_hits(h, m0, mb, nh,
                                std::max(hs_scan_u32_temp((size_t)nh + 1), hs_sort_pairs_u64_u32_temp(nh))));
        const uint64_t *key = h->hit_key2.as<uint64_t>(), *val = h->hit_val2.as<uint64_t>();
        HS_HIP(h, h->sq_sidx.reserve((size_t)nh * 4));  // the sequence of every hit
        HS_HIP(h, h->sq_key.reserve((size_t)nh * 8));   // the row keys and the hit indices ...
        HS_HIP(h, h->sq_idx.reserve((size_t)nh * 4));
        HS_HIP(h, h->sq_skey.reserve((size_t)nh * 8));  // ... and their sorted copies
        HS_HIP(h, h->pf_sidx.reserve((size_t)nh * 4));
        HS_HIP(h, h->sq_head.reserve(((size_t)nh + 1) * 4));
        HS_HIP(h, h->sq_excl.reserve(((size_t)nh + 1) * 4));
        HS_HIP(h, hs_launch_pssm_seq_of(key, nh, f.d_id_start, f.n_seq, h->sq_sidx.as<uint32_t>(), h->stream));
        HS_HIP(h, hs_launch_pssm_family_key(key, h->sq_sidx.as<uint32_t>(), nh, f.d_m_group, f.d_m_off, f.d_id_start,
                                            f.ws, f.wd, f.max_off, h->sq_key.as<uint64_t>(), h->sq_idx.as<uint32_t>(),
                                            d_cnt_out, h->stream));
        HS_HIP(h, hs_sort_pairs_u64_u32(h->temp.p, h->temp.cap, h->sq_key.as<uint64_t>(), h->sq_skey.as<uint64_t>(),
                                        h->sq_idx.as<uint32_t>(), h->pf_sidx.as<uint32_t>(), nh, 0, key_bits,
                                        h->stream));
        HS_HIP(h, hs_launch_sm_head(h->sq_skey.as<uint64_t>(), nh, h->sq_head.as<uint32_t>(), h->stream));
        HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, h->sq_head.as<uint32_t>(), h->sq_excl.as<uint32_t>(),
                                        (size_t)nh + 1, h->stream));
        uint32_t rows = 0;
        HS_HIP(h, hipMemcpyAsync(&rows, h->sq_excl.as<uint32_t>() + nh, 4, hipMemcpyDeviceToHost, h->stream));
        HS_HIP(h, hipStreamSynchronize(h->stream));
        if (!rows || rows > nh)
          return fail(h, HS_ERR_HIP, std::string(FAMILY_NAME) + ": the row count of a batch is out of range");
        HS_HIP(h, h->pf_start.reserve(((size_t)rows + 1) * 4));
        HS_HIP(h, h->pf_rows.reserve((size_t)rows * 48));
        HS_HIP(h, h->pf_keep.reserve(((size_t)rows + 1) * 4));
        HS_HIP(h, h->pf_pos.reserve(((size_t)rows + 1) * 4));
        HS_HIP(h, hs_launch_pssm_family_rows(h->sq_skey.as<uint64_t>(), h->pf_sidx.as<uint32_t>(),
                                             h->sq_head.as<uint32_t>(), h->sq_excl.as<uint32_t>(), nh, rows, key, val,
                                             f.d_id_start, f.ws, f.wd, f.max_off, f.min_count, f.d_t_group,
                                             h->pf_start.as<uint32_t>(), h->pf_rows.p, h->pf_keep.as<uint32_t>(),
                                             h->stream));
        HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, h->pf_keep.as<uint32_t>(), h->pf_pos.as<uint32_t>(),
                                        (size_t)rows + 1, h->stream));
        uint32_t kept = 0;
        HS_HIP(h, hipMemcpyAsync(&kept, h->pf_pos.as<uint32_t>() + rows, 4, hipMemcpyDeviceToHost, h->stream));
        HS_HIP(h, hipStreamSynchronize(h->stream));
        if (kept > rows)
          return fail(h, HS_ERR_HIP, std::string(FAMILY_NAME) + ": the kept rows of a batch are out of range");
        const uint64_t at = std::min<uint64_t>(kept_rows, cap);
        const bool fits = kept <= cap - at;
        HS_HIP(h, hs_launch_pssm_family_write(h->pf_rows.p, h->pf_keep.as<uint32_t>(), h->pf_pos.as<uint32_t>(), rows,
                                              fits && kept, fits && kept ? out.at(at) : HsFamilyOut(), d_grp_rows,
                                              h->stream));
        all_rows += rows;
        kept_rows += kept;
        return HS_OK;
      }));
  h->prof.pssm_fam_rows = all_rows;
  h->prof.pssm_fam_kept = kept_rows;
  *n_out = kept_rows;
  if (kept_rows > cap) return fail(h, HS_ERR_CAPACITY, "row buffers too small; see *n_out");
  return HS_OK;
}

// ---- hs_pssm_family_chain: the best gapped chain per (family, sequence) (kernels: hs_pssm_chain.hip) ----------------
struct PssmChain {
  uint32_t max_shift = 0;
  double gap_open = 0.0, gap_ext = 0.0;
};

const char* const CHAIN_NAME = "hs_pssm_family_chain";

// what both forms refuse beside the family scan's argument refusals
hs_status pssm_chain_args(hs_handle* h, const void* m_off, const PssmChain& c) {
  if (!m_off) return fail(h, HS_ERR_INVALID, "hs_pssm_family_chain: m_off is null");
  if (c.max_shift > HS_PSSM_CHAIN_MAX_SHIFT) return fail(h, HS_ERR_INVALID, "hs_pssm_family_chain: max_shift is above 65535");
  if (!hs_pssm_chain_params_ok(c.max_shift, c.gap_open, c.gap_ext))
    return fail(h, HS_ERR_INVALID, "hs_pssm_family_chain: gap_open and gap_ext must be finite and not negative");
  return HS_OK;
}

// The call with every array on the device; the callers have checked the arguments and the values.  Batches are cut at
// group starts, so a batch's segments are final and their rows follow the rows of the batches before it.
hs_status pssm_chain_core(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm, const PssmFamily& f,
                          const PssmChain& c, const HsChainOut& out, uint64_t cap, uint64_t* n_out, uint64_t* n_hits,
                          uint64_t* d_cnt_out, uint64_t* d_grp_rows) {
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  if (d_cnt_out && nm) HS_HIP(h, hipMemsetAsync(d_cnt_out, 0, nm * 8, h->stream));
  if (d_grp_rows && f.n_groups) HS_HIP(h, hipMemsetAsync(d_grp_rows, 0, f.n_groups * 8, h->stream));
  const auto cut = [&](uint64_t m0, uint32_t size) -> uint32_t { return pssm_family_cut(f, nm, m0, size); };
  uint64_t all_segs = 0, kept_rows = 0;
  const int key_bits = std::max(1, f.wg + f.ws);
  HS_CHECK(pssm_batches(
      h, d_S, d_t, nm, n_hits, cut, "hs_pssm_family_chain: the filter survivors of one group exceed 2^32",
      [&](uint32_t m0, uint32_t mb, uint32_t nh) -> hs_status {
        HS_CHECK(pssm_sort_hits(h, m0, mb, nh,
                                std::max(hs_scan_u32_temp((size_t)nh + 1), hs_sort_pairs_u64_u32_temp(nh))));
        const uint64_t *key = h->hit_key2.as<uint64_t>(), *val = h->hit_val2.as<uint64_t>();
        HS_HIP(h, h->sq_sidx.reserve((size_t)nh * 4));  // the sequence of every hit
        HS_HIP(h, h->sq_key.reserve((size_t)nh * 8));   // the segment keys and the hit indices ...
        HS_HIP(h, h->sq_idx.reserve((size_t)nh * 4));
        HS_HIP(h, h->sq_skey.reserve((size_t)nh * 8));  // ... and their sorted copies
        HS_HIP(h, h->pf_sidx.reserve((size_t)nh * 4));
        HS_HIP(h, h->sq_head.reserve(((size_t)nh + 1) * 4));
        HS_HIP(h, h->sq_excl.reserve(((size_t)nh + 1) * 4));
        HS_HIP(h, hs_launch_pssm_seq_of(key, nh, f.d_id_start, f.n_seq, h->sq_sidx.as<uint32_t>(), h->stream));
        // the family's key kernel without a diagonal field: g << ws | s
        HS_HIP(h, hs_launch_pssm_family_key(key, h->sq_sidx.as<uint32_t>(), nh, f.d_m_group, nullptr, f.d_id_start, f.ws,
                                            0, 0, h->sq_key.as<uint64_t>(), h->sq_idx.as<uint32_t>(), d_cnt_out,
                                            h->stream));
        HS_HIP(h, hs_sort_pairs_u64_u32(h->temp.p, h->temp.cap, h->sq_key.as<uint64_t>(), h->sq_skey.as<uint64_t>(),
                                        h->sq_idx.as<uint32_t>(), h->pf_sidx.as<uint32_t>(), nh, 0, key_bits,
                                        h->stream));
        HS_HIP(h, hs_launch_sm_head(h->sq_skey.as<uint64_t>(), nh, h->sq_head.as<uint32_t>(), h->stream));
        HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, h->sq_head.as<uint32_t>(), h->sq_excl.as<uint32_t>(),
                                        (size_t)nh + 1, h->stream));
        uint32_t segs = 0;
        HS_HIP(h, hipMemcpyAsync(&segs, h->sq_excl.as<uint32_t>() + nh, 4, hipMemcpyDeviceToHost, h->stream));
        HS_HIP(h, hipStreamSynchronize(h->stream));
        if (!segs || segs > nh)
          return fail(h, HS_ERR_HIP, std::string(CHAIN_NAME) + ": the segment count of a batch is out of range");
        HS_HIP(h, h->pf_start.reserve(((size_t)segs + 1) * 4));
        HS_HIP(h, h->pch_state.reserve(hs_pssm_chain_state_bytes(nh)));
        HS_HIP(h, h->pch_rows.reserve((size_t)segs * 44));
        HS_HIP(h, h->pf_keep.reserve(((size_t)segs + 1) * 4));
        HS_HIP(h, h->pf_pos.reserve(((size_t)segs + 1) * 4));
        HS_HIP(h, hs_launch_pssm_chain(h->sq_skey.as<uint64_t>(), h->pf_sidx.as<uint32_t>(), h->sq_head.as<uint32_t>(),
                                       h->sq_excl.as<uint32_t>(), nh, segs, key, val, f.d_id_start, f.d_m_off, f.ws,
                                       c.max_shift, c.gap_open, c.gap_ext, f.min_count, f.d_t_group,
                                       h->pf_start.as<uint32_t>(), h->pch_state.p, h->pch_rows.p,
                                       h->pf_keep.as<uint32_t>(), h->stream));
        HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, h->pf_keep.as<uint32_t>(), h->pf_pos.as<uint32_t>(),
                                        (size_t)segs + 1, h->stream));
        uint32_t kept = 0;
        HS_HIP(h, hipMemcpyAsync(&kept, h->pf_pos.as<uint32_t>() + segs, 4, hipMemcpyDeviceToHost, h->stream));
        HS_HIP(h, hipStreamSynchronize(h->stream));
        if (kept > segs)
          return fail(h, HS_ERR_HIP, std::string(CHAIN_NAME) + ": the kept rows of a batch are out of range");
        const uint64_t at = std::min<uint64_t>(kept_rows, cap);
        const bool fits = kept <= cap - at;
        HS_HIP(h, hs_launch_pssm_chain_write(h->pch_rows.p, h->pf_keep.as<uint32_t>(), h->pf_pos.as<uint32_t>(), segs,
                                             fits && kept, fits && kept ? out.at(at) : HsChainOut(), d_grp_rows,
                                             h->stream));
        all_segs += segs;
        kept_rows += kept;
        return HS_OK;
      }));
  h->prof.pssm_chain_segs = all_segs;
  h->prof.pssm_chain_kept = kept_rows;
  *n_out = kept_rows;
  if (kept_rows > cap) return fail(h, HS_ERR_CAPACITY, "row buffers too small; see *n_out");
  return HS_OK;
}

// The value errors of a family call's device arrays (the argument refusals are behind it): the words of sq_chk --
// [0..2] hs_sm_check_kernel's {flags, largest m_off, most ids of a sequence}, [4] the BAD_* bits of S and t, [6] the
// HS_FAM_BAD_* bits, of which the call refuses those in `refused` -- and, in the same read-back, m_group for the cut
// points.  f and cuts are filled.
hs_status pssm_family_dev_check(hs_handle* h, const char* name, const double* d_S, const double* d_t, uint64_t nm,
                                const uint32_t* d_m_group, uint64_t n_groups, const uint32_t* d_m_off,
                                const uint64_t* d_id_start, uint64_t n_seq, uint32_t min_count, const double* d_t_group,
                                uint32_t refused, PssmFamily* f, std::vector<uint32_t>* cuts) {
  HS_CHECK(ensure_device(h));
  uint64_t chk[7] = {0, 0, 0, 0, 0, 0, 0};
  std::vector<uint32_t> groups;
  HS_HIP(h, h->sq_chk.reserve(64));
  HS_HIP(h, hipMemsetAsync(h->sq_chk.p, 0, 64, h->stream));
  if (nm) HS_HIP(h, hs_launch_pssm_check(d_S, nm * h->p.k * h->alphabet, d_t, nm, h->sq_chk.as<uint32_t>() + 8, h->stream));
  HS_HIP(h, hs_launch_sm_check(d_m_group, d_m_off, nm, n_groups, d_id_start, n_seq, h->n, h->sq_chk.as<uint64_t>(),
                               h->stream));
  HS_HIP(h, hs_launch_pssm_family_check(d_m_group, d_m_off, d_t_group, nm, n_groups, h->sq_chk.as<uint32_t>() + 12,
                                        h->stream));
  HS_HIP(h, hipMemcpyAsync(chk, h->sq_chk.p, sizeof(chk), hipMemcpyDeviceToHost, h->stream));
  if (d_m_group && nm) {
    try {
      groups.resize(nm);
    } catch (const std::bad_alloc&) {
      return fail(h, HS_ERR_NOMEM, std::string(name) + ": no memory for the groups");
    }
    HS_HIP(h, hipMemcpyAsync(groups.data(), d_m_group, nm * 4, hipMemcpyDeviceToHost, h->stream));
  }
  HS_HIP(h, hipStreamSynchronize(h->stream));
  HS_CHECK(pssm_refuse(h, (uint32_t)chk[4] | (chk[0] & 7 ? (uint32_t)BAD_ID_START : 0u), "threshold", name));
  f->d_m_group = d_m_group;
  f->n_groups = n_groups;
  f->d_m_off = d_m_off;
  f->d_id_start = d_id_start;
  f->n_seq = n_seq;
  f->min_count = min_count;
  f->d_t_group = d_t_group;
  f->max_off = d_m_off ? chk[1] : 0;
  HS_CHECK(pssm_family_refuse(
      h, name, ((uint32_t)chk[6] & refused) | (chk[0] & 8 ? (uint32_t)HS_FAM_BAD_GROUP_VALUE : 0u), chk[2], f));
  if (d_m_group) {
    try {
      *cuts = pssm_family_cuts(groups.data(), nm);
    } catch (const std::bad_alloc&) {
      return fail(h, HS_ERR_NOMEM, std::string(name) + ": no memory for the groups");
    }
    f->cuts = cuts;
  }
  return HS_OK;
}

// ... and of a call's host arrays
hs_status pssm_family_host_check(hs_handle* h, const char* name, const double* S, const double* t, uint64_t nm,
                                 const uint32_t* m_group, uint64_t n_groups, const uint32_t* m_off,
                                 const uint64_t* id_start, uint64_t n_seq, uint32_t min_count, const double* t_group,
                                 uint32_t refused, PssmFamily* f, std::vector<uint32_t>* cuts) {
  HS_CHECK(pssm_refuse(h, pssm_host_bad(h, S, t, nm) | pssm_id_start_bad(h, id_start, n_seq), "threshold", name));
  f->n_groups = n_groups;
  f->n_seq = n_seq;
  f->min_count = min_count;
  uint64_t max_len = 0;
  for (uint64_t s = 0; s < n_seq; ++s) max_len = std::max(max_len, id_start[s + 1] - id_start[s]);
  HS_CHECK(pssm_family_refuse(
      h, name, hs_pssm_family_values_bad(nm, m_group, n_groups, m_off, t_group, &f->max_off) & refused, max_len, f));
  if (m_group) {
    try {
      *cuts = pssm_family_cuts(m_group, nm);
    } catch (const std::bad_alloc&) {
      return fail(h, HS_ERR_NOMEM, std::string(name) + ": no memory for the groups");
    }
    f->cuts = cuts;
  }
  return HS_OK;
}

// A host-pointer family call's arrays on their way up: S and t (io_centers, io_radii), id_start (sq_in), m_group,
// m_off, t_group (pf_in), room for out_bytes of rows (sq_out) and, where the caller wants them, for cnt and grp_rows
// (io_cand).  f receives the device pointers.  (The per-group arrays only where the caller has them: n_groups may be
// 2^32 with neither.)
hs_status pssm_family_stage(hs_handle* h, const double* S, const double* t, uint64_t nm, const uint32_t* m_group,
                            uint64_t n_groups, const uint32_t* m_off, const uint64_t* id_start, uint64_t n_seq,
                            const double* t_group, bool want_cnt, bool want_grp, size_t out_bytes, PssmFamily* f,
                            uint64_t** d_cnt, uint64_t** d_grp) {
  HS_CHECK(ensure_device(h));
  const size_t sb = ((size_t)n_seq + 1) * 8, cb = std::max<size_t>(16, nm * 8);
  const size_t tb = t_group ? std::max<size_t>(16, n_groups * 8) : 16, gb = want_grp ? std::max<size_t>(16, n_groups * 8) : 16;
  const size_t mb4 = (std::max<size_t>(16, nm * 4) + 15) & ~(size_t)15;
  HS_CHECK(pssm_stage_in(h, S, t, nm, h->io_radii));
  HS_HIP(h, h->sq_in.reserve(sb));
  HS_HIP(h, h->pf_in.reserve(2 * mb4 + tb));  // m_group, m_off, t_group
  HS_HIP(h, h->sq_out.reserve(std::max<size_t>(64, out_bytes)));
  if (want_cnt || want_grp) HS_HIP(h, h->io_cand.reserve(cb + gb));
  HS_HIP(h, hipMemcpyAsync(h->sq_in.p, id_start, sb, hipMemcpyHostToDevice, h->stream));
  char* const in = h->pf_in.as<char>();
  if (m_group && nm) HS_HIP(h, hipMemcpyAsync(in, m_group, nm * 4, hipMemcpyHostToDevice, h->stream));
  if (m_off && nm) HS_HIP(h, hipMemcpyAsync(in + mb4, m_off, nm * 4, hipMemcpyHostToDevice, h->stream));
  if (t_group && n_groups)
    HS_HIP(h, hipMemcpyAsync(in + 2 * mb4, t_group, n_groups * 8, hipMemcpyHostToDevice, h->stream));
  f->d_m_group = m_group ? reinterpret_cast<const uint32_t*>(in) : nullptr;
  f->d_m_off = m_off ? reinterpret_cast<const uint32_t*>(in + mb4) : nullptr;
  f->d_t_group = t_group ? reinterpret_cast<const double*>(in + 2 * mb4) : nullptr;
  f->d_id_start = h->sq_in.as<uint64_t>();
  *d_cnt = want_cnt ? h->io_cand.as<uint64_t>() : nullptr;
  *d_grp = want_grp ? reinterpret_cast<uint64_t*>(h->io_cand.as<char>() + cb) : nullptr;
  return HS_OK;
}

// ---- hs_pssm_hit_counts / hs_pssm_refine: the position frequency matrices of a scan's hits (hs_pssm_counts.hip) ----
// Sites per work item for a batch of ns sites: what HS_OPT_PSSM_COUNT_CHUNK says, else ns / 4096 within 256 .. 2048.
// An item is one wave's serial walk over its sites (two dependent loads per step), so few long items leave a small
// batch waiting on a handful of waves; 4096 items are 16 waves on every CU.  At 2048 sites the flush of at most 2400
// bins is a twentieth of the item's 5 x 10^4 increments at k = 25.
uint32_t pssm_count_chunk(const hs_handle* h, uint32_t ns) {
  if (h->knobs.pssm_count_chunk) return h->knobs.pssm_count_chunk;
  return std::min(2048u, std::max(256u, (ns + 4095u) / 4096u));
}

// The weighted outputs of hs_pssm_weighted_counts (hs_pssm_weights.hip), on the device or the host: wcounts
// [nm][k][alphabet]; wsum [nm] and distinct [nm] may be null.
struct PssmWeightOut {
  uint64_t *wcounts = nullptr, *wsum = nullptr;
  uint32_t* distinct = nullptr;
};

// The call with every array on the device; the callers have checked the arguments and the values.  d_id_start null:
// every hit is a site; else the sites are the best ids of the batch's (profile, sequence) rows.  Every hit of a
// profile lies in one batch, so a batch finishes its profiles' counts -- and, with w given, the weights of its sites
// follow from them in a second stage over the same sites and work items.  w null: hs_pssm_hit_counts, launch for launch.
hs_status pssm_counts_core(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm, const uint64_t* d_id_start,
                           uint64_t n_seq, uint32_t* d_counts, uint64_t* d_cnt_out, uint64_t* d_used_out,
                           uint64_t* n_hits, const PssmWeightOut* w = nullptr) {
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  const int k = (int)h->p.k;
  const size_t cells = (size_t)h->p.k * h->alphabet;
  if (nm) HS_HIP(h, hipMemsetAsync(d_counts, 0, nm * cells * 4, h->stream));
  if (d_cnt_out && nm) HS_HIP(h, hipMemsetAsync(d_cnt_out, 0, nm * 8, h->stream));
  if (d_used_out && nm) HS_HIP(h, hipMemsetAsync(d_used_out, 0, nm * 8, h->stream));
  if (w && nm) {
    HS_HIP(h, hipMemsetAsync(w->wcounts, 0, nm * cells * 8, h->stream));
    if (w->wsum) HS_HIP(h, hipMemsetAsync(w->wsum, 0, nm * 8, h->stream));
    if (w->distinct) HS_HIP(h, hipMemsetAsync(w->distinct, 0, nm * 4, h->stream));
  }
  uint64_t sites = 0, items = 0;
  HS_CHECK(pssm_batches(h, d_S, d_t, nm, n_hits, [&](uint32_t m0, uint32_t mb, uint32_t nh) -> hs_status {
    const uint32_t *site_m = nullptr, *site_id = nullptr;
    uint32_t ns = 0;
    const size_t scan_items = hs_scan_u32_temp((size_t)mb + 1);
    if (!d_id_start) {  // the hits, ordered on their profile bits alone
      HS_HIP(h, h->pc_m.reserve((size_t)nh * 4));
      HS_HIP(h, h->pc_id.reserve((size_t)nh * 4));
      HS_HIP(h, h->pc_m2.reserve((size_t)nh * 4));
      HS_HIP(h, h->pc_id2.reserve((size_t)nh * 4));
      HS_HIP(h, h->temp.reserve(std::max(hs_sort_pairs_u32_u32_temp(nh), scan_items) + 256));
      HS_HIP(h, hs_launch_pssm_counts_split(h->hit_key.as<uint64_t>(), nh, h->pc_m.as<uint32_t>(),
                                            h->pc_id.as<uint32_t>(), h->stream));
      HS_HIP(h, hs_sort_pairs_u32_u32(h->temp.p, h->temp.cap, h->pc_m.as<uint32_t>(), h->pc_m2.as<uint32_t>(),
                                      h->pc_id.as<uint32_t>(), h->pc_id2.as<uint32_t>(), nh, bit_width_u32(m0 + mb),
                                      h->stream));
      site_m = h->pc_m2.as<uint32_t>();
      site_id = h->pc_id2.as<uint32_t>();
      ns = nh;
    } else {  // the rows of hs_pssm_seq_scan, kept on the device: their m and best_id are the sites
      HS_CHECK(pssm_row_pass(h, m0, mb, nh, d_id_start, n_seq, scan_items, nullptr, 0, 0, d_cnt_out, nullptr,
                             "hs_pssm_hit_counts", &ns));
      const PssmSeqOut rows = PssmSeqOut::in(h->pc_rows.as<char>(), ns);
      site_m = rows.m;
      site_id = rows.best_id;
    }
    const uint32_t ch = pssm_count_chunk(h, ns);
    HS_HIP(h, h->pc_start.reserve(((size_t)mb + 1) * 4));
    HS_HIP(h, h->pc_nitem.reserve(((size_t)mb + 1) * 4));
    HS_HIP(h, h->pc_off.reserve(((size_t)mb + 1) * 4));
    HS_HIP(h, hs_launch_pssm_counts_items(site_m, ns, m0, mb, ch, h->pc_start.as<uint32_t>(),
                                          h->pc_nitem.as<uint32_t>(), h->stream));
    HS_HIP(h, hs_exclusive_scan_u32(h->temp.p, h->temp.cap, h->pc_nitem.as<uint32_t>(), h->pc_off.as<uint32_t>(),
                                    (size_t)mb + 1, h->stream));
    uint32_t n_items = 0;
    HS_HIP(h, hipMemcpyAsync(&n_items, h->pc_off.as<uint32_t>() + mb, 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    if (!n_items || n_items > (uint64_t)ns / ch + mb)
      return fail(h, HS_ERR_HIP, "hs_pssm_hit_counts: the item count of a batch is out of range");
    HS_HIP(h, hs_launch_pssm_counts(h->codes.as<uint8_t>(), k, h->alphabet, site_id, h->pc_start.as<uint32_t>(),
                                    h->pc_off.as<uint32_t>(), m0, mb, ch, n_items, d_counts, h->stream));
    HS_HIP(h, hs_launch_pssm_counts_used(d_counts + (size_t)m0 * cells, mb, k, h->alphabet,
                                         d_used_out ? d_used_out + m0 : nullptr,
                                         d_cnt_out && !d_id_start ? d_cnt_out + m0 : nullptr, h->stream));
    if (w) {  // the batch's counts are final: u from them, the sites' weights, their sums
      HS_HIP(h, h->pw_u.reserve(hs_pssm_weights_table_bytes(mb, k, h->alphabet)));
      HS_HIP(h, hs_launch_pssm_weights_table(d_counts + (size_t)m0 * cells, mb, k, h->alphabet, h->pw_u.as<uint64_t>(),
                                             w->distinct ? w->distinct + m0 : nullptr, h->stream));
      HS_HIP(h, hs_launch_pssm_weights(h->codes.as<uint8_t>(), k, h->alphabet, site_id, h->pc_start.as<uint32_t>(),
                                       h->pc_off.as<uint32_t>(), m0, mb, ch, n_items, h->pw_u.as<uint64_t>(),
                                       w->wcounts, h->stream));
      HS_HIP(h, hs_launch_pssm_weights_sum(w->wcounts + (size_t)m0 * cells, mb, k, h->alphabet,
                                           w->wsum ? w->wsum + m0 : nullptr, h->stream));
    }
    sites += ns;
    items += n_items;
    return HS_OK;
  }));
  h->prof.pssm_count_sites = sites;
  h->prof.pssm_count_items = items;
  if (w) {
    h->prof.pssm_weight_sites = sites;
    h->prof.pssm_weight_items = items;
  }
  return HS_OK;
}

// what every form refuses from the arguments alone (hs_pssm_scan's refusals first); id_start null: every site counts
// (counts: the array the call must be given -- wcounts for the weighted call, whose text is counts_null then)
hs_status pssm_counts_args(hs_handle* h, const void* S, const void* t, uint64_t nm, const void* id_start,
                           uint64_t n_seq, const void* counts,
                           const char* counts_null = "hs_pssm_hit_counts: counts is null") {
  HS_CHECK(pssm_args_start(h, nm, S && t ? nullptr : "hs_pssm_hit_counts: S or t is null"));
  if (nm && !counts) return fail(h, HS_ERR_INVALID, counts_null);
  if (id_start && n_seq > (1ull << 32)) return fail(h, HS_ERR_INVALID, "hs_pssm_hit_counts: more than 2^32 sequences");
  if (id_start && !n_seq && h->n)
    return fail(h, HS_ERR_INVALID, "hs_pssm_hit_counts: no sequence owns the index's k-mers");
  return HS_OK;
}

// the values a host-pointer call refuses (t null: the thresholds are the call's own)
hs_status pssm_counts_values(hs_handle* h, const double* S, const double* t, uint64_t nm, const uint64_t* id_start,
                             uint64_t n_seq) {
  const uint32_t bad = pssm_host_bad(h, S, t, nm) | (id_start ? pssm_id_start_bad(h, id_start, n_seq) : 0u);
  return pssm_refuse(h, bad, "threshold", "hs_pssm_hit_counts");
}

// A checked host-pointer call: S and t up, counts (and cnt, used) down.  ids_resident: id_start already lies in sq_in
// (the later iterations of a refinement).  w (host arrays) given: the weighted call -- wcounts, wsum and distinct come
// down too, and counts may be null.
hs_status pssm_counts_host(hs_handle* h, const double* S, const double* t, uint64_t nm, const uint64_t* id_start,
                           uint64_t n_seq, bool ids_resident, uint32_t* counts, uint64_t* cnt, uint64_t* used,
                           uint64_t* n_hits, const PssmWeightOut* w = nullptr) {
  HS_CHECK(ensure_device(h));
  const size_t ka = (size_t)h->p.k * h->alphabet;
  const size_t sb = ((size_t)n_seq + 1) * 8, cb = std::max<size_t>(16, nm * 8), ob = std::max<size_t>(16, nm * ka * 4);
  HS_CHECK(pssm_stage_in(h, S, t, nm, h->io_radii));
  if (id_start) HS_HIP(h, h->sq_in.reserve(sb));
  HS_HIP(h, h->pc_out.reserve(2 * cb + ob));
  if (w) HS_HIP(h, h->pw_out.reserve(2 * cb + 2 * ob));
  if (id_start && !ids_resident)
    HS_HIP(h, hipMemcpyAsync(h->sq_in.p, id_start, sb, hipMemcpyHostToDevice, h->stream));
  char* const o = h->pc_out.as<char>();
  uint64_t* const d_cnt = cnt ? reinterpret_cast<uint64_t*>(o) : nullptr;
  uint64_t* const d_used = used ? reinterpret_cast<uint64_t*>(o + cb) : nullptr;
  uint32_t* const d_counts = reinterpret_cast<uint32_t*>(o + 2 * cb);
  PssmWeightOut dw;
  if (w) {  // wsum, distinct, wcounts in pw_out
    char* const wo = h->pw_out.as<char>();
    dw.wsum = w->wsum ? reinterpret_cast<uint64_t*>(wo) : nullptr;
    dw.distinct = w->distinct ? reinterpret_cast<uint32_t*>(wo + cb) : nullptr;
    dw.wcounts = reinterpret_cast<uint64_t*>(wo + 2 * cb);
  }
  HS_CHECK(pssm_counts_core(h, h->io_centers.as<double>(), h->io_radii.as<double>(), nm,
                            id_start ? h->sq_in.as<uint64_t>() : nullptr, n_seq, d_counts, d_cnt, d_used, n_hits,
                            w ? &dw : nullptr));
  if (nm) {
    if (counts) HS_HIP(h, hipMemcpyAsync(counts, d_counts, nm * ka * 4, hipMemcpyDeviceToHost, h->stream));
    if (cnt) HS_HIP(h, hipMemcpyAsync(cnt, d_cnt, nm * 8, hipMemcpyDeviceToHost, h->stream));
    if (used) HS_HIP(h, hipMemcpyAsync(used, d_used, nm * 8, hipMemcpyDeviceToHost, h->stream));
    if (w) {
      HS_HIP(h, hipMemcpyAsync(w->wcounts, dw.wcounts, nm * ka * 8, hipMemcpyDeviceToHost, h->stream));
      if (w->wsum) HS_HIP(h, hipMemcpyAsync(w->wsum, dw.wsum, nm * 8, hipMemcpyDeviceToHost, h->stream));
      if (w->distinct) HS_HIP(h, hipMemcpyAsync(w->distinct, dw.distinct, nm * 4, hipMemcpyDeviceToHost, h->stream));
    }
  }
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

// ---- hs_pssm_topk: the topk best k-mers per profile (kernels, the argument and the three steps: hs_pssm_topk.hip) ----
// The call with every array on the device; the callers have checked the arguments and the values.  d_floor, d_tused
// may be null.
hs_status pssm_topk_core(hs_handle* h, const double* d_S, const double* d_floor, uint64_t nm, uint32_t topk,
                         uint32_t* d_id, double* d_score, uint32_t* d_count, double* d_tused) {
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, h->knn_total.reserve(16));
  HS_HIP(h, hipMemsetAsync(h->knn_total.p, 0, 16, h->stream));  // the profiles raised above their floor
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  const uint32_t n = (uint32_t)h->n, n_s = (uint32_t)std::min<uint64_t>(h->n, h->knobs.pssm_topk_sample);
  uint64_t total = 0, raised = 0;
  // (an empty index runs no batch: nothing would write the rows)
  if (nm && !n) HS_HIP(h, hs_launch_pssm_topk_fill(nm, topk, d_floor, d_id, d_score, d_count, d_tused, h->stream));
  if (nm && n) {
    const size_t ka = (size_t)h->p.k * h->alphabet;
    // profiles per batch: at most 4096 and few enough that the hits to expect -- topk * n / n_s per profile -- stay
    // within 2^24
    const uint64_t per = std::max<uint64_t>(1, (uint64_t)topk * n / n_s);
    const uint32_t MB = (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(1, (1ull << 24) / per));
    const double* fl = nullptr;  // the batch's floors and thresholds used: step 1 sets them for steps 2 and 3
    double* tu = nullptr;
    HS_CHECK(pssm_batch_loop(
        h, d_S, nm, MB, true, true, &total,
        [&](uint32_t m0, uint32_t mb, const double** d_t) -> hs_status {  // 1. the sample pass: ms_hash
          if (!d_tused) HS_HIP(h, h->pt_tused.reserve((size_t)mb * 8));
          HS_HIP(h, h->pt_parts.reserve(std::max<size_t>(16, hs_pssm_sample_part_bytes(mb, n_s))));
          *d_t = tu = d_tused ? d_tused + m0 : h->pt_tused.as<double>();
          fl = d_floor ? d_floor + m0 : nullptr;
          HS_HIP(h, hipEventRecord(h->ev[10], h->stream));
          HS_HIP(h, hs_launch_pssm_sample(h->codes.as<uint8_t>(), d_S + m0 * ka, fl, (int)h->p.k, h->alphabet, n, n_s,
                                          topk, mb, h->pt_parts.p, tu, h->stream));
          HS_HIP(h, hipEventRecord(h->ev[11], h->stream));
          return HS_OK;
        },
        [&](uint32_t m0, uint32_t mb, uint32_t nh) -> hs_status {  // 3. the selection; it writes the rows
          const size_t words = ((size_t)mb + 1) * 4;
          HS_HIP(h, h->knn_cnt.reserve(words));
          HS_HIP(h, h->knn_off.reserve(words));
          HS_HIP(h, h->knn_cur.reserve(words));
          HS_HIP(h, h->hit_key2.reserve(std::max<size_t>(16, (size_t)nh * 8)));
          HS_HIP(h, h->hit_val2.reserve(std::max<size_t>(16, (size_t)nh * 8)));
          HS_HIP(h, h->temp.reserve(hs_pssm_topk_temp(mb) + 256));
          HS_HIP(h, hs_launch_pssm_topk_select(h->hit_key.as<uint64_t>(), h->hit_val.as<uint64_t>(), nh, m0, mb,
                                               h->knn_cnt.as<uint32_t>(), h->knn_off.as<uint32_t>(),
                                               h->knn_cur.as<uint32_t>(), h->temp.p, h->temp.cap,
                                               h->hit_key2.as<uint64_t>(), h->hit_val2.as<uint64_t>(), topk, fl, tu, d_id,
                                               d_score, d_count, h->knn_total.as<uint64_t>(), h->stream));
          return HS_OK;
        }));
    HS_HIP(h, hipMemcpyAsync(&raised, h->knn_total.p, 8, hipMemcpyDeviceToHost, h->stream));
  }
  HS_CHECK(pssm_call_end(h, total));
  h->prof.pssm_topk_sample = n_s;
  h->prof.pssm_topk_raised = raised;
  return HS_OK;
}

hs_status pssm_topk_args(hs_handle* h, const void* S, uint64_t nm, uint32_t topk, const void* top_id,
                         const void* top_score, const void* top_count) {
  HS_CHECK(pssm_args_start(h, nm, nullptr));
  if (!topk_ok(topk)) return fail(h, HS_ERR_INVALID, "hs_pssm_topk: topk must be 1 .. 64");
  if (nm && !S) return fail(h, HS_ERR_INVALID, "hs_pssm_topk: S is null");
  if (nm && (!top_id || !top_score || !top_count)) return fail(h, HS_ERR_INVALID, "an output array is null");
  return HS_OK;
}

// ---- hs_pssm_rank: the score of every profile's rank-th best k-mer (kernels, the argument, a round: hs_pssm_rank.hip) ----
// The call with every array on the device; the callers have checked the arguments and the values (so n > 0 where
// nm > 0) and know the largest rank.  d_tscan_out, d_rounds may be null.
hs_status pssm_rank_core(hs_handle* h, const double* d_S, const uint64_t* d_rank, uint64_t nm, uint64_t max_rank,
                         double* d_t_rank, uint64_t* d_ge, uint64_t* d_gt, double* d_tscan_out, uint32_t* d_rounds) {
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  const uint32_t n = (uint32_t)h->n, n_s = (uint32_t)std::min<uint64_t>(h->n, h->knobs.pssm_rank_sample);
  uint64_t total = 0, retries = 0;
  if (nm && n) {
    HS_HIP(h, h->pr_resolved.reserve(nm * 4));
    HS_HIP(h, h->pr_tscan.reserve(nm * 8));
    HS_HIP(h, h->pr_unres.reserve(16));
    uint32_t* const resolved = h->pr_resolved.as<uint32_t>();
    uint32_t* const d_unres = h->pr_unres.as<uint32_t>();
    double* const tscan = h->pr_tscan.as<double>();
    HS_HIP(h, hs_launch_pssm_rank_init(nm, resolved, d_unres, h->stream));
    const uint32_t SB = hs_pssm_rank_sample_batch(n_s);
    for (uint32_t round = 0;; ++round) {
      // 1. the sample pass and its select, in sub-batches of its own: the key buffer stays within 2^27 bytes
      HS_HIP(h, hipEventRecord(h->ev[10], h->stream));
      for (uint64_t m0 = 0; m0 < nm; m0 += SB) {
        const uint32_t mb = (uint32_t)std::min<uint64_t>(SB, nm - m0);
        HS_HIP(h, h->pr_keys.reserve((size_t)mb * n_s * 8));
        HS_HIP(h, h->pr_off.reserve(((size_t)mb + 1) * 4));
        HS_HIP(h, h->pr_state.reserve(hs_pssm_rank_state_bytes(mb)));
        HS_HIP(h, hs_launch_pssm_rank_sample(h->codes.as<uint8_t>(), d_S, d_rank, resolved, (int)h->p.k, h->alphabet, n,
                                             n_s, round, (uint32_t)m0, mb, h->pr_keys.as<uint64_t>(),
                                             h->pr_off.as<uint32_t>(), h->pr_state.p, tscan, d_tscan_out, h->stream));
      }
      HS_HIP(h, hipEventRecord(h->ev[11], h->stream));
      HS_HIP(h, hipMemsetAsync(d_unres, 0, 4, h->stream));
      HS_HIP(h, hipStreamSynchronize(h->stream));
      h->prof.ms_hash += ev_ms(h, 10, 11);
      // 2. the scan.  Profiles per batch: at most 4096 and few enough that the hits to expect -- the largest rank's
      // r_s * n / n_s per profile, n at the ladder's last rung -- stay within 2^24
      uint64_t r_s = 0;
      if (hs_pssm_rank_plan_rule(max_rank, n, n_s, round, &r_s)) return fail(h, HS_ERR_HIP, "hs_pssm_rank: no plan");
      const uint64_t per = r_s > n_s ? n : std::max<uint64_t>(1, r_s * n / n_s);
      const uint32_t MB = (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(1, (1ull << 24) / per));
      HS_CHECK(pssm_batch_loop(
          h, d_S, nm, MB, false, true, &total,
          [&](uint32_t m0, uint32_t, const double** d_t) -> hs_status {
            *d_t = tscan + m0;
            return HS_OK;
          },
          // 3. the selection and the resolve step; they run for a batch without hits too: its profiles are counted
          [&](uint32_t m0, uint32_t mb, uint32_t nh) -> hs_status {
            const size_t words = ((size_t)mb + 1) * 4;
            HS_HIP(h, h->knn_cnt.reserve(words));
            HS_HIP(h, h->knn_off.reserve(words));
            HS_HIP(h, h->knn_cur.reserve(words));
            HS_HIP(h, h->hit_key2.reserve(std::max<size_t>(16, (size_t)nh * 8)));
            HS_HIP(h, h->pr_state.reserve(hs_pssm_rank_state_bytes(mb)));
            HS_HIP(h, h->temp.reserve(hs_pssm_rank_temp(mb) + 256));
            HS_HIP(h, hs_launch_pssm_rank_select(h->hit_key.as<uint64_t>(), h->hit_val.as<uint64_t>(), nh, m0, mb,
                                                 h->knn_cnt.as<uint32_t>(), h->knn_off.as<uint32_t>(),
                                                 h->knn_cur.as<uint32_t>(), h->temp.p, h->temp.cap,
                                                 h->hit_key2.as<uint64_t>(), h->pr_state.p, d_rank, resolved, round,
                                                 d_t_rank, d_ge, d_gt, d_rounds, d_unres, h->stream));
            return HS_OK;
          }));
      uint32_t unresolved = 0;
      HS_HIP(h, hipMemcpyAsync(&unresolved, d_unres, 4, hipMemcpyDeviceToHost, h->stream));
      HS_HIP(h, hipStreamSynchronize(h->stream));
      if (!unresolved) break;
      retries += unresolved;  // (each of them takes one more round)
      // (the plan saturates beyond round 16: that round scans at -DBL_MAX and resolves everything)
      if (round >= 17) return fail(h, HS_ERR_HIP, "hs_pssm_rank: profiles left after the ladder's last rung");
    }
  }
  HS_CHECK(pssm_call_end(h, total));
  h->prof.pssm_rank_sample = n_s;
  h->prof.pssm_rank_retries = retries;
  return HS_OK;
}

hs_status pssm_rank_args(hs_handle* h, const void* S, const void* rank, uint64_t nm, const void* t_rank,
                         const void* cnt_ge, const void* cnt_gt) {
  HS_CHECK(pssm_args_start(h, nm, S ? nullptr : "hs_pssm_rank: S is null"));
  if (nm && (!rank || !t_rank || !cnt_ge || !cnt_gt))
    return fail(h, HS_ERR_INVALID, "hs_pssm_rank: rank or an output array is null");
  return HS_OK;
}

// The refine loop of hs_pssm_refine (by_rank false: every iteration scans at the thresholds t) and
// hs_pssm_refine_rank (by_rank: at the thresholds that admit rank[m] k-mers of the iteration's profiles, which
// hs_pssm_rank finds and t_out hands out): counts of the hits, log-odds against the background, until the counts repeat.
// neff_rule < 0: the sites count 1 each.  Else hs_pssm_refine_weighted: the scans are hs_pssm_weighted_counts', the
// log-odds hs_pssm_log_odds_weighted's with n_eff = used (rule 0) or distinct / k (rule 1), and the loop has converged
// when counts and wcounts both repeat; wo: where the last scan's wcounts, wsum and distinct go (each may be null).
hs_status pssm_refine(hs_handle* h, const double* S0, const double* t, const uint64_t* rank, bool by_rank, uint64_t nm,
                      const uint64_t* id_start, uint64_t n_seq, const double* bg, double pseudo, uint32_t n_iter,
                      double* S_out, double* t_out, uint32_t* counts, uint64_t* used, uint32_t* iters,
                      uint32_t* converged, int neff_rule = -1, const PssmWeightOut& wo = PssmWeightOut()) {
  if (!h || !iters || !converged) return HS_ERR_INVALID;
  *iters = 0;
  *converged = 0;
  const bool weighted = neff_rule >= 0;
  HS_CHECK(pssm_counts_args(h, S0, by_rank ? (const void*)rank : t, nm, id_start, n_seq, S_out));
  if (by_rank && nm && !t_out) return fail(h, HS_ERR_INVALID, "hs_pssm_refine_rank: t_out is null");
  if (n_iter < 1 || n_iter > 100) return fail(h, HS_ERR_INVALID, "hs_pssm_refine: n_iter must be 1 .. 100");
  if (neff_rule > 1) return fail(h, HS_ERR_INVALID, "hs_pssm_refine_weighted: neff_rule must be 0 or 1");
  const uint32_t k = h->p.k, A = (uint32_t)h->alphabet;
  double bgv[32];
  if (!(pseudo > 0.0 && pseudo <= 1.7976931348623157e308) || (bg && !hs_pssm_bg_ok(bg, A, pseudo)))
    return fail(h, HS_ERR_INVALID, "hs_pssm_refine: the background must be positive and finite, pseudo finite and > 0");
  HS_CHECK(pssm_counts_values(h, S0, by_rank ? nullptr : t, nm, id_start, n_seq));
  uint64_t max_rank = 0;
  if (by_rank) HS_CHECK(pssm_refuse(h, pssm_rank_bad(h, rank, nm, &max_rank), "threshold", "hs_pssm_rank"));
  const size_t cells = (size_t)k * A;
  try {
    uint64_t nh = 0;
    if (bg) {
      for (uint32_t a = 0; a < A; ++a) bgv[a] = bg[a];
    } else {  // the residue composition of the index: one profile that hits everything, every site counted
      const std::vector<double> zero(cells, 0.0);
      std::vector<uint32_t> all(cells);
      const double t0 = 0.0;
      HS_CHECK(pssm_counts_host(h, zero.data(), &t0, 1, nullptr, 0, false, all.data(), nullptr, nullptr, &nh));
      if (hs_pssm_background_host(all.data(), k, A, bgv))
        return fail(h, HS_ERR_INVALID, "hs_pssm_refine: an empty index has no background");
    }
    std::vector<double> S(S0, S0 + nm * cells), T(by_rank ? nm : 0, 0.0);
    std::vector<uint32_t> C(nm * cells), prev;
    std::vector<uint64_t> U(nm), ge(T.size()), gt(T.size());
    std::vector<uint64_t> WC(weighted ? nm * cells : 0), WS(weighted ? nm : 0), prev_w;
    std::vector<uint32_t> D(weighted ? nm : 0);
    PssmWeightOut wi;
    wi.wcounts = WC.data();
    wi.wsum = WS.data();
    wi.distinct = D.data();
    const double* const ti = by_rank ? T.data() : t;
    uint32_t done = 0, conv = 0;
    for (uint32_t i = 0; i < n_iter; ++i) {
      if (by_rank) HS_CHECK(hs_pssm_rank(h, S.data(), rank, nm, T.data(), ge.data(), gt.data(), nullptr, nullptr));
      HS_CHECK(pssm_counts_host(h, S.data(), ti, nm, id_start, n_seq, i > 0, C.data(), nullptr, U.data(), &nh,
                                weighted ? &wi : nullptr));
      ++done;
      if (i > 0 && C == prev && WC == prev_w) {
        conv = 1;
        break;
      }
      for (uint64_t m = 0; m < nm; ++m) {
        if (!U[m]) continue;  // a profile that finds nothing keeps its matrix
        int bad;
        if (weighted) {
          const double n_eff = neff_rule ? (double)D[m] / (double)k : (double)U[m];
          bad = hs_pssm_log_odds_weighted_host(WC.data() + m * cells, WS.data() + m, &n_eff, 1, k, A, bgv, pseudo,
                                               S.data() + m * cells);
        } else {
          bad = hs_pssm_log_odds_host(C.data() + m * cells, 1, k, A, bgv, pseudo, S.data() + m * cells);
        }
        if (bad) return fail(h, HS_ERR_INVALID, "hs_pssm_refine: a log-odds entry is not finite");
      }
      prev = C;
      prev_w = WC;
    }
    for (size_t i = 0; i < S.size(); ++i) S_out[i] = S[i];
    for (size_t m = 0; m < T.size(); ++m) t_out[m] = T[m];
    if (counts)
      for (size_t i = 0; i < C.size(); ++i) counts[i] = C[i];
    if (used)
      for (uint64_t m = 0; m < nm; ++m) used[m] = U[m];
    if (wo.wcounts)
      for (size_t i = 0; i < WC.size(); ++i) wo.wcounts[i] = WC[i];
    for (size_t m = 0; m < WS.size(); ++m) {
      if (wo.wsum) wo.wsum[m] = WS[m];
      if (wo.distinct) wo.distinct[m] = D[m];
    }
    *iters = done;
    *converged = conv;
  } catch (const std::bad_alloc&) {
    return fail(h, HS_ERR_NOMEM, "hs_pssm_refine: out of host memory");
  }
  return HS_OK;
}

// ---- hs_pssm_pvalue, hs_pssm_pvalue_threshold: the null-model score distribution (kernels: hs_pssm_null.hip) -------
// What both calls refuse from their arguments.  No index is needed unless the background is the index's composition.
hs_status pssm_null_args(hs_handle* h, const void* S, const void* bg, uint64_t nm, const char* name) {
  if (nm >= (1ull << 27)) return fail(h, HS_ERR_INVALID, "nm must be < 2^27 per call");
  if (nm && !S) return fail(h, HS_ERR_INVALID, std::string(name) + ": S is null");
  if (nm && !bg && (!h->built || !h->n))
    return fail(h, !h->built ? HS_ERR_STATE : HS_ERR_INVALID,
                std::string(name) + ": without bg the index must be built and hold k-mers");
  return HS_OK;
}

hs_status pssm_null_refuse(hs_handle* h, uint32_t bad, const char* name) {
  if (bad & BAD_S) return fail(h, HS_ERR_INVALID, "a profile entry is NaN, infinite or beyond 2^100");
  if (bad & BAD_T) return fail(h, HS_ERR_INVALID, std::string(name) + ": a t_lo is NaN or infinite");
  if (bad & 16u) return fail(h, HS_ERR_INVALID, std::string(name) + ": bg must lie in 0 .. 1 with one entry positive");
  if (bad & 32u) return fail(h, HS_ERR_INVALID, std::string(name) + ": a p is NaN or outside (0, 1]");
  if (bad & 64u) return fail(h, HS_ERR_INVALID, std::string(name) + ": a hit's profile is >= nm");
  if (bad & 128u) return fail(h, HS_ERR_INVALID, std::string(name) + ": a hit score is NaN");
  return HS_OK;
}

// the values of a host-pointer call
uint32_t pssm_null_host_bad(const hs_handle* h, const double* S, const double* bg, const double* t_lo, const double* p,
                            uint64_t nm, const uint32_t* hit_m, const double* hit_score, uint64_t n) {
  uint32_t bad = pssm_host_bad(h, S, t_lo, nm);
  if (bg && nm && !hs_pssm_null_bg_ok(bg, (uint32_t)h->alphabet)) bad |= 16u;
  for (uint64_t m = 0; p && m < nm; ++m)
    if (!hs_pssm_null_p_ok(p[m])) bad |= 32u;
  for (uint64_t i = 0; hit_m && i < n; ++i) {
    if (hit_m[i] >= nm) bad |= 64u;
    if (hit_score[i] != hit_score[i]) bad |= 128u;
  }
  return bad;
}

// ... of a device-pointer call: the reductions into pn_chk and one read-back
hs_status pssm_null_dev_check(hs_handle* h, const double* d_S, const double* d_bg, const double* d_t_lo,
                              const double* d_p, uint64_t nm, const uint32_t* d_hit_m, const double* d_hit_score,
                              uint64_t n, const char* name) {
  uint32_t bits = 0;
  HS_HIP(h, h->pn_chk.reserve(64));
  HS_HIP(h, hipMemsetAsync(h->pn_chk.p, 0, 64, h->stream));
  uint32_t* const d_bits = h->pn_chk.as<uint32_t>();
  HS_HIP(h, hs_launch_pssm_check(d_S, nm * h->p.k * h->alphabet, d_t_lo, d_t_lo ? nm : 0, d_bits, h->stream));
  HS_HIP(h, hs_launch_pssm_null_check(d_bg, (uint32_t)h->alphabet, d_p, nm, d_hit_m, d_hit_score, n, d_bits, h->stream));
  HS_HIP(h, hipMemcpyAsync(&bits, d_bits, 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return pssm_null_refuse(h, bits, name);
}

// bg == null: the index's residue composition as hs_pssm_refine takes it (one scan), into pn_bg; else *d_bg stays
hs_status pssm_null_background(hs_handle* h, const double** d_bg) {
  if (*d_bg) return HS_OK;
  const uint32_t k = h->p.k, A = (uint32_t)h->alphabet;
  double bgv[32];
  try {
    const std::vector<double> zero((size_t)k * A, 0.0);
    std::vector<uint32_t> all((size_t)k * A);
    const double t0 = 0.0;
    uint64_t nh = 0;
    HS_CHECK(pssm_counts_host(h, zero.data(), &t0, 1, nullptr, 0, false, all.data(), nullptr, nullptr, &nh));
    if (hs_pssm_background_host(all.data(), k, A, bgv))
      return fail(h, HS_ERR_INVALID, "hs_pssm_pvalue: an empty index has no background");
  } catch (const std::bad_alloc&) {
    return fail(h, HS_ERR_NOMEM, "hs_pssm_pvalue: out of host memory");
  }
  HS_HIP(h, h->pn_bg.reserve(32 * 8));
  HS_HIP(h, hipMemcpyAsync(h->pn_bg.p, bgv, A * 8, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));  // (bgv leaves scope)
  *d_bg = h->pn_bg.as<double>();
  return HS_OK;
}

// Both calls with every array on the device, checked, the background resolved (pssm_null_background: BEFORE a
// host-pointer call stages its S, as that scan stages its own).  d_p given: the thresholds (d_t_p, d_flag; d_p_hi / d_p_lo [nm]);
// else the lookups of the n hits (d_p_hi / d_p_lo [n]).  d_p_lo null: the upper side alone.  Profiles per batch:
// HS_OPT_QUERY_BATCH if set, else at most 4096 and few enough that the batch's cdf tables stay within 2^28 bytes.
hs_status pssm_null_core(hs_handle* h, const double* d_S, const double* d_bg, const double* d_t_lo, uint64_t nm,
                         const double* d_p, const uint32_t* d_hit_m, const double* d_hit_score, uint64_t n,
                         double* d_t_p, double* d_p_hi, double* d_p_lo, uint32_t* d_flag) {
  memset(&h->prof, 0, sizeof(h->prof));
  const uint32_t k = h->p.k, A = (uint32_t)h->alphabet, B = h->knobs.pssm_null_bins;
  const int sides = d_p_lo ? 2 : 1;
  const size_t ka = (size_t)k * A;
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  const uint32_t MB = h->knobs.query_batch
                          ? h->knobs.query_batch
                          : (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4096, (1ull << 28) / ((uint64_t)sides * B * 8)));
  for (uint64_t m0 = 0; m0 < nm; m0 += MB) {
    const uint32_t mb = (uint32_t)std::min<uint64_t>(MB, nm - m0);
    HS_HIP(h, h->pn_prof.reserve(hs_pssm_null_prof_bytes(mb)));
    HS_HIP(h, h->pn_q.reserve(2 * (size_t)mb * ka * 2));
    HS_HIP(h, h->pn_cdf.reserve((size_t)sides * mb * B * 8));
    uint16_t* const q_dn = h->pn_q.as<uint16_t>();
    HS_HIP(h, hipEventRecord(h->ev[10], h->stream));
    HS_HIP(h, hs_launch_pssm_null_tables(d_S + m0 * ka, d_bg, d_t_lo ? d_t_lo + m0 : nullptr, mb, k, A, B, sides,
                                         h->pn_prof.p, q_dn, q_dn + (size_t)mb * ka, h->pn_cdf.as<double>(),
                                         h->stream));
    HS_HIP(h, hipEventRecord(h->ev[11], h->stream));
    HS_HIP(h, hipEventRecord(h->ev[6], h->stream));
    if (d_p)
      HS_HIP(h, hs_launch_pssm_null_threshold(h->pn_prof.p, h->pn_cdf.as<double>(), mb, k, A, B, sides,
                                              d_t_lo ? d_t_lo + m0 : nullptr, d_p + m0, d_t_p + m0, d_p_hi + m0,
                                              d_p_lo ? d_p_lo + m0 : nullptr, d_flag + m0, h->stream));
    else
      HS_HIP(h, hs_launch_pssm_null_lookup(h->pn_prof.p, h->pn_cdf.as<double>(), (uint32_t)m0, mb, k, A, B, sides,
                                           d_hit_m, d_hit_score, n, d_p_hi, d_p_lo, h->stream));
    HS_HIP(h, hipEventRecord(h->ev[7], h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    h->prof.ms_hash += ev_ms(h, 10, 11);
    h->prof.ms_finalize += ev_ms(h, 6, 7);
  }
  HS_CHECK(pssm_call_end(h, 0));
  h->prof.pssm_null_bins = B;
  h->prof.pssm_null_profiles = nm;
  return HS_OK;
}

// ---- hs_pssm_compare: profile against profile at every offset (kernels: hs_pssm_compare.hip) ----------------------
// what the call refuses from its arguments (no index is needed).  Y null: self mode, ny is not looked at
hs_status pcmp_args(hs_handle* h, const void* X, uint64_t nx, const void* Y, uint64_t ny, const void* t, uint32_t v,
                    const void* hit_x, const void* hit_y, const void* hit_d, const void* hit_score, uint64_t cap) {
  if (nx >= (1ull << 27) || (Y && ny >= (1ull << 27)))
    return fail(h, HS_ERR_INVALID, "hs_pssm_compare: nx and ny must be < 2^27 per call");
  if (Y && (nx == 0) != (ny == 0)) return fail(h, HS_ERR_INVALID, "hs_pssm_compare: one of nx, ny is 0 and the other is not");
  if (v < 1 || v > h->p.k) return fail(h, HS_ERR_INVALID, "hs_pssm_compare: min_overlap must lie in 1..k");
  if (nx && (!X || !t)) return fail(h, HS_ERR_INVALID, "hs_pssm_compare: X or t is null");
  if (cap && (!hit_x || !hit_y || !hit_d || !hit_score)) return fail(h, HS_ERR_INVALID, "an output array is null");
  return HS_OK;
}

// the pairs a batch examines: profiles m0 .. m0 + mb - 1 of the call against ny (self: those with x < y, ny = nx)
uint64_t pcmp_pairs(uint64_t m0, uint64_t mb, uint64_t ny, bool self) {
  if (!self) return mb * ny;
  uint64_t pairs = 0;
  for (uint64_t x = m0; x < m0 + mb; ++x) pairs += ny - 1 - x;
  return pairs;
}

// One batch of mb X profiles (d_X, d_t: the batch's first; number m0 of the call) against all ny profiles d_Y: the
// tables and the int8 MFMA filter -- Y in chunks of 65536 profiles through one table buffer -- or, with the filter
// off, nothing; then the exact pass, under filter_passes' survivor protocol.  On success the batch's nh hits lie
// unordered in hit_key / hit_val.
hs_status pcmp_batch(hs_handle* h, const double* d_X, const double* d_t, uint32_t m0, uint32_t mb, const double* d_Y,
                     uint32_t ny, bool self, uint32_t v, bool filt, uint32_t* nh) {
  const uint32_t k = h->p.k, A = (uint32_t)h->alphabet, YC = 65536u;
  const hs_pcmp_shape sh = hs_pcmp_shape_of(k, A, v);
  const size_t ka = (size_t)k * A;
  uint32_t* const d_cnt = h->counters.as<uint32_t>();
  if (filt) {
    const size_t xr = (mb + 31u) & ~31u, yr = (std::min(ny, YC) + 31u) & ~31u;
    HS_HIP(h, h->pcm_xq.reserve(xr * sh.xrow));
    HS_HIP(h, h->pcm_xpar.reserve(xr * sizeof(hs_pcmp_par)));
    HS_HIP(h, h->pcm_yq.reserve(yr * sh.yrow));
    HS_HIP(h, h->pcm_ypar.reserve(yr * sizeof(hs_pcmp_par)));
  }
  HS_HIP(h, hipMemsetAsync(d_cnt, 0, 256, h->stream));
  HS_HIP(h, hipEventRecord(h->ev[0], h->stream));
  HS_HIP(h, hipEventRecord(h->ev[1], h->stream));
  HS_HIP(h, hipEventRecord(h->ev[2], h->stream));
  HS_CHECK(filter_passes(h, mb, 0, false, nh, [&](uint32_t prov_cap, uint32_t hit_cap, bool again) -> hs_status {
    HS_HIP(h, hipEventRecord(h->ev[3], h->stream));
    if (filt) {
      if (!again)
        HS_HIP(h, hs_launch_pcmp_tables(d_X, mb, k, A, sh.stride, sh.lead, sh.xrow, h->pcm_xq.p, h->pcm_xpar.p, h->stream));
      for (uint32_t y0 = 0; y0 < ny; y0 += YC) {
        const uint32_t nyc = std::min(YC, ny - y0);
        if (self && y0 + nyc - 1u <= m0) continue;  // no y of the chunk above the batch's first x
        HS_HIP(h, hs_launch_pcmp_tables(d_Y + y0 * ka, nyc, k, A, sh.stride, 0, sh.yrow, h->pcm_yq.p, h->pcm_ypar.p,
                                        h->stream));
        HS_HIP(h, hs_launch_pcmp_filter(h->pcm_xq.p, h->pcm_xpar.p, d_t, m0, mb, h->pcm_yq.p, h->pcm_ypar.p, y0, nyc, k, A,
                                        v, self, d_cnt, prov_cap, h->prov.as<uint2>(), h->stream));
      }
    }
    HS_HIP(h, hipEventRecord(h->ev[4], h->stream));
    HS_HIP(h, hs_launch_pcmp_exact(d_X, d_Y, d_t, k, A, v, m0, mb, ny, self, h->prov.as<uint2>(), d_cnt, prov_cap, !filt,
                                   hit_cap, h->hit_key.as<uint64_t>(), h->hit_val.as<uint64_t>(), h->n_cu, h->stream));
    HS_HIP(h, hipEventRecord(h->ev[5], h->stream));
    HS_HIP(h, hipMemcpyAsync(h->pin_cnt, d_cnt, HS_CNT_WORDS * 4, hipMemcpyDeviceToHost, h->stream));
    return HS_OK;
  }));
  const uint64_t pairs = pcmp_pairs(m0, mb, ny, self);
  h->prof.pssm_cmp_pairs += pairs;
  h->prof.pssm_cmp_survivors += filt ? (uint64_t)h->pin_cnt[0] : pairs;
  h->prof.pssm_cmp_steps = filt ? hs_pcmp_steps_issued(k, A, v) : 0;
  return HS_OK;
}

// The comparison with every array on the device (d_Y null: self mode); the callers have checked the arguments and
// the values.  X profiles per batch: 4096, or what HS_OPT_QUERY_BATCH says; a batch whose survivors overflow the
// counter runs again in halves, as pssm_batch_loop's do.
hs_status pcmp_core(hs_handle* h, const double* d_X, uint64_t nx, const double* d_Y, uint64_t ny, const double* d_t,
                    uint32_t v, uint32_t* d_hit_x, uint32_t* d_hit_y, int32_t* d_hit_d, double* d_hit_score,
                    uint64_t cap, uint64_t* n_hits, uint64_t* d_cnt_out) {
  const bool self = !d_Y;
  if (self) {
    d_Y = d_X;
    ny = nx;
  }
  const uint32_t k = h->p.k, A = (uint32_t)h->alphabet;
  const bool filt = !h->knobs.no_pssm_cmp_filter && hs_pcmp_shape_of(k, A, v).steps > 0;
  const size_t ka = (size_t)k * A;
  memset(&h->prof, 0, sizeof(h->prof));
  HS_HIP(h, h->counters.reserve(256));
  HS_HIP(h, hipEventRecord(h->ev[8], h->stream));
  if (d_cnt_out && nx) HS_HIP(h, hipMemsetAsync(d_cnt_out, 0, nx * 8, h->stream));
  uint64_t total = 0;
  uint32_t MB = h->knobs.query_batch ? h->knobs.query_batch : 4096u, mb = 0;
  for (uint64_t m0 = 0; m0 < nx && ny; m0 += mb) {
    mb = (uint32_t)std::min<uint64_t>(MB, nx - m0);
    if (self && m0 + 1 >= nx) break;  // the last profile has no partner above it
    uint32_t nh = 0;
    const hs_status st = pcmp_batch(h, d_X + m0 * ka, d_t + m0, (uint32_t)m0, mb, d_Y, (uint32_t)ny, self, v, filt, &nh);
    if (st == HS_SPLIT_BATCH) {
      if (mb == 1) return fail(h, HS_ERR_CAPACITY, "the filter survivors of one profile exceed 2^32");
      MB = (mb + 1) / 2;
      mb = 0;
      continue;
    }
    if (st) return st;
    if (nh) {
      HS_HIP(h, hipEventRecord(h->ev[6], h->stream));
      const uint64_t at = std::min<uint64_t>(total, cap);
      const bool fits = nh <= cap - at;
      const uint64_t *key = h->hit_key.as<uint64_t>(), *val = h->hit_val.as<uint64_t>();
      if (fits) {  // the order (x, y): the 64-bit sort on the key x << 35 | y << 8 | d + 128
        HS_HIP(h, h->hit_key2.reserve((size_t)nh * 8));
        HS_HIP(h, h->hit_val2.reserve((size_t)nh * 8));
        HS_HIP(h, h->temp.reserve(hs_sort_pairs_u64_u64_temp(nh) + 256));
        HS_HIP(h, hs_sort_pairs_u64_u64(h->temp.p, h->temp.cap, key, h->hit_key2.as<uint64_t>(), val,
                                        h->hit_val2.as<uint64_t>(), nh, 35 + bit_width_u32((uint32_t)m0 + mb), h->stream));
        key = h->hit_key2.as<uint64_t>();
        val = h->hit_val2.as<uint64_t>();
      }
      HS_HIP(h, hs_launch_pcmp_emit(key, val, nh, fits, fits ? d_hit_x + at : nullptr, fits ? d_hit_y + at : nullptr,
                                    fits ? d_hit_d + at : nullptr, fits ? d_hit_score + at : nullptr, d_cnt_out,
                                    h->stream));
      HS_HIP(h, hipEventRecord(h->ev[7], h->stream));
      HS_HIP(h, hipStreamSynchronize(h->stream));
      h->prof.ms_finalize += ev_ms(h, 6, 7);
    }
    total += nh;
  }
  HS_CHECK(pssm_call_end(h, total));
  *n_hits = total;
  if (total > cap) return fail(h, HS_ERR_CAPACITY, "hit buffers too small; see *n_hits");
  return HS_OK;
}

hs_status pssm_null_status(int r) { return r == 0 ? HS_OK : r == 1 ? HS_ERR_INVALID : HS_ERR_NOMEM; }

}  // namespace

extern "C" {

hs_status hs_pssm_scan_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm, uint32_t* d_hit_m,
                           uint32_t* d_hit_id, double* d_hit_score, uint64_t cap, uint64_t* n_hits, uint64_t* d_cnt) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  HS_CHECK(pssm_args(h, d_S, d_t, nm, d_hit_m, d_hit_id, d_hit_score, cap));
  HS_CHECK(ensure_device(h));
  HS_CHECK(pssm_dev_check(h, d_S, d_t, nm, nullptr, nullptr, 0, "threshold", "hs_pssm_scan", nullptr));
  return pssm_core(h, d_S, d_t, nm, d_hit_m, d_hit_id, d_hit_score, cap, n_hits, d_cnt);
}

hs_status hs_pssm_scan(hs_handle* h, const double* S, const double* t, uint64_t nm, uint32_t* hit_m, uint32_t* hit_id,
                       double* hit_score, uint64_t cap, uint64_t* n_hits, uint64_t* cnt) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  HS_CHECK(pssm_args(h, S, t, nm, hit_m, hit_id, hit_score, cap));
  HS_CHECK(pssm_refuse(h, pssm_host_bad(h, S, t, nm), "threshold", "hs_pssm_scan"));
  HS_CHECK(ensure_device(h));
  HS_CHECK(pssm_stage_in(h, S, t, nm, h->io_radii));
  HS_HIP(h, h->io_q.reserve(std::max<size_t>(16, cap * 4)));
  HS_HIP(h, h->io_id.reserve(std::max<size_t>(16, cap * 4)));
  HS_HIP(h, h->io_dist.reserve(std::max<size_t>(16, cap * 8)));
  if (cnt) HS_HIP(h, h->io_cand.reserve(std::max<size_t>(16, nm * 8)));
  const hs_status st = pssm_core(h, h->io_centers.as<double>(), h->io_radii.as<double>(), nm, h->io_q.as<uint32_t>(),
                                 h->io_id.as<uint32_t>(), h->io_dist.as<double>(), cap, n_hits,
                                 cnt ? h->io_cand.as<uint64_t>() : nullptr);
  if (st != HS_OK && st != HS_ERR_CAPACITY) return st;
  if (cnt && nm) HS_HIP(h, hipMemcpyAsync(cnt, h->io_cand.p, nm * 8, hipMemcpyDeviceToHost, h->stream));
  const uint64_t nh = *n_hits;
  if (st == HS_OK && nh) {
    HS_HIP(h, hipMemcpyAsync(hit_m, h->io_q.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(hit_id, h->io_id.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(hit_score, h->io_dist.p, nh * 8, hipMemcpyDeviceToHost, h->stream));
  }
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return st;
}

// The filter's tables on the host (hs_pssm_tables.h): no GPU, no handle
hs_status hs_pssm_tables(const double* S, const double* t, uint64_t nm, uint32_t k, uint32_t alphabet, uint8_t* code,
                         double* tau, uint8_t* dead) {
  return hs_pssm_tables_host(S, t, nm, k, alphabet, code, tau, dead) ? HS_ERR_INVALID : HS_OK;
}

hs_status hs_pssm_seq_scan_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm,
                               const uint64_t* d_id_start, uint64_t n_seq, uint32_t* d_out_m, uint32_t* d_out_seq,
                               uint32_t* d_out_count, double* d_out_best_score, uint32_t* d_out_best_id,
                               uint32_t* d_out_lo, uint32_t* d_out_hi, uint64_t cap, uint64_t* n_out, uint64_t* n_hits,
                               uint64_t* d_cnt, uint64_t* d_seq_cnt) {
  if (!h || !n_out || !n_hits) return HS_ERR_INVALID;
  *n_out = 0;
  *n_hits = 0;
  const PssmSeqOut out{d_out_m, d_out_seq, d_out_count, d_out_best_score, d_out_best_id, d_out_lo, d_out_hi};
  HS_CHECK(pssm_seq_args(h, d_S, d_t, nm, d_id_start, n_seq, out, cap));
  HS_CHECK(ensure_device(h));
  HS_CHECK(pssm_dev_check(h, d_S, d_t, nm, nullptr, d_id_start, n_seq, "threshold", "hs_pssm_seq_scan", nullptr));
  return pssm_seq_core(h, d_S, d_t, nm, d_id_start, n_seq, out, cap, n_out, n_hits, d_cnt, d_seq_cnt);
}

hs_status hs_pssm_seq_scan(hs_handle* h, const double* S, const double* t, uint64_t nm, const uint64_t* id_start,
                           uint64_t n_seq, uint32_t* out_m, uint32_t* out_seq, uint32_t* out_count,
                           double* out_best_score, uint32_t* out_best_id, uint32_t* out_lo, uint32_t* out_hi,
                           uint64_t cap, uint64_t* n_out, uint64_t* n_hits, uint64_t* cnt, uint64_t* seq_cnt) {
  if (!h || !n_out || !n_hits) return HS_ERR_INVALID;
  *n_out = 0;
  *n_hits = 0;
  const PssmSeqOut out{out_m, out_seq, out_count, out_best_score, out_best_id, out_lo, out_hi};
  HS_CHECK(pssm_seq_args(h, S, t, nm, id_start, n_seq, out, cap));
  HS_CHECK(pssm_refuse(h, pssm_host_bad(h, S, t, nm) | pssm_id_start_bad(h, id_start, n_seq), "threshold",
                       "hs_pssm_seq_scan"));
  HS_CHECK(ensure_device(h));
  // the rows are staged on the device at the caller's capacity: 32 bytes per row cross PCIe, never the hits
  const size_t sb = ((size_t)n_seq + 1) * 8, cb = std::max<size_t>(16, nm * 8);
  HS_CHECK(pssm_stage_in(h, S, t, nm, h->io_radii));
  HS_HIP(h, h->sq_in.reserve(sb));
  HS_HIP(h, h->sq_out.reserve(std::max<size_t>(64, (size_t)cap * 32)));
  if (cnt || seq_cnt) HS_HIP(h, h->io_cand.reserve(2 * cb));
  HS_HIP(h, hipMemcpyAsync(h->sq_in.p, id_start, sb, hipMemcpyHostToDevice, h->stream));
  const PssmSeqOut dev = PssmSeqOut::in(h->sq_out.as<char>(), cap);
  uint64_t* const d_cnt = cnt ? h->io_cand.as<uint64_t>() : nullptr;
  uint64_t* const d_seq_cnt = seq_cnt ? reinterpret_cast<uint64_t*>(h->io_cand.as<char>() + cb) : nullptr;
  const hs_status st = pssm_seq_core(h, h->io_centers.as<double>(), h->io_radii.as<double>(), nm,
                                     h->sq_in.as<uint64_t>(), n_seq, dev, cap, n_out, n_hits, d_cnt, d_seq_cnt);
  if (st != HS_OK && st != HS_ERR_CAPACITY) return st;
  if (cnt && nm) HS_HIP(h, hipMemcpyAsync(cnt, d_cnt, nm * 8, hipMemcpyDeviceToHost, h->stream));
  if (seq_cnt && nm) HS_HIP(h, hipMemcpyAsync(seq_cnt, d_seq_cnt, nm * 8, hipMemcpyDeviceToHost, h->stream));
  const size_t r = (size_t)*n_out;
  if (st == HS_OK && r) {
    HS_HIP(h, hipMemcpyAsync(out_m, dev.m, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_seq, dev.seq, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_count, dev.count, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_best_score, dev.best_score, r * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_best_id, dev.best_id, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_lo, dev.lo, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_hi, dev.hi, r * 4, hipMemcpyDeviceToHost, h->stream));
  }
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return st;
}

hs_status hs_pssm_family_scan_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm,
                                  const uint32_t* d_m_group, uint64_t n_groups, const uint32_t* d_m_off,
                                  const uint64_t* d_id_start, uint64_t n_seq, uint32_t min_count,
                                  const double* d_t_group, uint32_t* d_out_group, uint32_t* d_out_seq,
                                  int32_t* d_out_diag, uint32_t* d_out_count, double* d_out_sum,
                                  double* d_out_best_score, uint32_t* d_out_best_m, uint32_t* d_out_best_id,
                                  uint32_t* d_out_lo, uint32_t* d_out_hi, uint64_t cap, uint64_t* n_out,
                                  uint64_t* n_hits, uint64_t* d_cnt, uint64_t* d_grp_rows) {
  if (!h || !n_out || !n_hits) return HS_ERR_INVALID;
  *n_out = 0;
  *n_hits = 0;
  const HsFamilyOut out{d_out_group,      d_out_seq,    d_out_diag,    d_out_count, d_out_sum,
                        d_out_best_score, d_out_best_m, d_out_best_id, d_out_lo,    d_out_hi};
  HS_CHECK(pssm_family_args(h, FAMILY_NAME, d_S, d_t, nm, d_m_group != nullptr, n_groups, d_id_start, n_seq, min_count,
                            out.all(), cap));
  PssmFamily f;
  std::vector<uint32_t> cuts;
  HS_CHECK(pssm_family_dev_check(h, FAMILY_NAME, d_S, d_t, nm, d_m_group, n_groups, d_m_off, d_id_start, n_seq,
                                 min_count, d_t_group, ~(uint32_t)HS_FAM_BAD_OFF_ORDER, &f, &cuts));
  return pssm_family_core(h, d_S, d_t, nm, f, out, cap, n_out, n_hits, d_cnt, d_grp_rows);
}

hs_status hs_pssm_family_scan(hs_handle* h, const double* S, const double* t, uint64_t nm, const uint32_t* m_group,
                              uint64_t n_groups, const uint32_t* m_off, const uint64_t* id_start, uint64_t n_seq,
                              uint32_t min_count, const double* t_group, uint32_t* out_group, uint32_t* out_seq,
                              int32_t* out_diag, uint32_t* out_count, double* out_sum, double* out_best_score,
                              uint32_t* out_best_m, uint32_t* out_best_id, uint32_t* out_lo, uint32_t* out_hi,
                              uint64_t cap, uint64_t* n_out, uint64_t* n_hits, uint64_t* cnt, uint64_t* grp_rows) {
  if (!h || !n_out || !n_hits) return HS_ERR_INVALID;
  *n_out = 0;
  *n_hits = 0;
  const HsFamilyOut out{out_group, out_seq, out_diag, out_count, out_sum, out_best_score, out_best_m, out_best_id,
                        out_lo,    out_hi};
  HS_CHECK(pssm_family_args(h, FAMILY_NAME, S, t, nm, m_group != nullptr, n_groups, id_start, n_seq, min_count, out.all(),
                            cap));
  PssmFamily f;
  std::vector<uint32_t> cuts;
  HS_CHECK(pssm_family_host_check(h, FAMILY_NAME, S, t, nm, m_group, n_groups, m_off, id_start, n_seq, min_count, t_group,
                                  ~(uint32_t)HS_FAM_BAD_OFF_ORDER, &f, &cuts));
  // the rows are staged on the device at the caller's capacity: 48 bytes per row cross PCIe, never the hits
  uint64_t *d_cnt = nullptr, *d_grp = nullptr;
  HS_CHECK(pssm_family_stage(h, S, t, nm, m_group, n_groups, m_off, id_start, n_seq, t_group, cnt != nullptr,
                             grp_rows != nullptr, (size_t)cap * 48, &f, &d_cnt, &d_grp));
  const HsFamilyOut dev = HsFamilyOut::in(h->sq_out.as<char>(), cap);
  const hs_status st = pssm_family_core(h, h->io_centers.as<double>(), h->io_radii.as<double>(), nm, f, dev, cap, n_out,
                                        n_hits, d_cnt, d_grp);
  if (st != HS_OK && st != HS_ERR_CAPACITY) return st;
  if (st == HS_ERR_CAPACITY && *n_out <= cap) return st;  // (one group's survivors: no count is valid)
  if (cnt && nm) HS_HIP(h, hipMemcpyAsync(cnt, d_cnt, nm * 8, hipMemcpyDeviceToHost, h->stream));
  if (grp_rows && n_groups) HS_HIP(h, hipMemcpyAsync(grp_rows, d_grp, n_groups * 8, hipMemcpyDeviceToHost, h->stream));
  const size_t r = (size_t)*n_out;
  if (st == HS_OK && r) {
    HS_HIP(h, hipMemcpyAsync(out_group, dev.group, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_seq, dev.seq, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_diag, dev.diag, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_count, dev.count, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_sum, dev.sum, r * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_best_score, dev.best_score, r * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_best_m, dev.best_m, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_best_id, dev.best_id, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_lo, dev.lo, r * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(out_hi, dev.hi, r * 4, hipMemcpyDeviceToHost, h->stream));
  }
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return st;
}

hs_status hs_pssm_family_chain_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm,
                                   const uint32_t* d_m_group, uint64_t n_groups, const uint32_t* d_m_off,
                                   const uint64_t* d_id_start, uint64_t n_seq, uint32_t max_shift, double gap_open,
                                   double gap_ext, uint32_t min_count, const double* d_t_group, uint32_t* d_out_group,
                                   uint32_t* d_out_seq, uint32_t* d_out_count, uint32_t* d_out_gaps, double* d_out_score,
                                   uint32_t* d_out_first_m, uint32_t* d_out_first_id, uint32_t* d_out_last_m,
                                   uint32_t* d_out_last_id, int32_t* d_out_shift, uint64_t cap, uint64_t* n_out,
                                   uint64_t* n_hits, uint64_t* d_cnt, uint64_t* d_grp_rows) {
  if (!h || !n_out || !n_hits) return HS_ERR_INVALID;
  *n_out = 0;
  *n_hits = 0;
  const HsChainOut out{d_out_group,   d_out_seq,      d_out_count,  d_out_gaps,    d_out_score,
                       d_out_first_m, d_out_first_id, d_out_last_m, d_out_last_id, d_out_shift};
  PssmChain c;
  c.max_shift = max_shift;
  c.gap_open = gap_open;
  c.gap_ext = gap_ext;
  HS_CHECK(pssm_family_args(h, CHAIN_NAME, d_S, d_t, nm, d_m_group != nullptr, n_groups, d_id_start, n_seq, min_count,
                            out.all(), cap));
  HS_CHECK(pssm_chain_args(h, d_m_off, c));
  PssmFamily f;
  std::vector<uint32_t> cuts;
  HS_CHECK(pssm_family_dev_check(h, CHAIN_NAME, d_S, d_t, nm, d_m_group, n_groups, d_m_off, d_id_start, n_seq, min_count,
                                 d_t_group, ~0u, &f, &cuts));
  return pssm_chain_core(h, d_S, d_t, nm, f, c, out, cap, n_out, n_hits, d_cnt, d_grp_rows);
}

hs_status hs_pssm_family_chain(hs_handle* h, const double* S, const double* t, uint64_t nm, const uint32_t* m_group,
                               uint64_t n_groups, const uint32_t* m_off, const uint64_t* id_start, uint64_t n_seq,
                               uint32_t max_shift, double gap_open, double gap_ext, uint32_t min_count,
                               const double* t_group, uint32_t* out_group, uint32_t* out_seq, uint32_t* out_count,
                               uint32_t* out_gaps, double* out_score, uint32_t* out_first_m, uint32_t* out_first_id,
                               uint32_t* out_last_m, uint32_t* out_last_id, int32_t* out_shift, uint64_t cap,
                               uint64_t* n_out, uint64_t* n_hits, uint64_t* cnt, uint64_t* grp_rows) {
  if (!h || !n_out || !n_hits) return HS_ERR_INVALID;
  *n_out = 0;
  *n_hits = 0;
  const HsChainOut out{out_group,   out_seq,      out_count,  out_gaps,    out_score,
                       out_first_m, out_first_id, out_last_m, out_last_id, out_shift};
  PssmChain c;
  c.max_shift = max_shift;
  c.gap_open = gap_open;
  c.gap_ext = gap_ext;
  HS_CHECK(pssm_family_args(h, CHAIN_NAME, S, t, nm, m_group != nullptr, n_groups, id_start, n_seq, min_count, out.all(),
                            cap));
  HS_CHECK(pssm_chain_args(h, m_off, c));
  PssmFamily f;
  std::vector<uint32_t> cuts;
  HS_CHECK(pssm_family_host_check(h, CHAIN_NAME, S, t, nm, m_group, n_groups, m_off, id_start, n_seq, min_count, t_group,
                                  ~0u, &f, &cuts));
  // the rows are staged on the device at the caller's capacity: 44 bytes per row cross PCIe, never the hits
  uint64_t *d_cnt = nullptr, *d_grp = nullptr;
  HS_CHECK(pssm_family_stage(h, S, t, nm, m_group, n_groups, m_off, id_start, n_seq, t_group, cnt != nullptr,
                             grp_rows != nullptr, (size_t)cap * 44, &f, &d_cnt, &d_grp));
  const HsChainOut dev = HsChainOut::in(h->sq_out.as<char>(), cap);
  const hs_status st = pssm_chain_core(h, h->io_centers.as<double>(), h->io_radii.as<double>(), nm, f, c, dev, cap, n_out,
                                       n_hits, d_cnt, d_grp);
  if (st != HS_OK && st != HS_ERR_CAPACITY) return st;
  if (st == HS_ERR_CAPACITY && *n_out <= cap) return st;  // (one group's survivors: no count is valid)
  if (cnt && nm) HS_HIP(h, hipMemcpyAsync(cnt, d_cnt, nm * 8, hipMemcpyDeviceToHost, h->stream));
  if (grp_rows && n_groups) HS_HIP(h, hipMemcpyAsync(grp_rows, d_grp, n_groups * 8, hipMemcpyDeviceToHost, h->stream));
  const size_t r = (size_t)*n_out;
  if (st == HS_OK && r) {
    const struct {
      void* to;
      const void* from;
      size_t bytes;
    } copies[10] = {{out_group, dev.group, 4},       {out_seq, dev.seq, 4},         {out_count, dev.count, 4},
                    {out_gaps, dev.gaps, 4},         {out_score, dev.score, 8},     {out_first_m, dev.first_m, 4},
                    {out_first_id, dev.first_id, 4}, {out_last_m, dev.last_m, 4},   {out_last_id, dev.last_id, 4},
                    {out_shift, dev.shift, 4}};
    for (const auto& cp : copies)
      HS_HIP(h, hipMemcpyAsync(cp.to, cp.from, r * cp.bytes, hipMemcpyDeviceToHost, h->stream));
  }
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return st;
}

hs_status hs_pssm_hit_counts_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm,
                                 const uint64_t* d_id_start, uint64_t n_seq, uint32_t* d_counts, uint64_t* d_cnt,
                                 uint64_t* d_used, uint64_t* n_hits) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  HS_CHECK(pssm_counts_args(h, d_S, d_t, nm, d_id_start, n_seq, d_counts));
  HS_CHECK(ensure_device(h));
  HS_CHECK(pssm_dev_check(h, d_S, d_t, nm, nullptr, d_id_start, n_seq, "threshold", "hs_pssm_hit_counts", nullptr));
  return pssm_counts_core(h, d_S, d_t, nm, d_id_start, n_seq, d_counts, d_cnt, d_used, n_hits);
}

hs_status hs_pssm_hit_counts(hs_handle* h, const double* S, const double* t, uint64_t nm, const uint64_t* id_start,
                             uint64_t n_seq, uint32_t* counts, uint64_t* cnt, uint64_t* used, uint64_t* n_hits) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  HS_CHECK(pssm_counts_args(h, S, t, nm, id_start, n_seq, counts));
  HS_CHECK(pssm_counts_values(h, S, t, nm, id_start, n_seq));
  return pssm_counts_host(h, S, t, nm, id_start, n_seq, false, counts, cnt, used, n_hits);
}

hs_status hs_pssm_weighted_counts_dev(hs_handle* h, const double* d_S, const double* d_t, uint64_t nm,
                                      const uint64_t* d_id_start, uint64_t n_seq, uint32_t* d_counts,
                                      uint64_t* d_wcounts, uint64_t* d_wsum, uint32_t* d_distinct, uint64_t* d_cnt,
                                      uint64_t* d_used, uint64_t* n_hits) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  HS_CHECK(pssm_counts_args(h, d_S, d_t, nm, d_id_start, n_seq, d_wcounts, "hs_pssm_weighted_counts: wcounts is null"));
  HS_CHECK(ensure_device(h));
  HS_CHECK(pssm_dev_check(h, d_S, d_t, nm, nullptr, d_id_start, n_seq, "threshold", "hs_pssm_hit_counts", nullptr));
  if (!d_counts) {  // the raw counts stay in the handle's scratch
    HS_HIP(h, h->pw_counts.reserve(std::max<size_t>(16, nm * h->p.k * h->alphabet * 4)));
    d_counts = h->pw_counts.as<uint32_t>();
  }
  PssmWeightOut w;
  w.wcounts = d_wcounts;
  w.wsum = d_wsum;
  w.distinct = d_distinct;
  return pssm_counts_core(h, d_S, d_t, nm, d_id_start, n_seq, d_counts, d_cnt, d_used, n_hits, &w);
}

hs_status hs_pssm_weighted_counts(hs_handle* h, const double* S, const double* t, uint64_t nm, const uint64_t* id_start,
                                  uint64_t n_seq, uint32_t* counts, uint64_t* wcounts, uint64_t* wsum,
                                  uint32_t* distinct, uint64_t* cnt, uint64_t* used, uint64_t* n_hits) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  HS_CHECK(pssm_counts_args(h, S, t, nm, id_start, n_seq, wcounts, "hs_pssm_weighted_counts: wcounts is null"));
  HS_CHECK(pssm_counts_values(h, S, t, nm, id_start, n_seq));
  PssmWeightOut w;
  w.wcounts = wcounts;
  w.wsum = wsum;
  w.distinct = distinct;
  return pssm_counts_host(h, S, t, nm, id_start, n_seq, false, counts, cnt, used, n_hits, &w);
}

hs_status hs_pssm_topk_dev(hs_handle* h, const double* d_S, const double* d_floor, uint64_t nm, uint32_t topk,
                           uint32_t* d_top_id, double* d_top_score, uint32_t* d_top_count, double* d_t_used) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(pssm_topk_args(h, d_S, nm, topk, d_top_id, d_top_score, d_top_count));
  HS_CHECK(ensure_device(h));
  HS_CHECK(pssm_dev_check(h, d_S, d_floor, nm, nullptr, nullptr, 0, "floor", "hs_pssm_topk", nullptr));
  return pssm_topk_core(h, d_S, d_floor, nm, topk, d_top_id, d_top_score, d_top_count, d_t_used);
}

hs_status hs_pssm_topk(hs_handle* h, const double* S, const double* t_floor, uint64_t nm, uint32_t topk,
                       uint32_t* top_id, double* top_score, uint32_t* top_count, double* t_used) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(pssm_topk_args(h, S, nm, topk, top_id, top_score, top_count));
  HS_CHECK(pssm_refuse(h, pssm_host_bad(h, S, t_floor, nm), "floor", "hs_pssm_topk"));
  HS_CHECK(ensure_device(h));
  const size_t e = (size_t)nm * topk;
  HS_CHECK(pssm_stage_in(h, S, t_floor, nm, h->io_cand));
  HS_HIP(h, h->io_id.reserve(std::max<size_t>(16, e * 4)));
  HS_HIP(h, h->io_dist.reserve(std::max<size_t>(16, e * 8)));
  HS_HIP(h, h->knn_io_count.reserve(std::max<size_t>(16, nm * 4)));
  if (t_used) HS_HIP(h, h->io_radii.reserve(std::max<size_t>(16, nm * 8)));
  // the rows are selected on the device: topk x 12 + 4 (+ 8) bytes per profile cross PCIe
  HS_CHECK(pssm_topk_core(h, h->io_centers.as<double>(), t_floor ? h->io_cand.as<double>() : nullptr, nm, topk,
                          h->io_id.as<uint32_t>(), h->io_dist.as<double>(), h->knn_io_count.as<uint32_t>(),
                          t_used ? h->io_radii.as<double>() : nullptr));
  if (nm) {
    HS_HIP(h, hipMemcpyAsync(top_id, h->io_id.p, e * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(top_score, h->io_dist.p, e * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(top_count, h->knn_io_count.p, nm * 4, hipMemcpyDeviceToHost, h->stream));
    if (t_used) HS_HIP(h, hipMemcpyAsync(t_used, h->io_radii.p, nm * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return HS_OK;
}

hs_status hs_pssm_rank_dev(hs_handle* h, const double* d_S, const uint64_t* d_rank, uint64_t nm, double* d_t_rank,
                           uint64_t* d_cnt_ge, uint64_t* d_cnt_gt, double* d_t_scan, uint32_t* d_rounds) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(pssm_rank_args(h, d_S, d_rank, nm, d_t_rank, d_cnt_ge, d_cnt_gt));
  HS_CHECK(ensure_device(h));
  uint64_t max_rank = 0;
  HS_CHECK(pssm_dev_check(h, d_S, nullptr, nm, d_rank, nullptr, 0, "threshold", "hs_pssm_rank", &max_rank));
  return pssm_rank_core(h, d_S, d_rank, nm, max_rank, d_t_rank, d_cnt_ge, d_cnt_gt, d_t_scan, d_rounds);
}

hs_status hs_pssm_rank(hs_handle* h, const double* S, const uint64_t* rank, uint64_t nm, double* t_rank,
                       uint64_t* cnt_ge, uint64_t* cnt_gt, double* t_scan, uint32_t* rounds) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(pssm_rank_args(h, S, rank, nm, t_rank, cnt_ge, cnt_gt));
  uint64_t max_rank = 0;
  uint32_t bad = pssm_host_bad(h, S, nullptr, nm);
  if (!bad) bad = pssm_rank_bad(h, rank, nm, &max_rank);
  HS_CHECK(pssm_refuse(h, bad, "threshold", "hs_pssm_rank"));
  HS_CHECK(ensure_device(h));
  const size_t cb = std::max<size_t>(16, nm * 8);
  HS_CHECK(pssm_stage_in(h, S, rank, nm, h->pr_rank));
  HS_HIP(h, h->pr_out.reserve(5 * cb));
  // one double and two counts per profile (and the diagnostics) cross PCIe
  char* const o = h->pr_out.as<char>();
  double* const d_t = reinterpret_cast<double*>(o);
  uint64_t* const d_ge = reinterpret_cast<uint64_t*>(o + cb);
  uint64_t* const d_gt = reinterpret_cast<uint64_t*>(o + 2 * cb);
  double* const d_ts = t_scan ? reinterpret_cast<double*>(o + 3 * cb) : nullptr;
  uint32_t* const d_ro = rounds ? reinterpret_cast<uint32_t*>(o + 4 * cb) : nullptr;
  HS_CHECK(pssm_rank_core(h, h->io_centers.as<double>(), h->pr_rank.as<uint64_t>(), nm, max_rank, d_t, d_ge, d_gt, d_ts,
                          d_ro));
  if (nm) {
    HS_HIP(h, hipMemcpyAsync(t_rank, d_t, nm * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(cnt_ge, d_ge, nm * 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(cnt_gt, d_gt, nm * 8, hipMemcpyDeviceToHost, h->stream));
    if (t_scan) HS_HIP(h, hipMemcpyAsync(t_scan, d_ts, nm * 8, hipMemcpyDeviceToHost, h->stream));
    if (rounds) HS_HIP(h, hipMemcpyAsync(rounds, d_ro, nm * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
  }
  return HS_OK;
}

hs_status hs_pssm_refine(hs_handle* h, const double* S0, const double* t, uint64_t nm, const uint64_t* id_start,
                         uint64_t n_seq, const double* bg, double pseudo, uint32_t n_iter, double* S_out,
                         uint32_t* counts, uint64_t* used, uint32_t* iters, uint32_t* converged) {
  return pssm_refine(h, S0, t, nullptr, false, nm, id_start, n_seq, bg, pseudo, n_iter, S_out, nullptr, counts, used,
                     iters, converged);
}

// hs_pssm_refine with the threshold rule: every iteration scans at the threshold that admits rank[m] k-mers of S_i
hs_status hs_pssm_refine_rank(hs_handle* h, const double* S0, const uint64_t* rank, uint64_t nm,
                              const uint64_t* id_start, uint64_t n_seq, const double* bg, double pseudo, uint32_t n_iter,
                              double* S_out, double* t_out, uint32_t* counts, uint64_t* used, uint32_t* iters,
                              uint32_t* converged) {
  return pssm_refine(h, S0, nullptr, rank, true, nm, id_start, n_seq, bg, pseudo, n_iter, S_out, t_out, counts, used,
                     iters, converged);
}

// hs_pssm_refine / hs_pssm_refine_rank (rank given) under sequence weights
hs_status hs_pssm_refine_weighted(hs_handle* h, const double* S0, const double* t, const uint64_t* rank, uint64_t nm,
                                  const uint64_t* id_start, uint64_t n_seq, const double* bg, double pseudo,
                                  uint32_t neff_rule, uint32_t n_iter, double* S_out, double* t_out, uint32_t* counts,
                                  uint64_t* wcounts, uint64_t* wsum, uint32_t* distinct, uint64_t* used,
                                  uint32_t* iters, uint32_t* converged) {
  if (!h || !iters || !converged) return HS_ERR_INVALID;
  *iters = 0;
  *converged = 0;
  if ((t != nullptr) == (rank != nullptr))
    return fail(h, HS_ERR_INVALID, "hs_pssm_refine_weighted: exactly one of t and rank must be given");
  if (neff_rule > 1) return fail(h, HS_ERR_INVALID, "hs_pssm_refine_weighted: neff_rule must be 0 or 1");
  PssmWeightOut wo;
  wo.wcounts = wcounts;
  wo.wsum = wsum;
  wo.distinct = distinct;
  return pssm_refine(h, S0, t, rank, rank != nullptr, nm, id_start, n_seq, bg, pseudo, n_iter, S_out, t_out, counts,
                     used, iters, converged, (int)neff_rule, wo);
}

hs_status hs_pssm_pvalue_dev(hs_handle* h, const double* d_S, const double* d_bg, const double* d_t_lo, uint64_t nm,
                             const uint32_t* d_hit_m, const double* d_hit_score, uint64_t n, double* d_p_hi,
                             double* d_p_lo) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(pssm_null_args(h, d_S, d_bg, n ? nm : 0, "hs_pssm_pvalue"));
  if (n && (!d_hit_m || !d_hit_score || !d_p_hi)) return fail(h, HS_ERR_INVALID, "hs_pssm_pvalue: a hit array or p_hi is null");
  if (!n) return HS_OK;
  if (!nm) return fail(h, HS_ERR_INVALID, "hs_pssm_pvalue: a hit's profile is >= nm");
  HS_CHECK(ensure_device(h));
  HS_CHECK(pssm_null_dev_check(h, d_S, d_bg, d_t_lo, nullptr, nm, d_hit_m, d_hit_score, n, "hs_pssm_pvalue"));
  HS_CHECK(pssm_null_background(h, &d_bg));
  return pssm_null_core(h, d_S, d_bg, d_t_lo, nm, nullptr, d_hit_m, d_hit_score, n, nullptr, d_p_hi, d_p_lo, nullptr);
}

hs_status hs_pssm_pvalue(hs_handle* h, const double* S, const double* bg, const double* t_lo, uint64_t nm,
                         const uint32_t* hit_m, const double* hit_score, uint64_t n, double* p_hi, double* p_lo) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(pssm_null_args(h, S, bg, n ? nm : 0, "hs_pssm_pvalue"));
  if (n && (!hit_m || !hit_score || !p_hi)) return fail(h, HS_ERR_INVALID, "hs_pssm_pvalue: a hit array or p_hi is null");
  if (!n) return HS_OK;
  if (!nm) return fail(h, HS_ERR_INVALID, "hs_pssm_pvalue: a hit's profile is >= nm");
  HS_CHECK(pssm_null_refuse(h, pssm_null_host_bad(h, S, bg, t_lo, nullptr, nm, hit_m, hit_score, n), "hs_pssm_pvalue"));
  HS_CHECK(ensure_device(h));
  // in: t_lo [nm], bg [32], hit_score [n], hit_m [n]; out: p_hi [n], p_lo [n]
  const size_t cb = std::max<size_t>(16, nm * 8), hb = std::max<size_t>(16, n * 8);
  const double* d_bg0 = nullptr;
  if (!bg) HS_CHECK(pssm_null_background(h, &d_bg0));
  HS_CHECK(pssm_stage_in(h, S, nullptr, nm, h->pn_in));
  HS_HIP(h, h->pn_in.reserve(cb + 256 + 2 * hb));
  HS_HIP(h, h->pn_out.reserve(2 * hb));
  char* const in = h->pn_in.as<char>();
  double* const d_t_lo = t_lo ? reinterpret_cast<double*>(in) : nullptr;
  const double* const d_bg = bg ? reinterpret_cast<double*>(in + cb) : d_bg0;
  double* const d_score = reinterpret_cast<double*>(in + cb + 256);
  uint32_t* const d_m = reinterpret_cast<uint32_t*>(in + cb + 256 + hb);
  double* const d_hi = h->pn_out.as<double>();
  double* const d_lo = p_lo ? reinterpret_cast<double*>(h->pn_out.as<char>() + hb) : nullptr;
  if (t_lo) HS_HIP(h, hipMemcpyAsync(d_t_lo, t_lo, nm * 8, hipMemcpyHostToDevice, h->stream));
  if (bg) HS_HIP(h, hipMemcpyAsync(in + cb, bg, (size_t)h->alphabet * 8, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipMemcpyAsync(d_score, hit_score, n * 8, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipMemcpyAsync(d_m, hit_m, n * 4, hipMemcpyHostToDevice, h->stream));
  HS_CHECK(pssm_null_core(h, h->io_centers.as<double>(), d_bg, d_t_lo, nm, nullptr, d_m, d_score, n, nullptr, d_hi, d_lo,
                          nullptr));
  HS_HIP(h, hipMemcpyAsync(p_hi, d_hi, n * 8, hipMemcpyDeviceToHost, h->stream));
  if (p_lo) HS_HIP(h, hipMemcpyAsync(p_lo, d_lo, n * 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

hs_status hs_pssm_pvalue_threshold_dev(hs_handle* h, const double* d_S, const double* d_bg, const double* d_t_lo,
                                       const double* d_p, uint64_t nm, double* d_t_p, double* d_p_hi, double* d_p_lo,
                                       uint32_t* d_flag) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(pssm_null_args(h, d_S, d_bg, nm, "hs_pssm_pvalue_threshold"));
  if (nm && (!d_p || !d_t_p || !d_p_hi || !d_flag))
    return fail(h, HS_ERR_INVALID, "hs_pssm_pvalue_threshold: p, t_p, p_hi or flag is null");
  if (!nm) return HS_OK;
  HS_CHECK(ensure_device(h));
  HS_CHECK(pssm_null_dev_check(h, d_S, d_bg, d_t_lo, d_p, nm, nullptr, nullptr, 0, "hs_pssm_pvalue_threshold"));
  HS_CHECK(pssm_null_background(h, &d_bg));
  return pssm_null_core(h, d_S, d_bg, d_t_lo, nm, d_p, nullptr, nullptr, 0, d_t_p, d_p_hi, d_p_lo, d_flag);
}

hs_status hs_pssm_pvalue_threshold(hs_handle* h, const double* S, const double* bg, const double* t_lo, const double* p,
                                   uint64_t nm, double* t_p, double* p_hi, double* p_lo, uint32_t* flag) {
  if (!h) return HS_ERR_INVALID;
  HS_CHECK(pssm_null_args(h, S, bg, nm, "hs_pssm_pvalue_threshold"));
  if (nm && (!p || !t_p || !p_hi || !flag))
    return fail(h, HS_ERR_INVALID, "hs_pssm_pvalue_threshold: p, t_p, p_hi or flag is null");
  if (!nm) return HS_OK;
  HS_CHECK(pssm_null_refuse(h, pssm_null_host_bad(h, S, bg, t_lo, p, nm, nullptr, nullptr, 0), "hs_pssm_pvalue_threshold"));
  HS_CHECK(ensure_device(h));
  // in: t_lo [nm], p [nm], bg [32]; out: t_p, p_hi, p_lo, flag [nm]: one double, two probabilities and a flag per profile
  const size_t cb = std::max<size_t>(16, nm * 8);
  const double* d_bg0 = nullptr;
  if (!bg) HS_CHECK(pssm_null_background(h, &d_bg0));
  HS_CHECK(pssm_stage_in(h, S, nullptr, nm, h->pn_in));
  HS_HIP(h, h->pn_in.reserve(2 * cb + 256));
  HS_HIP(h, h->pn_out.reserve(4 * cb));
  char *const in = h->pn_in.as<char>(), *const out = h->pn_out.as<char>();
  double* const d_t_lo = t_lo ? reinterpret_cast<double*>(in) : nullptr;
  double* const d_p = reinterpret_cast<double*>(in + cb);
  const double* const d_bg = bg ? reinterpret_cast<double*>(in + 2 * cb) : d_bg0;
  double* const d_tp = reinterpret_cast<double*>(out);
  double* const d_hi = reinterpret_cast<double*>(out + cb);
  double* const d_lo = p_lo ? reinterpret_cast<double*>(out + 2 * cb) : nullptr;
  uint32_t* const d_fl = reinterpret_cast<uint32_t*>(out + 3 * cb);
  if (t_lo) HS_HIP(h, hipMemcpyAsync(d_t_lo, t_lo, nm * 8, hipMemcpyHostToDevice, h->stream));
  HS_HIP(h, hipMemcpyAsync(d_p, p, nm * 8, hipMemcpyHostToDevice, h->stream));
  if (bg) HS_HIP(h, hipMemcpyAsync(in + 2 * cb, bg, (size_t)h->alphabet * 8, hipMemcpyHostToDevice, h->stream));
  HS_CHECK(pssm_null_core(h, h->io_centers.as<double>(), d_bg, d_t_lo, nm, d_p, nullptr, nullptr, 0, d_tp, d_hi, d_lo,
                          d_fl));
  HS_HIP(h, hipMemcpyAsync(t_p, d_tp, nm * 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(p_hi, d_hi, nm * 8, hipMemcpyDeviceToHost, h->stream));
  if (p_lo) HS_HIP(h, hipMemcpyAsync(p_lo, d_lo, nm * 8, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipMemcpyAsync(flag, d_fl, nm * 4, hipMemcpyDeviceToHost, h->stream));
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return HS_OK;
}

// The same rule on the host (hs_pssm_null.h): no GPU, no handle
hs_status hs_pssm_null_tables(const double* S, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                              const double* t_lo, uint32_t bins, uint16_t* q_dn, uint16_t* q_up, double* delta,
                              uint8_t* dead, double* cdf_dn, double* cdf_up) {
  return pssm_null_status(hs_pssm_null_tables_host(S, nm, k, alphabet, bg, t_lo, bins, q_dn, q_up, delta, dead, cdf_dn,
                                                   cdf_up));
}

hs_status hs_pssm_pvalue_host(const double* S, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                              const double* t_lo, uint32_t bins, const uint32_t* hit_m, const double* hit_score,
                              uint64_t n, double* p_hi, double* p_lo) {
  return pssm_null_status(hs_pssm_pvalue_host_rule(S, nm, k, alphabet, bg, t_lo, bins, hit_m, hit_score, n, p_hi, p_lo));
}

hs_status hs_pssm_threshold_host(const double* S, uint64_t nm, uint32_t k, uint32_t alphabet, const double* bg,
                                 const double* t_lo, uint32_t bins, const double* p, double* t_p, double* p_hi,
                                 double* p_lo, uint32_t* flag) {
  return pssm_null_status(hs_pssm_threshold_host_rule(S, nm, k, alphabet, bg, t_lo, bins, p, t_p, p_hi, p_lo, flag));
}

// ---- hs_pssm_compare ---------------------------------------------------------------------------------------------
hs_status hs_pssm_compare_dev(hs_handle* h, const double* d_X, uint64_t nx, const double* d_Y, uint64_t ny,
                              const double* d_t, uint32_t min_overlap, uint32_t* d_hit_x, uint32_t* d_hit_y,
                              int32_t* d_hit_d, double* d_hit_score, uint64_t cap, uint64_t* n_hits, uint64_t* d_cnt) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  HS_CHECK(pcmp_args(h, d_X, nx, d_Y, ny, d_t, min_overlap, d_hit_x, d_hit_y, d_hit_d, d_hit_score, cap));
  HS_CHECK(ensure_device(h));
  if (nx) {  // the value errors: one reduction per array, one read-back, before anything is written
    uint32_t bits[2] = {0, 0};
    const uint64_t ka = (uint64_t)h->p.k * h->alphabet;
    HS_HIP(h, h->sq_chk.reserve(64));
    HS_HIP(h, hipMemsetAsync(h->sq_chk.p, 0, 64, h->stream));
    HS_HIP(h, hs_launch_pssm_check(d_X, nx * ka, d_t, nx, h->sq_chk.as<uint32_t>(), h->stream));
    if (d_Y) HS_HIP(h, hs_launch_pssm_check(d_Y, ny * ka, nullptr, 0, h->sq_chk.as<uint32_t>() + 1, h->stream));
    HS_HIP(h, hipMemcpyAsync(bits, h->sq_chk.p, sizeof(bits), hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    HS_CHECK(pssm_refuse(h, bits[0] | bits[1], "threshold", "hs_pssm_compare"));
  }
  return pcmp_core(h, d_X, nx, d_Y, ny, d_t, min_overlap, d_hit_x, d_hit_y, d_hit_d, d_hit_score, cap, n_hits, d_cnt);
}

hs_status hs_pssm_compare(hs_handle* h, const double* X, uint64_t nx, const double* Y, uint64_t ny, const double* t,
                          uint32_t min_overlap, uint32_t* hit_x, uint32_t* hit_y, int32_t* hit_d, double* hit_score,
                          uint64_t cap, uint64_t* n_hits, uint64_t* cnt) {
  if (!h || !n_hits) return HS_ERR_INVALID;
  *n_hits = 0;
  HS_CHECK(pcmp_args(h, X, nx, Y, ny, t, min_overlap, hit_x, hit_y, hit_d, hit_score, cap));
  const size_t ka = (size_t)h->p.k * h->alphabet;
  uint32_t bad = pssm_host_bad(h, X, t, nx);
  for (uint64_t i = 0; Y && i < ny * ka && !bad; ++i)
    if (hs_pcmp_bad_value(Y[i], HS_PCMP_MAX_ABS)) bad = BAD_S;
  HS_CHECK(pssm_refuse(h, bad, "threshold", "hs_pssm_compare"));
  HS_CHECK(ensure_device(h));
  HS_CHECK(pssm_stage_in(h, X, t, nx, h->io_radii));
  if (Y) {
    HS_HIP(h, h->pcm_y.reserve(std::max<size_t>(16, ny * ka * 8)));
    if (ny) HS_HIP(h, hipMemcpyAsync(h->pcm_y.p, Y, ny * ka * 8, hipMemcpyHostToDevice, h->stream));
  }
  HS_HIP(h, h->io_q.reserve(std::max<size_t>(16, cap * 4)));
  HS_HIP(h, h->io_id.reserve(std::max<size_t>(16, cap * 4)));
  HS_HIP(h, h->io_table.reserve(std::max<size_t>(16, cap * 4)));
  HS_HIP(h, h->io_dist.reserve(std::max<size_t>(16, cap * 8)));
  if (cnt) HS_HIP(h, h->io_cand.reserve(std::max<size_t>(16, nx * 8)));
  const hs_status st = pcmp_core(h, h->io_centers.as<double>(), nx, Y ? h->pcm_y.as<double>() : nullptr, ny,
                                 h->io_radii.as<double>(), min_overlap, h->io_q.as<uint32_t>(), h->io_id.as<uint32_t>(),
                                 h->io_table.as<int32_t>(), h->io_dist.as<double>(), cap, n_hits,
                                 cnt ? h->io_cand.as<uint64_t>() : nullptr);
  if (st != HS_OK && st != HS_ERR_CAPACITY) return st;
  if (cnt && nx) HS_HIP(h, hipMemcpyAsync(cnt, h->io_cand.p, nx * 8, hipMemcpyDeviceToHost, h->stream));
  const uint64_t nh = *n_hits;
  if (st == HS_OK && nh) {
    HS_HIP(h, hipMemcpyAsync(hit_x, h->io_q.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(hit_y, h->io_id.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(hit_d, h->io_table.p, nh * 4, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipMemcpyAsync(hit_score, h->io_dist.p, nh * 8, hipMemcpyDeviceToHost, h->stream));
  }
  HS_HIP(h, hipStreamSynchronize(h->stream));
  return st;
}

// The same rule on the host (hs_pssm_compare.h): no GPU, no handle
hs_status hs_pssm_compare_host(const double* X, uint64_t nx, const double* Y, uint64_t ny, uint32_t k, uint32_t alphabet,
                               const double* t, uint32_t min_overlap, uint32_t* hit_x, uint32_t* hit_y, int32_t* hit_d,
                               double* hit_score, uint64_t cap, uint64_t* n_hits, uint64_t* cnt) {
  if (!n_hits) return HS_ERR_INVALID;
  const int r = hs_pssm_compare_host_rule(X, nx, Y, ny, k, alphabet, t, min_overlap, hit_x, hit_y, hit_d, hit_score, cap,
                                          n_hits, cnt);
  return r == 0 ? HS_OK : r == 1 ? HS_ERR_INVALID : HS_ERR_CAPACITY;
}

hs_status hs_pssm_compare_tables(const double* X, uint64_t nx, uint32_t k, uint32_t alphabet, int8_t* q, double* s,
                                 double* l1, double* amax) {
  if (k < 1 || alphabet < 1 || (nx && !X)) return HS_ERR_INVALID;
  return hs_pssm_compare_tables_host(X, nx, k, alphabet, q, s, l1, amax) ? HS_ERR_INVALID : HS_OK;
}

int hs_pssm_compare_pass(int64_t I, double s_x, double l1_x, double amax_x, double s_y, double l1_y, uint32_t k,
                         uint32_t alphabet, double t) {
  return hs_pcmp_pass(I, s_x, l1_x, amax_x, s_y, l1_y, k * alphabet, t);
}

hs_status hs_pssm_compare_columns(const double* X, uint64_t nm, uint32_t k, uint32_t alphabet, int mode, double* out) {
  return hs_pssm_compare_columns_host(X, nm, k, alphabet, mode, out) ? HS_ERR_INVALID : HS_OK;
}

}  // extern "C"
