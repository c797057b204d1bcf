// Stand-alone driver of hsearch_amd/csrc/hs_pssm_seq.h for the sanitizer run of tests/test_pssm_seq_cpu.py: the host
// rule on shuffled tuple lists with ties and repeats, over id_start arrays with empty sequences at the start, in the
// middle and at the end and with one sequence, the capacity protocol and the refused inputs -- against a plain loop
// over (profile, sequence) slots.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../hsearch_amd/csrc/hs_pssm_seq.h"

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #c);           \
      return 1;                                               \
    }                                                         \
  } while (0)

struct Rows {
  std::vector<uint32_t> m, seq, count, best_id, lo, hi;
  std::vector<double> best_score;
  explicit Rows(size_t cap, uint32_t fill = 9)
      : m(cap, fill), seq(cap, fill), count(cap, fill), best_id(cap, fill), lo(cap, fill), hi(cap, fill),
        best_score(cap, 9.0) {}
  bool untouched() const {
    for (size_t i = 0; i < m.size(); ++i)
      if (m[i] != 9 || seq[i] != 9 || count[i] != 9 || best_id[i] != 9 || lo[i] != 9 || hi[i] != 9 || best_score[i] != 9.0)
        return false;
    return true;
  }
};

static int call(const std::vector<uint32_t>& m, const std::vector<uint32_t>& id, const std::vector<double>& sc,
                uint64_t nm, const std::vector<uint64_t>& id_start, Rows& r, uint64_t cap, uint64_t* n_out) {
  return hs_pssm_seq_hits_host(m.data(), id.data(), sc.data(), m.size(), nm, id_start.data(), id_start.size() - 1,
                               r.m.data(), r.seq.data(), r.count.data(), r.best_score.data(), r.best_id.data(),
                               r.lo.data(), r.hi.data(), cap, n_out);
}

int main() {
  std::mt19937_64 rng(23);
  const std::vector<std::vector<uint64_t>> layouts = {
      {0, 0, 0, 5, 5, 5, 12, 40, 40, 41, 60, 60, 60},  // empty sequences at the start, in the middle and at the end
      {0, 60},                                         // one sequence
      {0, 1, 2, 3, 60},
      {0, 0, 60, 60}};
  for (int round = 0; round < 60; ++round) {
    const std::vector<uint64_t>& id_start = layouts[round % layouts.size()];
    const uint64_t n_seq = id_start.size() - 1, n = id_start[n_seq];
    const uint64_t nm = 1 + rng() % 4;
    const size_t nt = rng() % 500;
    std::vector<uint32_t> m(nt), id(nt);
    std::vector<double> sc(nt);
    for (size_t i = 0; i < nt; ++i) {
      m[i] = (uint32_t)(rng() % nm);
      id[i] = (uint32_t)(rng() % n);
      sc[i] = (double)((int)((id[i] * 7u + m[i] * 3u) % 5u) - 2);  // a function of (m, id): repeats agree; heavy ties
    }
    // the rows by a plain loop over the slots
    std::vector<uint32_t> wm, wseq, wcount, wid, wlo, whi;
    std::vector<double> wsc;
    for (uint64_t mm = 0; mm < nm; ++mm)
      for (uint64_t s = 0; s < n_seq; ++s) {
        std::vector<uint8_t> seen(n, 0);
        uint32_t count = 0, best = 0, lo = 0, hi = 0;
        double bs = 0;
        for (uint64_t x = id_start[s]; x < id_start[s + 1]; ++x)
          for (size_t i = 0; i < nt; ++i)
            if (m[i] == mm && id[i] == x && !seen[x]) {
              seen[x] = 1;
              if (!count || sc[i] > bs) {
                bs = sc[i];
                best = (uint32_t)x;
              }
              if (!count) lo = (uint32_t)(x - id_start[s]);
              hi = (uint32_t)(x - id_start[s]);
              ++count;
            }
        if (count) {
          wm.push_back((uint32_t)mm);
          wseq.push_back((uint32_t)s);
          wcount.push_back(count);
          wid.push_back(best);
          wsc.push_back(bs);
          wlo.push_back(lo);
          whi.push_back(hi);
        }
      }
    uint64_t n_out = 77;
    Rows none(4);
    CHECK(hs_pssm_seq_hits_host(m.data(), id.data(), sc.data(), nt, nm, id_start.data(), n_seq, nullptr, nullptr,
                                nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n_out) == (wm.empty() ? 0 : 3));
    CHECK(n_out == wm.size());
    if (wm.size() > 1) {  // one row short: the count, and nothing written
      Rows few(wm.size() - 1);
      CHECK(call(m, id, sc, nm, id_start, few, wm.size() - 1, &n_out) == 3 && n_out == wm.size() && few.untouched());
    }
    Rows r(wm.size() + 2);
    CHECK(call(m, id, sc, nm, id_start, r, wm.size() + 2, &n_out) == 0 && n_out == wm.size());
    for (size_t i = 0; i < wm.size(); ++i) {
      CHECK(r.m[i] == wm[i] && r.seq[i] == wseq[i] && r.count[i] == wcount[i] && r.best_id[i] == wid[i]);
      CHECK(r.best_score[i] == wsc[i] && !(r.best_score[i] == 0.0 && signbit(r.best_score[i])));
      CHECK(r.lo[i] == wlo[i] && r.hi[i] == whi[i]);
    }
    CHECK(r.m[wm.size()] == 9 && r.best_score[wm.size() + 1] == 9.0);
  }
  // refusals: nothing is written
  {
    const std::vector<uint64_t> id_start = {0, 3, 10};
    std::vector<uint32_t> m = {0, 0, 1}, id = {4, 4, 2};
    std::vector<double> sc = {1.0, 2.0, 0.5};
    Rows r(4);
    uint64_t n_out = 5;
    CHECK(call(m, id, sc, 2, id_start, r, 4, &n_out) == 1 && n_out == 0);  // two scores for (0, 4)
    sc[1] = 1.0;
    CHECK(call(m, id, sc, 1, id_start, r, 4, &n_out) == 1);                // m >= nm
    CHECK(call(m, id, sc, 2, {0, 3, 4}, r, 4, &n_out) == 1);               // an id at id_start[n_seq]
    CHECK(call(m, id, sc, 2, {1, 3, 10}, r, 4, &n_out) == 1);              // id_start[0] != 0
    CHECK(call(m, id, sc, 2, {0, 11, 10}, r, 4, &n_out) == 1);             // descending
    CHECK(call(m, id, sc, 2, {0}, r, 4, &n_out) == 1);                     // no sequence owns the ids
    CHECK(hs_pssm_seq_hits_host(m.data(), id.data(), sc.data(), 3, 2, nullptr, 2, r.m.data(), r.seq.data(),
                                r.count.data(), r.best_score.data(), r.best_id.data(), r.lo.data(), r.hi.data(), 4,
                                &n_out) == 1);
    CHECK(hs_pssm_seq_hits_host(m.data(), id.data(), sc.data(), 3, 2, id_start.data(), 2, nullptr, r.seq.data(),
                                r.count.data(), r.best_score.data(), r.best_id.data(), r.lo.data(), r.hi.data(), 4,
                                &n_out) == 1);
    CHECK(hs_pssm_seq_hits_host(m.data(), id.data(), sc.data(), 3, 2, id_start.data(), 2, r.m.data(), r.seq.data(),
                                r.count.data(), r.best_score.data(), r.best_id.data(), r.lo.data(), r.hi.data(), 4,
                                nullptr) == 1);
    sc[2] = NAN;
    CHECK(call(m, id, sc, 2, id_start, r, 4, &n_out) == 1);
    CHECK(r.untouched());
    sc[2] = -0.0;
    CHECK(call(m, id, sc, 2, id_start, r, 4, &n_out) == 0 && n_out == 2);
    CHECK(r.m[0] == 0 && r.seq[0] == 1 && r.count[0] == 1 && r.best_id[0] == 4 && r.lo[0] == 1 && r.hi[0] == 1);
    CHECK(r.m[1] == 1 && r.seq[1] == 0 && r.best_id[1] == 2 && r.lo[1] == 2 && !signbit(r.best_score[1]));
    // no tuples and no sequences: an empty, successful call
    const uint64_t zero = 0;
    CHECK(hs_pssm_seq_hits_host(nullptr, nullptr, nullptr, 0, 0, &zero, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, 0, &n_out) == 0 && n_out == 0);
  }
  printf("pssm_seq_san ok\n");
  return 0;
}
