// Stand-alone driver of hs_table_append_host (hsearch_amd/csrc/hs_table_append.h) for the sanitizer run of
// tests/test_index_append_cpu.py: g++ -fsanitize=address,undefined, no GPU, no library.  Tables are built here
// by sorting (fingerprint, id) pairs; an append must give the table built over the concatenation, with output
// arrays of EXACTLY the needed size (so that any write past them is a report).  Exit status 0 = all cases held.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../hsearch_amd/csrc/hs_table_append.h"

struct Table {
  std::vector<uint32_t> ids, start;
  std::vector<uint64_t> key;
  std::vector<int32_t> tuple;
};

static Table build(const std::vector<int32_t>& ints, uint32_t K, uint32_t seed) {
  const size_t n = ints.size() / K;
  std::vector<uint64_t> fp(n);
  for (size_t i = 0; i < n; ++i) fp[i] = hs_key_of(&ints[i * K], (int)K, seed);
  Table t;
  t.ids.resize(n);
  for (size_t i = 0; i < n; ++i) t.ids[i] = (uint32_t)i;
  std::sort(t.ids.begin(), t.ids.end(), [&](uint32_t x, uint32_t y) { return fp[x] != fp[y] ? fp[x] < fp[y] : x < y; });
  for (size_t i = 0; i < n; ++i)
    if (!i || fp[t.ids[i]] != fp[t.ids[i - 1]]) {
      t.key.push_back(fp[t.ids[i]]);
      t.start.push_back((uint32_t)i);
      t.tuple.insert(t.tuple.end(), &ints[(size_t)t.ids[i] * K], &ints[(size_t)t.ids[i] * K] + K);
    }
  t.start.push_back((uint32_t)n);
  return t;
}

static int failures = 0;
#define EXPECT(c)                                                      \
  do {                                                                 \
    if (!(c)) {                                                        \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #c);    \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

// status of the sized call; on success the outputs are compared with `want`
static int append(const Table& a, const std::vector<int32_t>& blk, uint32_t K, uint32_t seed, const Table* want,
                  uint32_t* collided) {
  const uint64_t n = a.ids.size(), nb = a.key.size(), m = blk.size() / K;
  uint64_t nb_out = 0;
  int st = hs_table_append_host(a.ids.data(), a.key.data(), a.start.data(), a.tuple.data(), n, nb, blk.data(), m, K, seed,
                                nullptr, nullptr, nullptr, nullptr, 0, &nb_out, collided);
  if (st != 0 && st != 4) return st;
  if (*collided) return 0;
  EXPECT(nb_out <= nb + m);
  std::vector<uint32_t> oi(n + m), os(nb_out + 1);
  std::vector<uint64_t> ok(nb_out);
  std::vector<int32_t> ot(nb_out * K);
  if (nb_out) {  // one bucket too few: nothing may be written
    uint64_t nb2 = 0;
    EXPECT(hs_table_append_host(a.ids.data(), a.key.data(), a.start.data(), a.tuple.data(), n, nb, blk.data(), m, K, seed,
                                oi.data(), ok.data(), os.data(), ot.data(), nb_out - 1, &nb2, collided) == 4);
    EXPECT(nb2 == nb_out);
  }
  st = hs_table_append_host(a.ids.data(), a.key.data(), a.start.data(), a.tuple.data(), n, nb, blk.data(), m, K, seed,
                            oi.data(), ok.data(), os.data(), ot.data(), nb_out, &nb_out, collided);
  if (st == 0 && want) {
    EXPECT(oi == want->ids);
    EXPECT(ok == want->key);
    EXPECT(os == want->start);
    EXPECT(ot == want->tuple);
  }
  return st;
}

int main() {
  const uint32_t K = 3, seed = 1;
  srand(7);
  auto draw = [&](size_t n, int spread, int offset) {
    std::vector<int32_t> v(n * K);
    for (auto& x : v) x = offset + rand() % spread - spread / 2;
    return v;
  };
  auto cat = [](std::vector<int32_t> x, const std::vector<int32_t>& y) {
    x.insert(x.end(), y.begin(), y.end());
    return x;
  };
  uint32_t col = 0;
  const std::vector<int32_t> A = draw(500, 5, 0), none;
  const Table ta = build(A, K, seed);
  for (int spread : {2, 5, 40}) {  // few new buckets ... nearly all new
    for (size_t m : {(size_t)1, (size_t)63, (size_t)700}) {
      const std::vector<int32_t> B = draw(m, spread, 0);
      const Table want = build(cat(A, B), K, seed);
      EXPECT(append(ta, B, K, seed, &want, &col) == 0 && !col);
    }
  }
  EXPECT(append(ta, none, K, seed, &ta, &col) == 0 && !col);                  // empty block
  {                                                                             // empty table
    const Table empty = build(none, K, seed), want = build(A, K, seed);
    EXPECT(append(empty, A, K, seed, &want, &col) == 0 && !col);
  }
  {                                                                             // the block = the table
    const Table want = build(cat(A, A), K, seed);
    EXPECT(append(ta, A, K, seed, &want, &col) == 0 && !col);
    EXPECT(want.key.size() == ta.key.size());
  }
  {  // aliased strings share a bucket: (1, 23, 0) and (12, 3, 0) are the string "1230" both
    const std::vector<int32_t> one = {1, 23, 0}, two = {12, 3, 0};
    const Table t1 = build(one, K, seed), want = build(cat(one, two), K, seed);
    EXPECT(want.key.size() == 1);
    EXPECT(append(t1, two, K, seed, &want, &col) == 0 && !col);
  }
  {  // a forged collision: an old key edited to a block tuple's fingerprint, under other ints
    const std::vector<int32_t> B = {1000, 1000, 1000};
    const uint64_t f = hs_key_of(B.data(), (int)K, seed);
    Table forged = ta;
    const size_t r = (size_t)(std::lower_bound(forged.key.begin(), forged.key.end(), f) - forged.key.begin());
    forged.key[r < forged.key.size() ? r : r - 1] = f;
    EXPECT(append(forged, B, K, seed, nullptr, &col) == 0 && col == 1);
  }
  {  // invalid tables
    Table bad = ta;
    std::swap(bad.ids[0], bad.ids[bad.ids.size() - 1]);  // ids no longer ascend inside their buckets
    bad.ids[1] = bad.ids[0];
    EXPECT(append(bad, draw(5, 5, 0), K, seed, nullptr, &col) == 1);
    bad = ta;
    bad.start[1] = bad.start[0];
    EXPECT(append(bad, draw(5, 5, 0), K, seed, nullptr, &col) == 1);
    bad = ta;
    bad.tuple[0] += 1;  // the tuple no longer has the bucket's fingerprint
    EXPECT(append(bad, draw(5, 5, 100), K, seed, nullptr, &col) == 1);
    bad = ta;
    bad.ids[3] = (uint32_t)bad.ids.size();
    EXPECT(append(bad, draw(5, 5, 0), K, seed, nullptr, &col) == 1);
  }
  if (failures) return 1;
  printf("index_table_append_san ok\n");
  return 0;
}
