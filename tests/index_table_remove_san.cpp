// Stand-alone driver of hs_table_remove_host (hsearch_amd/csrc/hs_table_remove.h) for the sanitizer run of
// tests/test_index_remove_cpu.py: g++ -fsanitize=address,undefined, no GPU, no library.  Tables are built here by
// sorting (fingerprint, id) pairs; a removal must give the table built over the surviving rows, with output arrays
// of EXACTLY the needed size (so that any write past them is a report).  Exit status 0 = all cases held.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../hsearch_amd/csrc/hs_table_remove.h"

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

static std::vector<int32_t> rows_without(const std::vector<int32_t>& ints, uint32_t K, const std::vector<uint32_t>& dead) {
  const size_t n = ints.size() / K;
  std::vector<char> gone(n, 0);
  for (uint32_t d : dead)
    if (d < n) gone[d] = 1;
  std::vector<int32_t> out;
  for (size_t i = 0; i < n; ++i)
    if (!gone[i]) out.insert(out.end(), &ints[i * K], &ints[i * K] + K);
  return out;
}

// status of the sized call; on success the outputs are compared with the table built over the survivors
static int remove_ids(const Table& a, const std::vector<int32_t>& ints, const std::vector<uint32_t>& dead, uint32_t K,
                      uint32_t seed, bool compare) {
  const uint64_t n = a.ids.size(), nb = a.key.size();
  uint64_t n_out = 0, nb_out = 0;
  int st = hs_table_remove_host(a.ids.data(), a.key.data(), a.start.data(), a.tuple.data(), n, nb, dead.data(),
                                dead.size(), ints.data(), K, seed, nullptr, nullptr, nullptr, nullptr, 0, &n_out, &nb_out);
  if (st != 0 && st != 4) return st;
  EXPECT(nb_out <= nb && n_out <= n);
  std::vector<uint32_t> oi(n_out), os(nb_out + 1);
  std::vector<uint64_t> ok(nb_out);
  std::vector<int32_t> ot(nb_out * K);
  if (nb_out) {  // one bucket too few: nothing may be written
    uint64_t n2 = 0, nb2 = 0;
    EXPECT(hs_table_remove_host(a.ids.data(), a.key.data(), a.start.data(), a.tuple.data(), n, nb, dead.data(),
                                dead.size(), ints.data(), K, seed, oi.data(), ok.data(), os.data(), ot.data(),
                                nb_out - 1, &n2, &nb2) == 4);
    EXPECT(nb2 == nb_out && n2 == n_out);
  }
  st = hs_table_remove_host(a.ids.data(), a.key.data(), a.start.data(), a.tuple.data(), n, nb, dead.data(), dead.size(),
                            ints.data(), K, seed, oi.data(), ok.data(), os.data(), ot.data(), nb_out, &n_out, &nb_out);
  if (st == 0 && compare) {
    const Table want = build(rows_without(ints, K, dead), K, seed);
    EXPECT(oi == want.ids);
    EXPECT(ok == want.key);
    EXPECT(os == want.start);
    EXPECT(ot == want.tuple);
  }
  return st;
}

int main() {
  const uint32_t K = 3, seed = 1;
  srand(7);
  auto draw = [&](size_t n, int spread) {
    std::vector<int32_t> v(n * K);
    for (auto& x : v) x = rand() % spread - spread / 2;
    return v;
  };
  for (int spread : {2, 5, 40}) {  // few large buckets ... nearly all singletons
    const std::vector<int32_t> A = draw(500, spread);
    const Table ta = build(A, K, seed);
    for (size_t m : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)300, (size_t)499, (size_t)500}) {
      std::vector<uint32_t> dead(500);
      for (size_t i = 0; i < 500; ++i) dead[i] = (uint32_t)i;
      for (size_t i = 499; i > 0; --i) std::swap(dead[i], dead[(size_t)rand() % (i + 1)]);
      dead.resize(m);
      EXPECT(remove_ids(ta, A, dead, K, seed, true) == 0);
      dead.insert(dead.end(), dead.begin(), dead.begin() + m / 2);  // duplicates
      EXPECT(remove_ids(ta, A, dead, K, seed, true) == 0);
    }
    // a whole bucket, and all of it but its last member
    const uint32_t b = (uint32_t)(ta.key.size() / 2);
    std::vector<uint32_t> members(ta.ids.begin() + ta.start[b], ta.ids.begin() + ta.start[b + 1]);
    EXPECT(remove_ids(ta, A, members, K, seed, true) == 0);
    members.pop_back();
    EXPECT(remove_ids(ta, A, members, K, seed, true) == 0);
    EXPECT(remove_ids(ta, A, {500u}, K, seed, false) == 1);  // an id outside the table
    EXPECT(remove_ids(ta, A, {3u, 0xffffffffu}, K, seed, false) == 1);
  }
  {  // aliased strings share a bucket: (1, 23, 0) and (12, 3, 0) are the string "1230" both; the tuple follows the
     // first member
    const std::vector<int32_t> both = {1, 23, 0, 12, 3, 0, 12, 3, 0};
    const Table t = build(both, K, seed);
    EXPECT(t.key.size() == 1 && t.tuple[0] == 1);
    EXPECT(remove_ids(t, both, {0u}, K, seed, true) == 0);
    EXPECT(remove_ids(t, both, {1u}, K, seed, true) == 0);
    EXPECT(remove_ids(t, both, {0u, 1u, 2u}, K, seed, true) == 0);
  }
  {  // an empty table
    const std::vector<int32_t> none;
    const Table empty = build(none, K, seed);
    EXPECT(remove_ids(empty, none, {}, K, seed, true) == 0);
    EXPECT(remove_ids(empty, none, {0u}, K, seed, false) == 1);
  }
  {  // invalid tables
    const std::vector<int32_t> A = draw(500, 5);
    const Table ta = build(A, K, seed);
    const std::vector<uint32_t> dead = {1u, 2u, 3u};
    Table bad = ta;
    std::swap(bad.ids[0], bad.ids[bad.ids.size() - 1]);  // ids no longer ascend inside their buckets
    bad.ids[1] = bad.ids[0];
    EXPECT(remove_ids(bad, A, dead, K, seed, false) == 1);
    bad = ta;
    bad.start[1] = bad.start[0];
    EXPECT(remove_ids(bad, A, dead, K, seed, false) == 1);
    bad = ta;
    bad.tuple[0] += 1;  // the tuple no longer has the bucket's fingerprint
    EXPECT(remove_ids(bad, A, dead, K, seed, false) == 1);
    bad = ta;
    bad.ids[3] = (uint32_t)bad.ids.size();
    EXPECT(remove_ids(bad, A, dead, K, seed, false) == 1);
  }
  if (failures) return 1;
  printf("index_table_remove_san ok\n");
  return 0;
}
