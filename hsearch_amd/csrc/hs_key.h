// hs_key.h -- the 64-bit key fingerprints of the tables and the exact HashKey string comparison, for device and
// host code alike (plain C++ too: the host-only entry points and their stand-alone test programs include it).
#ifndef HS_KEY_H
#define HS_KEY_H

#include <stdint.h>

#ifdef __HIPCC__
#define HS_HD __host__ __device__
#else
#define HS_HD
#endif
#ifndef HS_MAX_K
#define HS_MAX_K 32
#endif
#ifndef HS_KEY_CHARS
#define HS_KEY_CHARS (11 * HS_MAX_K + 1)
#endif

// ---- key fingerprints ---------------------------------------------------------------------------
// The reference keys a table by the STRING to_string(b_0)+...+to_string(b_{K-1}) (lsh.hpp:51-59).
// The index keys by a 64-bit fingerprint of exactly that character stream (so tuples whose strings
// alias, e.g. (1,23) and (12,3), share a fingerprint by construction) and verifies string equality
// exactly: at build time for every sorted neighbour pair, at probe time against the bucket's tuple.
HS_HD inline uint64_t hs_key_init(uint32_t seed) {
  return 0xcbf29ce484222325ull ^ ((uint64_t)(seed + 1) * 0x9e3779b97f4a7c15ull);
}
HS_HD inline uint64_t hs_key_put(uint64_t h, uint32_t ch) {
  return (h ^ ch) * 0x100000001b3ull;
}
HS_HD inline uint64_t hs_key_put_int(uint64_t h, int32_t v) {
  // the decimal characters of v, most significant first (std::to_string, lsh.hpp:51-59); divisions
  // by constants only, short numbers (the usual bucket ints) first
  uint32_t m;
  if (v < 0) {
    h = hs_key_put(h, '-');
    m = 0u - (uint32_t)v;
  } else {
    m = (uint32_t)v;
  }
  if (m < 10u) return hs_key_put(h, '0' + m);
  if (m < 100u) {
    const uint32_t q = m / 10u;
    h = hs_key_put(h, '0' + q);
    return hs_key_put(h, '0' + (m - 10u * q));
  }
  bool started = false;
#define HS_DIGIT(P)                            \
  {                                            \
    const uint32_t dgt = (m / (P)) % 10u;      \
    started = started || dgt != 0u;            \
    if (started) h = hs_key_put(h, '0' + dgt); \
  }
  HS_DIGIT(1000000000u) HS_DIGIT(100000000u) HS_DIGIT(10000000u) HS_DIGIT(1000000u) HS_DIGIT(100000u)
  HS_DIGIT(10000u) HS_DIGIT(1000u) HS_DIGIT(100u) HS_DIGIT(10u) HS_DIGIT(1u)
#undef HS_DIGIT
  return h;
}
HS_HD inline uint64_t hs_key_fin(uint64_t h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}
HS_HD inline uint64_t hs_key_of(const int32_t* t, int K, uint32_t seed) {
  uint64_t h = hs_key_init(seed);
  for (int i = 0; i < K; ++i) h = hs_key_put_int(h, t[i]);
  return hs_key_fin(h);
}
// Decimal characters of the concatenation; returns the length.
HS_HD inline int hs_key_chars(const int32_t* t, int K, char* out) {
  int n = 0;
  for (int i = 0; i < K; ++i) {
    int32_t v = t[i];
    uint32_t m;
    if (v < 0) {
      out[n++] = '-';
      m = 0u - (uint32_t)v;
    } else {
      m = (uint32_t)v;
    }
    uint32_t p = 1;
    while (m / p >= 10) p *= 10;
    while (p) {
      uint32_t dgt = m / p;
      out[n++] = (char)('0' + dgt);
      m -= dgt * p;
      p /= 10;
    }
  }
  return n;
}
// HashKey string equality of two K-tuples (fast path: identical tuples).
HS_HD inline bool hs_key_equal(const int32_t* x, const int32_t* y, int K) {
  bool same = true;
  for (int i = 0; i < K; ++i) same = same && (x[i] == y[i]);
  if (same) return true;
  char sx[HS_KEY_CHARS], sy[HS_KEY_CHARS];
  int nx = hs_key_chars(x, K, sx), ny = hs_key_chars(y, K, sy);
  if (nx != ny) return false;
  for (int i = 0; i < nx; ++i)
    if (sx[i] != sy[i]) return false;
  return true;
}

#endif
