// AddressSanitizer + UBSan driver of csrc/host_columns.hpp alone (tests/test_host_columns_sanitize.py builds and runs it): the
// gather of a trace held as separate columns over every (word0, len) of a small matrix, every buffer allocated at its exact size so
// that one word read or written past an end is a report, and the host reduction.
#include "host_columns.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sbn;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static uint64_t value(size_t c, size_t r) { return 0x9E3779B97F4A7C15ull * (c * 1000 + r + 1); }

// every range of the [ncols][n] matrix `m`, whose column c holds value(ids[c], r)
static void sweep(const HostColumns& m, const std::vector<size_t>& ids, size_t n) {
  const size_t words = ids.size() * n;
  for (size_t word0 = 0; word0 <= words; word0++)
    for (size_t len = 0; word0 + len <= words; len++) {
      uint64_t* out = len ? (uint64_t*)malloc(len * sizeof(uint64_t)) : nullptr;   // exact size; len = 0 must not touch it
      gather_columns(m, word0, len, out);
      for (size_t i = 0; i < len; i++) {
        const size_t w = word0 + i;
        if (out[i] != value(ids[w / n], w % n)) { EXPECT(!"gathered word differs"); i = len; }
      }
      free(out);
    }
}

int main() {
  const size_t n = 8, ncols = 5;
  // each column its own allocation, allocated in another order than the table's
  std::vector<uint64_t*> own(ncols);
  for (size_t c : {3u, 0u, 4u, 1u, 2u}) { own[c] = (uint64_t*)malloc(n * sizeof(uint64_t)); for (size_t r = 0; r < n; r++) own[c][r] = value(c, r); }
  std::vector<const uint64_t*> cols(own.begin(), own.end());
  std::vector<size_t> ids = {0, 1, 2, 3, 4};
  sweep(HostColumns{cols.data(), nullptr, n}, ids, n);
  EXPECT(gather_columns_refused(cols.data(), ncols, n, 0, 40) == 0);
  EXPECT(gather_columns_refused(cols.data(), ncols, n, 40, 0) == 0);
  EXPECT(gather_columns_refused(cols.data(), ncols, n, 40, 1) == 1);
  EXPECT(gather_columns_refused(cols.data(), ncols, n, 41, 0) == 1);
  EXPECT(gather_columns_refused(cols.data(), ncols, n, 1, (size_t)-1) == 1);
  EXPECT(gather_columns_refused(cols.data(), (size_t)-1, n, 0, 1) == 1);

  // a column at an odd 8-byte offset of a larger buffer, ending at the buffer's end
  uint64_t* big = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
  for (size_t r = 0; r < n; r++) big[1 + r] = value(7, r);
  std::vector<const uint64_t*> cols2 = cols; cols2[2] = big + 1;
  sweep(HostColumns{cols2.data(), nullptr, n}, {0, 1, 7, 3, 4}, n);
  EXPECT(gather_columns_refused(cols2.data(), ncols, n, 0, 40) == 0);

  // two entries are the same pointer
  std::vector<const uint64_t*> cols3 = cols; cols3[4] = cols3[1];
  sweep(HostColumns{cols3.data(), nullptr, n}, {0, 1, 2, 3, 1}, n);

  // a null and a misaligned entry are named
  std::vector<const uint64_t*> cols4 = cols; cols4[3] = nullptr;
  EXPECT(gather_columns_refused(cols4.data(), ncols, n, 0, 0) == 2 + 3);
  cols4[3] = cols[3]; cols4[1] = (const uint64_t*)((const char*)cols[1] + 4);
  EXPECT(gather_columns_refused(cols4.data(), ncols, n, 0, 0) == 2 + 1);
  EXPECT(gather_columns_refused(nullptr, ncols, n, 0, 0) == 2);

  // the flat matrix: columns n words apart in one allocation
  uint64_t* flat = (uint64_t*)malloc(ncols * n * sizeof(uint64_t));
  for (size_t c = 0; c < ncols; c++) for (size_t r = 0; r < n; r++) flat[c * n + r] = value(c, r);
  sweep(HostColumns{nullptr, flat, n}, ids, n);

  // the host reduction: 0, p - 1, p, p + 1, 2^64 - 1 at counts 0, 1, 2, 3, 1025
  const uint64_t p = 0xFFFFFFFF00000001ull, pat[5] = {0, p - 1, p, p + 1, ~0ull}, red[5] = {0, p - 1, 0, 1, 0xFFFFFFFEull};
  for (size_t count : {0u, 1u, 2u, 3u, 1025u})
    for (size_t shift = 0; shift < 5; shift++) {
      uint64_t* w = count ? (uint64_t*)malloc(count * sizeof(uint64_t)) : nullptr;
      uint64_t want = 0;
      for (size_t i = 0; i < count; i++) { w[i] = pat[(i + shift) % 5]; want += w[i] >= p; }
      EXPECT(reduce_words_host(w, count) == want);
      for (size_t i = 0; i < count; i++) EXPECT(w[i] == red[(i + shift) % 5]);
      free(w);
    }

  for (uint64_t* q : own) free(q);
  free(big); free(flat);
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("host columns: gather sweep and reduction ok\n");
  return 0;
}
