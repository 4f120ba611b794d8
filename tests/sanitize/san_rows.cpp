// AddressSanitizer + UBSan driver of csrc/host_rows.hpp alone (tests/test_host_rows_sanitize.py builds and runs it): the packing
// copy of a row-major trace over every piece cut of a 7 x 5 matrix, from the flat form (packed and with a stride of 8) and from the
// pointer form, every buffer allocated at its exact size so that one word read or written past an end is a report; and the
// refusal helper.
#include "host_rows.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sbn;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const size_t N = 7, C = 5;
static uint64_t value(size_t r, size_t c) { return 0x9E3779B97F4A7C15ull * (r * 1000 + c + 1); }

// every cut of the row range into pieces of `per` whole rows (per = 1 .. N + 1: seven pieces, ragged last pieces, one piece), every
// piece into a buffer of exactly its size; and every single range [r0, r1) on top, the empty ones with a null destination
static void sweep(const HostRows& m) {
  for (size_t slot = 1; slot <= (N + 1) * C; slot++) {   // ring slots of any word count: whole rows only, zero rows when none fits
    const size_t per = rows_per_piece(N, C, slot);
    EXPECT(per == (slot / C < N ? slot / C : N));
    size_t covered = 0, r0 = 0, r1 = 0, k = 0;
    for (; piece_rows(N, per, k, &r0, &r1); k++) {
      EXPECT(r0 == covered && r1 > r0 && r1 - r0 <= per && r1 <= N);
      uint64_t* out = (uint64_t*)malloc((r1 - r0) * C * sizeof(uint64_t));
      copy_rows(m, r0, r1, out);
      for (size_t r = r0; r < r1; r++) for (size_t c = 0; c < C; c++) if (out[(r - r0) * C + c] != value(r, c)) { EXPECT(!"packed word differs"); c = C; r = r1 - 1; }
      free(out);
      covered = r1;
    }
    EXPECT(per == 0 ? k == 0 : (covered == N && k == (N + per - 1) / per));
    EXPECT(!piece_rows(N, per, k + 1, &r0, &r1) && !piece_rows(N, per, (size_t)-1, &r0, &r1));
  }
  for (size_t r0 = 0; r0 <= N; r0++)
    for (size_t r1 = r0; r1 <= N; r1++) {
      uint64_t* out = r1 > r0 ? (uint64_t*)malloc((r1 - r0) * C * sizeof(uint64_t)) : nullptr;   // an empty range must not touch it
      copy_rows(m, r0, r1, out);
      for (size_t r = r0; r < r1; r++) for (size_t c = 0; c < C; c++) if (out[(r - r0) * C + c] != value(r, c)) { EXPECT(!"packed word differs"); c = C; r = r1 - 1; }
      free(out);
    }
}

int main() {
  // the flat form, packed: exactly N * C words
  uint64_t* flat = (uint64_t*)malloc(N * C * sizeof(uint64_t));
  for (size_t r = 0; r < N; r++) for (size_t c = 0; c < C; c++) flat[r * C + c] = value(r, c);
  const HostRows packed{flat, C, nullptr, N, C};
  EXPECT(host_rows_refused(packed) == 0);
  sweep(packed);

  // the flat form with a stride of 8: the allocation ends with the last row's last WORD (N - 1 strides and one row), so a copy that
  // took the padding of the last row along would read past the end; the padding in between holds words no trace may hold
  const size_t S = 8;
  uint64_t* wide = (uint64_t*)malloc(((N - 1) * S + C) * sizeof(uint64_t));
  for (size_t i = 0; i < (N - 1) * S + C; i++) wide[i] = ~0ull;
  for (size_t r = 0; r < N; r++) for (size_t c = 0; c < C; c++) wide[r * S + c] = value(r, c);
  const HostRows strided{wide, S, nullptr, N, C};
  EXPECT(host_rows_refused(strided) == 0);
  sweep(strided);

  // the pointer form: one allocation of exactly C words per row, allocated in another order than the table's
  std::vector<uint64_t*> own(N);
  for (size_t r : {4u, 0u, 6u, 2u, 1u, 5u, 3u}) { own[r] = (uint64_t*)malloc(C * sizeof(uint64_t)); for (size_t c = 0; c < C; c++) own[r][c] = value(r, c); }
  std::vector<const uint64_t*> ptrs(own.begin(), own.end());
  const HostRows table{nullptr, 0, ptrs.data(), N, C};
  EXPECT(host_rows_refused(table) == 0);
  sweep(table);

  // the refusals: both or neither form, a short stride, an overflowing extent, null and misaligned pointers named by their row
  EXPECT(host_rows_refused(HostRows{flat, C, ptrs.data(), N, C}) == 1);
  EXPECT(host_rows_refused(HostRows{nullptr, C, nullptr, N, C}) == 1);
  EXPECT(host_rows_refused(HostRows{flat, C - 1, nullptr, N, C}) == 2);
  EXPECT(host_rows_refused(HostRows{flat, (size_t)-1 / 16, nullptr, N, C}) == 2);
  EXPECT(host_rows_refused(HostRows{(const uint64_t*)((const char*)flat + 4), C, nullptr, N, C}) == 3);
  std::vector<const uint64_t*> bad = ptrs; bad[5] = nullptr;
  EXPECT(host_rows_refused(HostRows{nullptr, 0, bad.data(), N, C}) == 3 + 5);
  bad = ptrs; bad[6] = (const uint64_t*)((const char*)ptrs[6] + 2);
  EXPECT(host_rows_refused(HostRows{nullptr, 0, bad.data(), N, C}) == 3 + 6);
  EXPECT(host_rows_refused(HostRows{nullptr, 0, ptrs.data(), 0, C}) == 0);   // no row: no pointer is looked at
  EXPECT(rows_per_piece(N, 0, 16) == N);

  for (uint64_t* q : own) free(q);
  free(flat); free(wide);
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("host rows: piece cuts, both source forms and refusals ok\n");
  return 0;
}
