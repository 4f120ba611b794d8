// A host trace held as separate columns (include/sbn.h sbn_prover_prove_host_columns): the reference's
// `Vec<PolynomialValues<F>>`, one allocation per table column.  The upload of prove_host_trace reads the caller's memory through
// gather_columns below, piece by piece into its pinned ring, so no flat copy of the trace is ever made; the flat matrix of
// sbn_prover_prove_host_trace is the case whose columns lie n words apart.  Plain C++ (no HIP): tests/sanitize/san_columns.cpp
// includes this header alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace sbn {

// The virtual column-major matrix [n_columns][n]: column c is cols[c][0 .. n), or flat[c * n .. c * n + n) when cols is null.
struct HostColumns {
  const uint64_t* const* cols;
  const uint64_t* flat;
  size_t n;
  const uint64_t* column(size_t c) const { return cols ? cols[c] : flat + c * n; }
};

// out[0 .. len) = the flat words [word0, word0 + len) of the matrix, cut at column seams: a range may lie inside one column (a
// column longer than a ring piece), cover many whole columns (32 per piece at 2^16 rows), or start and end inside columns.
// The caller has checked the range and the pointers (gather_columns_refused).
inline void gather_columns(const HostColumns& m, size_t word0, size_t len, uint64_t* out) {
  if (len == 0) return;
  size_t c = word0 / m.n, r = word0 % m.n;
  while (len) {
    const size_t take = len < m.n - r ? len : m.n - r;
    memcpy(out, m.column(c) + r, take * sizeof(uint64_t));
    out += take; len -= take; c++; r = 0;
  }
}

// 0: the range lies in the matrix and every column is a non-null, 8-byte aligned pointer; 1: the range does not (or n_columns * n
// overflows); 2 + c: column c is null or misaligned.
inline size_t gather_columns_refused(const uint64_t* const* cols, size_t n_columns, size_t n, size_t word0, size_t len) {
  if (n && n_columns > (size_t)-1 / n) return 1;
  const size_t words = n_columns * n;
  if (word0 > words || len > words - word0) return 1;
  if (!cols) return n_columns ? 2 : 0;
  for (size_t c = 0; c < n_columns; c++) if (!cols[c] || ((uintptr_t)cols[c] & 7)) return 2 + c;
  return 0;
}

// words >= p become w - p (one subtraction: 2^64 - 1 - p < p); returns how many changed.  The host twin of reduce_words_kernel.
inline uint64_t reduce_words_host(uint64_t* w, size_t count) {
  const uint64_t p = 0xFFFFFFFF00000001ull;
  uint64_t changed = 0;
  for (size_t i = 0; i < count; i++) if (w[i] >= p) { w[i] -= p; changed++; }
  return changed;
}

}  // namespace sbn
