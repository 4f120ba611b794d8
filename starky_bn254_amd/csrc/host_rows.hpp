// A host trace held ROW-major (include/sbn.h sbn_host_rows): what the reference's generators hold in front of their `transpose`,
// `rows: Vec<[F; N]>` (one flat allocation, rows `row_stride` words apart) or `Vec<Vec<F>>` (one allocation per row).  The upload
// of sbn_prover_load_trace_rows cuts the row range into ring pieces of whole rows and copies each piece PACKED -- n_cols words
// per row, the stride padding dropped -- through copy_rows below; the transposition to the column-major trace runs on the
// device (kernels_load.cuh).  The twin of host_columns.hpp.  Plain C++ (no HIP): tests/sanitize/san_rows.cpp includes this
// header alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace sbn {

// The virtual row-major matrix [n_rows][n_cols]: row r is ptrs[r][0 .. n_cols), or flat[r * stride .. r * stride + n_cols) when
// ptrs is null.  The words between n_cols and stride are never read.
struct HostRows {
  const uint64_t* flat;
  size_t stride;
  const uint64_t* const* ptrs;
  size_t n_rows, n_cols;
  const uint64_t* row(size_t r) const { return ptrs ? ptrs[r] : flat + r * stride; }
};

// Rows per ring piece: as many whole rows as `slot_words` holds, at least one (a row longer than a slot is refused by the caller),
// at most the matrix.
inline size_t rows_per_piece(size_t n_rows, size_t n_cols, size_t slot_words) {
  if (n_cols == 0) return n_rows;
  const size_t fit = slot_words / n_cols;
  return fit == 0 ? 0 : (fit < n_rows ? fit : n_rows);
}
// Piece k of the cut: rows [*r0, *r1); the last piece may be short.  Returns false past the last piece.
inline bool piece_rows(size_t n_rows, size_t per_piece, size_t k, size_t* r0, size_t* r1) {
  if (per_piece == 0 || k > n_rows / per_piece || k * per_piece >= n_rows) return false;
  *r0 = k * per_piece;
  *r1 = n_rows - *r0 < per_piece ? n_rows : *r0 + per_piece;
  return true;
}

// out[(r - r0) * n_cols + c] = row r, column c for r0 <= r < r1: the piece as the device transposition reads it.  A flat source
// whose stride is n_cols is one copy.  The caller has checked the range and the pointers (host_rows_refused).
inline void copy_rows(const HostRows& m, size_t r0, size_t r1, uint64_t* out) {
  if (r1 <= r0 || m.n_cols == 0) return;
  if (!m.ptrs && m.stride == m.n_cols) { memcpy(out, m.flat + r0 * m.stride, (r1 - r0) * m.n_cols * sizeof(uint64_t)); return; }
  for (size_t r = r0; r < r1; r++, out += m.n_cols) memcpy(out, m.row(r), m.n_cols * sizeof(uint64_t));
}

// The refusals of the pointers and the stride, in the order of include/sbn.h: 0 fine; 1: both or neither of flat / ptrs; 2: stride
// below n_cols (flat form), or n_rows * stride overflows; 3 + r: row r is null or not 8-byte aligned (flat form: r = 0).
inline size_t host_rows_refused(const HostRows& m) {
  if ((m.flat != nullptr) == (m.ptrs != nullptr)) return 1;
  if (m.flat) {
    if (m.stride < m.n_cols || (m.stride && m.n_rows > (size_t)-1 / sizeof(uint64_t) / m.stride)) return 2;
    return ((uintptr_t)m.flat & 7) ? 3 : 0;
  }
  for (size_t r = 0; r < m.n_rows; r++) if (!m.ptrs[r] || ((uintptr_t)m.ptrs[r] & 7)) return 3 + r;
  return 0;
}

}  // namespace sbn
