// The cell-by-cell difference of a loaded trace and the canonical witness of its instance list (include/sbn.h,
// sbn_diff_witness_host / sbn_prover_diff_witness), the part that is plain C++: the compare of one tile of the two column-major
// matrices, the statistics from the counters, the choice of the rows whose cells are listed, the listing of a chosen row on the
// host, and the cut of the chosen rows into launches whose cells fit a scratch.  The host form runs all of it; the device form
// (witness_diff.hip) runs the compare and the listing as kernels (kernels_witdiff.cuh) and takes the rest from here.
// ORDER of the list: ascending (row, column) over the main columns [0, num_main); only when those are exhausted the same order
// over the derived columns [num_main, C).  Every count is exact whatever the cap.
// Plain C++ (no HIP): tests/sanitize/san_witness_diff.cpp includes this header alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sbn {

struct WitCell { uint64_t row, column, got, want; };                                               // = sbn_witness_cell
struct WitDiff {                                                                                    // = sbn_witness_diff
  uint32_t struct_size, reserved;
  uint64_t cells, main_cells, rows, columns, first_row, first_column, listed, pi_words, first_pi_word;
};
static constexpr uint64_t WIT_NONE = ~(uint64_t)0;
static constexpr uint32_t WIT_NO_ROW = ~(uint32_t)0;
static constexpr size_t WIT_TILE = 64;
static constexpr size_t WIT_MAX_CELLS = 65536;

// Rows [r0, r1) x columns [c0, c1) of the matrices (n rows; at most WIT_TILE each way, ragged edges shorter): a differing cell
// counts into col_cells[c - c0] and row_total[r - r0], a main one into row_main[r - r0] too; col_first[c - c0] becomes the smallest
// differing row of the column.  The four arrays are the TILE's (WIT_TILE entries, the caller's initial values); returns the count.
inline uint64_t wit_compare_tile(const uint64_t* got, const uint64_t* want, size_t n, size_t r0, size_t r1, size_t c0, size_t c1, size_t num_main,
                                 uint32_t* col_cells, uint32_t* col_first, uint32_t* row_main, uint32_t* row_total) {
  uint64_t cells = 0;
  for (size_t c = c0; c < c1; c++) {
    const uint64_t *g = got + c * n, *w = want + c * n;
    for (size_t r = r0; r < r1; r++) {
      if (g[r] == w[r]) continue;
      cells++;
      col_cells[c - c0]++;
      if ((uint32_t)r < col_first[c - c0]) col_first[c - c0] = (uint32_t)r;
      row_total[r - r0]++;
      if (c < num_main) row_main[r - r0]++;
    }
  }
  return cells;
}

// The statistics from the counters of all C columns and, where a cell differs, of all n rows (row_total may be null when none
// does).  first_row / first_column: the smallest (row, column) over the main columns, over the derived ones when no main cell
// differs -- a column that differs on the first such row has it as its own first row.
inline void wit_statistics(const uint32_t* col_cells, const uint32_t* col_first, size_t C, size_t num_main, const uint32_t* row_total, size_t n, WitDiff& d) {
  d.cells = d.main_cells = d.rows = d.columns = 0;
  d.first_row = d.first_column = WIT_NONE;
  for (size_t c = 0; c < C; c++) {
    if (!col_cells[c]) continue;
    d.cells += col_cells[c];
    d.columns++;
    if (c < num_main) d.main_cells += col_cells[c];
  }
  const size_t a = d.main_cells ? 0 : num_main, b = d.main_cells ? num_main : C;
  for (size_t c = a; c < b; c++)
    if (col_cells[c] && (d.first_row == WIT_NONE || col_first[c] < d.first_row)) { d.first_row = col_first[c]; d.first_column = c; }
  if (d.cells && row_total) for (size_t r = 0; r < n; r++) d.rows += row_total[r] != 0;
}

// One chosen row: its first `count` differing cells in columns [c0, c1), in column order, are entries [offset, offset + count) of
// the list.
struct WitJob { uint32_t row, c0, c1, offset, count; };

// The rows whose cells fill a list of `cap` entries: rows with a main cell in ascending order, then -- if the cap is not yet
// reached -- rows with a derived cell in ascending order; the last job may take only part of its row.  Returns the entries listed.
inline size_t wit_select_rows(const uint32_t* row_main, const uint32_t* row_total, size_t n, size_t num_main, size_t C, size_t cap, std::vector<WitJob>& jobs) {
  jobs.clear();
  size_t listed = 0;
  for (int phase = 0; phase < 2 && listed < cap; phase++)
    for (size_t r = 0; r < n && listed < cap; r++) {
      const size_t here = phase ? (size_t)row_total[r] - row_main[r] : row_main[r];
      if (!here) continue;
      const size_t take = std::min(here, cap - listed);
      jobs.push_back(WitJob{(uint32_t)r, (uint32_t)(phase ? num_main : 0), (uint32_t)(phase ? C : num_main), (uint32_t)listed, (uint32_t)take});
      listed += take;
    }
  return listed;
}

// The cells of one job from the matrices, on the host: out is the LIST (the job writes out[offset ..]).
inline void wit_list_row(const uint64_t* got, const uint64_t* want, size_t n, const WitJob& j, WitCell* out) {
  uint32_t written = 0;
  for (size_t c = j.c0; c < j.c1 && written < j.count; c++) {
    const uint64_t g = got[c * n + j.row], w = want[c * n + j.row];
    if (g != w) out[j.offset + written++] = WitCell{j.row, c, g, w};
  }
}

// The jobs [j0, j1) of one launch: as many as fit `room` bytes of scratch, each with its descriptor and its cells (j1 > j0 unless
// not even one fits: the caller refuses then).  The cells of a launch are contiguous in the list, from jobs[j0].offset on.
inline size_t wit_next_launch(const std::vector<WitJob>& jobs, size_t j0, size_t room) {
  size_t j1 = j0, used = 0;
  while (j1 < jobs.size()) {
    const size_t need = sizeof(WitJob) + (size_t)jobs[j1].count * sizeof(WitCell);
    if (used + need > room) break;
    used += need;
    j1++;
  }
  return j1;
}

}  // namespace sbn
