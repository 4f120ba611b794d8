// The exact multiset difference behind a failing permutation pair (include/sbn.h, sbn_explain_permutations_host /
// sbn_prover_explain_permutations): the lhs column of a pair against its rhs column as multisets of 64-bit words, no challenge and
// no seed.  Values below 2^16 -- every value of a range-checked pair -- are counted in one signed 32-bit histogram (+1 per lhs
// cell, -1 per rhs cell); all other values are collected as (value, row), sorted and walked side by side.  The statistics are
// exact whatever the cap; the listed values are the smallest first.  The device form (perm_diff.hip) runs the histogram in LDS
// and hands this header the cells it could not bin: diff_cells below is that second half alone.
// Plain C++ (no HIP): tests/sanitize/san_perm_diff.cpp includes this header alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sbn {

struct PermStat { uint64_t differing_values, excess_lhs, excess_rhs, entries; };                  // = sbn_perm_pair_stat
struct PermEntry { uint64_t value, count_lhs, count_rhs, first_row_lhs, first_row_rhs; };         // = sbn_perm_diff_entry
struct PermCell {
  uint64_t value, row;
  bool operator<(const PermCell& o) const { return value != o.value ? value < o.value : row < o.row; }
};
static constexpr uint64_t PERM_HIST_VALUES = (uint64_t)1 << 16;
static constexpr uint64_t PERM_NO_ROW = ~(uint64_t)0;

// One differing value into the statistics and, while the cap allows, into the list behind the entries already there.
inline void perm_diff_note(uint64_t value, uint64_t cl, uint64_t cr, uint64_t fl, uint64_t fr, size_t cap, PermStat& st, PermEntry* out) {
  st.differing_values++;
  if (cl > cr) st.excess_lhs += cl - cr; else st.excess_rhs += cr - cl;
  if (st.entries < cap) out[st.entries++] = PermEntry{value, cl, cr, fl, fr};
}

// The cells of the two sides given as lists (any order; sorted here): every value whose counts differ is added to `st` and
// appended to out[st.entries ..] up to `cap` entries in all, ascending.  The caller lists smaller values first.
inline void diff_cells(std::vector<PermCell>& l, std::vector<PermCell>& r, size_t cap, PermStat& st, PermEntry* out) {
  std::sort(l.begin(), l.end());
  std::sort(r.begin(), r.end());
  size_t i = 0, j = 0;
  while (i < l.size() || j < r.size()) {
    const uint64_t v = j == r.size() || (i < l.size() && l[i].value <= r[j].value) ? l[i].value : r[j].value;
    size_t i1 = i, j1 = j;
    while (i1 < l.size() && l[i1].value == v) i1++;
    while (j1 < r.size() && r[j1].value == v) j1++;
    if (i1 - i != j1 - j) perm_diff_note(v, i1 - i, j1 - j, i1 > i ? l[i].row : PERM_NO_ROW, j1 > j ? r[j].row : PERM_NO_ROW, cap, st, out);
    i = i1; j = j1;
  }
}

// Columns L and R of n rows as multisets.  out: room for min(differing values, cap) entries at least -- `cap` always suffices;
// never touched when cap == 0 (it may be null then).
inline void diff_columns(const uint64_t* L, const uint64_t* R, size_t n, size_t cap, PermStat& st, PermEntry* out) {
  st = PermStat{0, 0, 0, 0};
  std::vector<int32_t> hist(PERM_HIST_VALUES, 0);
  std::vector<PermCell> bl, br;
  for (size_t i = 0; i < n; i++) {
    if (L[i] < PERM_HIST_VALUES) hist[L[i]]++; else bl.push_back(PermCell{L[i], i});
    if (R[i] < PERM_HIST_VALUES) hist[R[i]]--; else br.push_back(PermCell{R[i], i});
  }
  // the histogram in ascending order: the statistics of every bin, the first `cap` values as candidates
  std::vector<uint32_t> cand;
  for (uint64_t v = 0; v < PERM_HIST_VALUES; v++) {
    const int32_t d = hist[v];
    hist[v] = -1;                                   // from here on: the candidate's index, or -1
    if (d == 0) continue;
    st.differing_values++;
    if (d > 0) st.excess_lhs += (uint64_t)d; else st.excess_rhs += (uint64_t)(-(int64_t)d);
    if (cand.size() < cap) { hist[v] = (int32_t)cand.size(); cand.push_back((uint32_t)v); }
  }
  // their counts and first rows: one more pass over the two columns
  if (!cand.empty()) {
    for (size_t k = 0; k < cand.size(); k++) out[k] = PermEntry{cand[k], 0, 0, PERM_NO_ROW, PERM_NO_ROW};
    for (size_t i = 0; i < n; i++) {
      if (L[i] < PERM_HIST_VALUES && hist[L[i]] >= 0) { PermEntry& e = out[hist[L[i]]]; if (!e.count_lhs++) e.first_row_lhs = i; }
      if (R[i] < PERM_HIST_VALUES && hist[R[i]] >= 0) { PermEntry& e = out[hist[R[i]]]; if (!e.count_rhs++) e.first_row_rhs = i; }
    }
    st.entries = cand.size();
  }
  diff_cells(bl, br, cap, st, out);                 // all of them larger than any binned value
}

}  // namespace sbn
