// AddressSanitizer + UBSan driver of csrc/witness_diff.hpp alone (tests/test_witness_diff_sanitize.py builds and runs it): the tile
// compare, the statistics, the row selection, the listing of a chosen row and the cut of the chosen rows into launches, on two
// matrices of 70 rows x 130 columns -- both dimensions ragged against the 64 x 64 tile, the main / derived boundary at column 70
// inside a tile -- with every buffer allocated at its exact size, so that one word read or written past an end is a report.  The
// caps: 0, 1, the exact number of differing cells, and more than that.  A brute-force walk in the header's order is the reference.
#include "witness_diff.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sbn;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const size_t N = 70, C = 130, MAIN = 70;
static uint64_t value(size_t r, size_t c) { return 0x9E3779B97F4A7C15ull * (r * 1000 + c + 1); }

struct Exact {   // a buffer of exactly k elements (a null pointer for none)
  void* p;
  Exact(size_t bytes) : p(bytes ? malloc(bytes) : nullptr) {}
  ~Exact() { free(p); }
};

// the list in the header's order, by brute force
static std::vector<WitCell> brute(const uint64_t* got, const uint64_t* want) {
  std::vector<WitCell> out;
  for (int phase = 0; phase < 2; phase++)
    for (size_t r = 0; r < N; r++)
      for (size_t c = phase ? MAIN : 0; c < (phase ? C : MAIN); c++)
        if (got[c * N + r] != want[c * N + r]) out.push_back(WitCell{r, c, got[c * N + r], want[c * N + r]});
  return out;
}

static void run(const std::vector<std::pair<size_t, size_t>>& planted) {
  Exact want_m(N * C * sizeof(uint64_t)), got_m(N * C * sizeof(uint64_t));
  uint64_t *want = (uint64_t*)want_m.p, *got = (uint64_t*)got_m.p;
  for (size_t c = 0; c < C; c++) for (size_t r = 0; r < N; r++) want[c * N + r] = value(r, c);
  memcpy(got, want, N * C * sizeof(uint64_t));
  for (auto& rc : planted) got[rc.second * N + rc.first] += 1;
  const std::vector<WitCell> ref = brute(got, want);

  // the compare, tile by tile as the host form runs it: the counters of a tile are WIT_TILE entries each, the rows' own a slice
  Exact cc_m(C * 4), cf_m(C * 4), rm_m(N * 4), rt_m(N * 4);
  uint32_t *col_cells = (uint32_t*)cc_m.p, *col_first = (uint32_t*)cf_m.p, *row_main = (uint32_t*)rm_m.p, *row_total = (uint32_t*)rt_m.p;
  memset(col_cells, 0, C * 4); memset(row_main, 0, N * 4); memset(row_total, 0, N * 4);
  for (size_t c = 0; c < C; c++) col_first[c] = WIT_NO_ROW;
  uint64_t total = 0;
  for (size_t r0 = 0; r0 < N; r0 += WIT_TILE)
    for (size_t c0 = 0; c0 < C; c0 += WIT_TILE) {
      const size_t r1 = std::min(N, r0 + WIT_TILE), c1 = std::min(C, c0 + WIT_TILE);
      // ragged tiles get ragged counters: exactly c1 - c0 and r1 - r0 entries
      Exact tc_m((c1 - c0) * 4), tf_m((c1 - c0) * 4);
      uint32_t *tc = (uint32_t*)tc_m.p, *tf = (uint32_t*)tf_m.p;
      for (size_t i = 0; i < c1 - c0; i++) { tc[i] = 0; tf[i] = WIT_NO_ROW; }
      total += wit_compare_tile(got, want, N, r0, r1, c0, c1, MAIN, tc, tf, row_main + r0, row_total + r0);
      for (size_t c = c0; c < c1; c++) { col_cells[c] += tc[c - c0]; col_first[c] = std::min(col_first[c], tf[c - c0]); }
    }
  EXPECT(total == ref.size());

  WitDiff d{};
  wit_statistics(col_cells, col_first, C, MAIN, row_total, N, d);
  size_t main_cells = 0, rows = 0, cols = 0;
  for (const WitCell& e : ref) main_cells += e.column < MAIN;
  for (size_t r = 0; r < N; r++) { bool any = false; for (const WitCell& e : ref) any |= e.row == r; rows += any; }
  for (size_t c = 0; c < C; c++) { bool any = false; for (const WitCell& e : ref) any |= e.column == c; cols += any; }
  EXPECT(d.cells == ref.size() && d.main_cells == main_cells && d.rows == rows && d.columns == cols);
  EXPECT(ref.empty() ? (d.first_row == WIT_NONE && d.first_column == WIT_NONE) : (d.first_row == ref[0].row && d.first_column == ref[0].column));
  WitDiff clean{};
  wit_statistics(col_cells, col_first, C, MAIN, nullptr, N, clean);   // no row counters: what a clean device diff hands in
  EXPECT(clean.cells == d.cells && (d.cells == 0 || clean.rows == 0));

  for (size_t cap : {(size_t)0, (size_t)1, ref.size(), ref.size() + 5}) {
    std::vector<WitJob> jobs;
    const size_t listed = wit_select_rows(row_main, row_total, N, MAIN, C, cap, jobs);
    EXPECT(listed == std::min(cap, ref.size()));
    Exact out_m(listed * sizeof(WitCell));
    WitCell* out = (WitCell*)out_m.p;
    size_t at = 0;
    for (const WitJob& j : jobs) { EXPECT(j.offset == at && j.count > 0); at += j.count; wit_list_row(got, want, N, j, out); }
    EXPECT(at == listed);
    for (size_t i = 0; i < listed; i++) EXPECT(out[i].row == ref[i].row && out[i].column == ref[i].column && out[i].got == ref[i].got && out[i].want == ref[i].want);
    // the launches of the device form: every room from one that holds nothing to one that holds everything cuts the jobs into
    // consecutive ranges whose cells and descriptors fit
    for (size_t room : {(size_t)0, sizeof(WitJob) + sizeof(WitCell), 3 * (sizeof(WitJob) + sizeof(WitCell)) + 7, (size_t)1 << 20}) {
      size_t j0 = 0, steps = 0;
      while (j0 < jobs.size()) {
        const size_t j1 = wit_next_launch(jobs, j0, room);
        if (j1 == j0) break;   // (a row that does not fit: the caller refuses)
        size_t used = 0;
        for (size_t j = j0; j < j1; j++) used += sizeof(WitJob) + jobs[j].count * sizeof(WitCell);
        EXPECT(used <= room && j1 <= jobs.size());
        j0 = j1; steps++;
      }
      if (room == (size_t)1 << 20) EXPECT(j0 == jobs.size() && steps <= 1);
      if (room == 0) EXPECT(j0 == 0);
    }
  }
}

int main() {
  run({});                                                                       // a clean pair
  run({{0, 0}});
  run({{69, 129}});                                                              // the last cell: derived only
  run({{63, 63}, {64, 64}, {69, 69}, {69, 70}, {0, 129}, {5, 64}, {5, 65}, {5, 3}});   // tile corners, the main / derived boundary, a derived cell on the first row
  std::vector<std::pair<size_t, size_t>> column, row, all;
  for (size_t r = 0; r < N; r++) column.push_back({r, 66});
  for (size_t c = 0; c < C; c++) row.push_back({65, c});
  for (size_t r = 0; r < N; r++) for (size_t c = 0; c < C; c++) all.push_back({r, c});
  run(column);
  run(row);
  run(all);
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("witness diff: tiles, statistics, caps 0, 1, exact and oversize, and the launch cuts ok\n");
  return 0;
}
