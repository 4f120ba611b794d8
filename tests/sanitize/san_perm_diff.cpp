// AddressSanitizer + UBSan driver of csrc/perm_diff.hpp alone (tests/test_perm_diff_sanitize.py builds and runs it): the multiset
// difference of two columns on small matrices, every buffer allocated at its exact size so that one word read or written past an
// end is a report -- the caps 0 (a null entry buffer), 1 and the exact number of differing values; a pair whose values are all out
// of the histogram's range; 512 rows with both kinds; and the list form the device route hands over.
#include "perm_diff.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

using namespace sbn;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const uint64_t GLP = 0xFFFFFFFF00000001ull;

// the answer by two ordered maps
struct Expect { PermStat st; std::vector<PermEntry> all; };
static Expect expect(const uint64_t* L, const uint64_t* R, size_t n) {
  std::map<uint64_t, PermEntry> m;
  for (size_t i = 0; i < n; i++) {
    PermEntry& a = m.emplace(L[i], PermEntry{L[i], 0, 0, PERM_NO_ROW, PERM_NO_ROW}).first->second;
    if (!a.count_lhs++) a.first_row_lhs = i;
    PermEntry& b = m.emplace(R[i], PermEntry{R[i], 0, 0, PERM_NO_ROW, PERM_NO_ROW}).first->second;
    if (!b.count_rhs++) b.first_row_rhs = i;
  }
  Expect e{PermStat{0, 0, 0, 0}, {}};
  for (const auto& kv : m) {
    const PermEntry& x = kv.second;
    if (x.count_lhs == x.count_rhs) continue;
    e.st.differing_values++;
    if (x.count_lhs > x.count_rhs) e.st.excess_lhs += x.count_lhs - x.count_rhs; else e.st.excess_rhs += x.count_rhs - x.count_lhs;
    e.all.push_back(x);
  }
  return e;
}
static bool same(const PermEntry& a, const PermEntry& b) {
  return a.value == b.value && a.count_lhs == b.count_lhs && a.count_rhs == b.count_rhs && a.first_row_lhs == b.first_row_lhs && a.first_row_rhs == b.first_row_rhs;
}

// the two columns in allocations of exactly n words, the entries in one of exactly min(cap, differing) -- none at all for cap 0
static void run(const std::vector<uint64_t>& l, const std::vector<uint64_t>& r, size_t cap) {
  const size_t n = l.size();
  uint64_t* L = (uint64_t*)malloc(n * sizeof(uint64_t));
  uint64_t* R = (uint64_t*)malloc(n * sizeof(uint64_t));
  for (size_t i = 0; i < n; i++) { L[i] = l[i]; R[i] = r[i]; }
  const Expect e = expect(L, R, n);
  const size_t room = cap < e.all.size() ? cap : e.all.size();
  PermEntry* out = room ? (PermEntry*)malloc(room * sizeof(PermEntry)) : nullptr;
  PermStat st{9, 9, 9, 9};
  diff_columns(L, R, n, cap, st, out);
  EXPECT(st.differing_values == e.st.differing_values && st.excess_lhs == e.st.excess_lhs && st.excess_rhs == e.st.excess_rhs && st.entries == room);
  for (size_t k = 0; k < room && k < st.entries; k++) EXPECT(same(out[k], e.all[k]));
  free(out); free(L); free(R);
}
static void caps(const std::vector<uint64_t>& l, const std::vector<uint64_t>& r) {
  std::vector<uint64_t> a = l, b = r;
  const size_t d = (size_t)expect(a.data(), b.data(), a.size()).st.differing_values;
  for (size_t cap : {(size_t)0, (size_t)1, d ? d - 1 : 0, d, d + 1, (size_t)1 << 20}) run(l, r, cap);
}

int main() {
  // small values only: the histogram and its ends and seam
  caps({0, 1, 1, 32767, 32768, 65535, 7, 7}, {1, 0, 32767, 2, 65535, 65535, 7, 9});
  // equal multisets in another order: nothing differs, nothing is written
  caps({5, 6, 7, 7, 65535, 0}, {7, 0, 65535, 5, 7, 6});
  // every value out of the histogram's range, the largest canonical word and repeats among them
  caps({65536, GLP - 1, GLP - 1, 1ull << 40, 70000, 65536}, {GLP - 1, 65536, 1ull << 40, 1ull << 41, 65537, 65537});
  // 512 rows: a sorted column against itself with cells of both kinds changed, first rows deep in the column
  {
    std::vector<uint64_t> l(512), r(512);
    for (size_t i = 0; i < 512; i++) l[i] = r[511 - i] = i / 2;
    caps(l, r);
    r[0] = 254; r[511] = 65536; r[255] = 32768; r[256] = GLP - 1; l[300] = 65535; l[301] = 1ull << 63;
    caps(l, r);
  }
  // the list form: cells in any order, appended behind entries that are already there
  {
    std::vector<PermCell> l{{70000, 9}, {65536, 4}, {70000, 2}, {GLP - 1, 0}}, r{{65536, 7}, {70000, 5}, {1ull << 33, 1}};
    PermEntry* out = (PermEntry*)malloc(3 * sizeof(PermEntry));
    out[0] = PermEntry{3, 1, 0, 0, PERM_NO_ROW};
    PermStat st{1, 1, 0, 1};
    diff_cells(l, r, 3, st, out);
    EXPECT(st.differing_values == 4 && st.excess_lhs == 3 && st.excess_rhs == 1 && st.entries == 3);
    EXPECT(same(out[0], PermEntry{3, 1, 0, 0, PERM_NO_ROW}) && same(out[1], PermEntry{70000, 2, 1, 2, 5}) && same(out[2], PermEntry{1ull << 33, 0, 1, PERM_NO_ROW, 1}));
    free(out);
    std::vector<PermCell> none;
    PermStat clean{0, 0, 0, 0};
    diff_cells(none, none, 0, clean, nullptr);
    EXPECT(clean.differing_values == 0 && clean.entries == 0);
  }
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("perm diff: caps, out-of-range pairs, 512 rows and the list form ok\n");
  return 0;
}
