// Kernels of sbn_prover_diff_witness (witness_diff.hip): the loaded trace against the canonical witness of its instance list, both
// column-major [C][n] on the device.
//   compare_kernel  one pass over both matrices.  A lane stands for a row: a wave loads 64 consecutive rows of one column from each
//                   matrix (512 contiguous bytes apiece) and walks over the 64 columns of its tile, four columns in flight.  Per
//                   column the ballot's popcount goes into ONE atomicAdd per wave and the first row into an atomicMin, both only
//                   when the ballot is non-zero; per row every lane keeps its main and total counts in registers across the columns
//                   and issues one atomicAdd each at the end, only if non-zero.  A clean trace issues no atomic.  All of them are
//                   integer adds and minima: the result does not depend on arrival order.  Ragged edges are lane predicates: the
//                   last column tile is short (1,676 = 26 * 64 + 12) and the main / derived boundary falls inside a tile (398).
//   list_kernel     one wave per chosen row (witness_diff.hpp WitJob): its differing cells in columns [c0, c1), in column order,
//                   written compactly by ballot and prefix popcount inside the wave-ordered loop over the columns, 64 at a time.
// n is a multiple of COMPARE_THREADS (a power of two >= 512: the launcher checks).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace wd {

typedef unsigned long long ull;
static constexpr unsigned COMPARE_THREADS = 256, TILE_COLS = 64, LIST_THREADS = 64, UNROLL = 4;
struct Job { unsigned row, c0, c1, offset, count; };   // = sbn::WitJob
struct Cell { ull row, column, got, want; };           // = sbn::WitCell = sbn_witness_cell

// grid (n / COMPARE_THREADS, ceil(C / TILE_COLS)).  col_cells, row_main, row_total zeroed and col_first all ones by the launcher.
__global__ __launch_bounds__(COMPARE_THREADS) void compare_kernel(const ull* __restrict__ got, const ull* __restrict__ want, size_t n, unsigned C, unsigned num_main,
                                                                  unsigned* __restrict__ col_cells, unsigned* __restrict__ col_first, unsigned* __restrict__ row_main,
                                                                  unsigned* __restrict__ row_total) {
  const size_t row = (size_t)blockIdx.x * COMPARE_THREADS + threadIdx.x;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave_row = (unsigned)row - lane;
  const unsigned c0 = blockIdx.y * TILE_COLS, c1 = min(c0 + TILE_COLS, C);
  unsigned mine_main = 0, mine_all = 0;
  for (unsigned c = c0; c < c1; c += UNROLL) {
    ull a[UNROLL], b[UNROLL];
#pragma unroll
    for (unsigned u = 0; u < UNROLL; u++) {   // a column past the edge re-reads the last one; its predicate is off
      const size_t at = (size_t)min(c + u, c1 - 1) * n + row;
      a[u] = got[at];
      b[u] = want[at];
    }
#pragma unroll
    for (unsigned u = 0; u < UNROLL; u++) {
      const bool differs = c + u < c1 && a[u] != b[u];
      const ull m = __ballot(differs);
      if (m) {   // wave-uniform
        if (lane == 0) {
          atomicAdd(&col_cells[c + u], (unsigned)__popcll(m));
          atomicMin(&col_first[c + u], wave_row + (unsigned)__ffsll((long long)m) - 1u);
        }
        mine_all += differs;
        mine_main += differs && c + u < num_main;
      }
    }
  }
  if (mine_all) atomicAdd(&row_total[row], mine_all);
  if (mine_main) atomicAdd(&row_main[row], mine_main);
}

// grid (jobs of the launch), LIST_THREADS lanes.  out: the cells of THIS launch, entry 0 = list entry `base` (= the offset of its
// first job); job j writes out[j.offset - base .. + j.count).
__global__ __launch_bounds__(LIST_THREADS) void list_kernel(const ull* __restrict__ got, const ull* __restrict__ want, size_t n, const Job* __restrict__ jobs, unsigned base,
                                                            Cell* __restrict__ out) {
  const Job j = jobs[blockIdx.x];
  const unsigned lane = threadIdx.x;
  unsigned written = 0;
  for (unsigned c = j.c0; c < j.c1 && written < j.count; c += LIST_THREADS) {
    const unsigned col = c + lane;
    const bool in = col < j.c1;
    ull a = 0, b = 0;
    if (in) { a = got[(size_t)col * n + j.row]; b = want[(size_t)col * n + j.row]; }
    const bool differs = in && a != b;
    const ull m = __ballot(differs);
    const unsigned pos = written + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (differs && pos < j.count) out[j.offset - base + pos] = Cell{j.row, col, a, b};
    written += (unsigned)__popcll(m);
  }
}

}  // namespace wd
