// Row-major pieces of a trace -> the column-major d_trace (trace_rows.hip; include/sbn.h sbn_prover_load_trace_rows).  Included by
// trace_rows.hip alone.
#pragma once
#include "gl.cuh"

namespace rowsk {


// One workgroup moves a tile of RT_TILE rows x RT_TILE columns through LDS.  Load: wave w takes the tile rows w, w + 4, ...; its 64
// lanes read 64 consecutive words of one source row (512 contiguous bytes; a row starts on an 8-byte boundary only, n_cols is odd
// in most tables) and write them to one LDS row -- consecutive 8-byte slots, no bank conflict.  Store: wave w takes the tile
// columns w, w + 4, ...; lane l reads LDS row l -- with RT_PITCH = 65 words the 32 lanes of a ds_read_b64 group sit 130 dwords
// apart, i.e. on the even banks 2l mod 64, each lane on its own pair -- and the wave writes 64 consecutive rows of one trace
// column (512 contiguous bytes).  All sixteen loads of a lane are issued before the first is used.
static constexpr int RT_TILE = 64, RT_PITCH = RT_TILE + 1, RT_THREADS = 256, RT_WAVES = RT_THREADS / 64, RT_PER_LANE = RT_TILE / RT_WAVES;

// err[0]: min over the words >= p of row * n_cols + col, rows counted in the whole trace (all ones: none; reduce = 0 only)
// err[1]: number of words reduced (reduce = 1 only)
// err[2]: the same minimum over the words >= 2^16 of the columns [rc0, rc1), after the reduction (all ones: none)
struct RowsParams {
  const u64* src; size_t src_stride;   // the piece: row r of it at src + r * src_stride, n_cols words
  size_t R, n_cols;                    // rows of the piece, words per row
  size_t r0, n;                        // its first row in the trace; rows of the trace (r0 + R <= n)
  u64* trace;                          // [>= n_cols][n]
  int reduce, rc0, rc1;                // rc0 == rc1: no range test
  unsigned long long* err;
};

__global__ __launch_bounds__(RT_THREADS, 4) void rows_to_columns_kernel(const RowsParams q) {   // (33,280 B of LDS: four workgroups per CU)
  __shared__ u64 tile[RT_TILE * RT_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t rt = (size_t)blockIdx.x * RT_TILE, ct = (size_t)blockIdx.y * RT_TILE;   // first row (of the piece) and column of the tile
  u64 bad = ~(u64)0, bad_range = ~(u64)0;
  unsigned changed = 0;
  {
    const size_t c = ct + lane;
    const bool col_ok = c < q.n_cols, ranged = col_ok && (long long)c >= q.rc0 && (long long)c < q.rc1;
    const u64* const src = q.src + (rt + wave) * q.src_stride + c;   // row k of this lane: RT_WAVES * k rows further
    const size_t rows_left = q.R > rt + wave ? q.R - (rt + wave) : 0;
    u64 w[RT_PER_LANE];
#pragma unroll
    for (int k = 0; k < RT_PER_LANE; k++)
      w[k] = (col_ok && (size_t)(RT_WAVES * k) < rows_left) ? src[(size_t)(RT_WAVES * k) * q.src_stride] : 0;   // (zero: canonical and in range, never stored to the trace)
#pragma unroll
    for (int k = 0; k < RT_PER_LANE; k++) {
      if (w[k] >= GLP) {
        if (q.reduce) { w[k] -= GLP; changed++; }   // one subtraction: 2^64 - 1 - p < p
        else { const u64 at = (q.r0 + rt + wave + RT_WAVES * k) * q.n_cols + c; bad = bad < at ? bad : at; }
      }
      if (ranged && w[k] >= 65536) { const u64 at = (q.r0 + rt + wave + RT_WAVES * k) * q.n_cols + c; bad_range = bad_range < at ? bad_range : at; }
      tile[(wave + RT_WAVES * k) * RT_PITCH + lane] = w[k];
    }
  }
  __syncthreads();
  {
    const size_t r = rt + lane;
    if (r < q.R) {
      u64* const dst = q.trace + (ct + wave) * q.n + q.r0 + r;   // column k of this lane: RT_WAVES * k columns further
      const size_t cols_left = q.n_cols > ct + wave ? q.n_cols - (ct + wave) : 0;
#pragma unroll
      for (int k = 0; k < RT_PER_LANE; k++)
        if ((size_t)(RT_WAVES * k) < cols_left) dst[(size_t)(RT_WAVES * k) * q.n] = tile[lane * RT_PITCH + wave + RT_WAVES * k];
    }
  }
  // the error words: every lane of the workgroup is here (no divergence behind the barrier), so the wave votes and shuffles are whole
  if (q.reduce) {
    if (__any(changed != 0)) {
      for (int d = 32; d >= 1; d >>= 1) changed += __shfl_xor(changed, d, 64);
      if (lane == 0) atomicAdd(q.err + 1, (unsigned long long)changed);
    }
  } else if (__any(bad != ~(u64)0)) {
    for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor((unsigned long long)bad, d, 64); bad = o < bad ? o : bad; }
    if (lane == 0) atomicMin(q.err, (unsigned long long)bad);
  }
  if (q.rc1 > q.rc0 && __any(bad_range != ~(u64)0)) {
    for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor((unsigned long long)bad_range, d, 64); bad_range = o < bad_range ? o : bad_range; }
    if (lane == 0) atomicMin(q.err + 2, (unsigned long long)bad_range);
  }
}

}  // namespace rowsk
