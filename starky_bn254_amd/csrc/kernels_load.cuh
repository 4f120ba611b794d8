// The kernels of the trace intake, included by trace_load.hip alone: row-major pieces of a trace -> the column-major d_trace
// (include/sbn.h sbn_prover_load_trace_rows), and behind it the canonical-form scan of a column-major upload and its reducing twin.
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

// Canonical-form scan of a host trace on its way in (trace_load.hip prove_host_trace; sbn_first_non_canonical): *first_bad =
// min(*first_bad, base + i) over the words w[i] >= p.  Bandwidth-bound: 16-byte loads, grid-stride; a wave whose lanes all saw
// canonical words issues no atomic (wave vote), any other wave issues one, after a min over its lanes.  `w` may sit 8 bytes
// off a 16-byte boundary: lane 0 of the grid takes the word in front of the first whole vector and the one behind the last.
typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));   // (a load of this type stays ONE global_load_dwordx4)
__global__ __launch_bounds__(256) void first_non_canonical_kernel(const u64* __restrict__ w, size_t count, u64 base, unsigned long long* first_bad) {
  const size_t head = (((size_t)w & 8) && count) ? 1 : 0;
  const u64x2_t* __restrict__ v = reinterpret_cast<const u64x2_t*>(w + head);
  const size_t nvec = (count - head) >> 1;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  u64 bad = ~(u64)0;
#pragma unroll 4
  for (size_t i = tid; i < nvec; i += stride) {
    const u64x2_t x = v[i];
    const bool b0 = x.x >= GLP, b1 = x.y >= GLP;
    if (b0 | b1) { const u64 j = head + 2 * i + (b0 ? 0 : 1); bad = bad < j ? bad : j; }
  }
  if (tid == 0) {
    const size_t last = head + 2 * nvec;   // < count iff one word is left behind the vectors
    if (last < count && w[last] >= GLP) bad = bad < last ? bad : last;
    if (head && w[0] >= GLP) bad = 0;
  }
  if (!__any(bad != ~(u64)0)) return;
  for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor((unsigned long long)bad, d, 64); bad = o < bad ? o : bad; }
  if ((threadIdx.x & 63) == 0) atomicMin(first_bad, (unsigned long long)(base + bad));
}

// The scan's twin for SBN_TRACE_REDUCE (trace_load.hip prove_host_columns; sbn_reduce_words): in place, w[i] >= p becomes w[i] - p
// (one subtraction: 2^64 - 1 - p < p), and *reduced grows by the number of words changed.  Bandwidth-bound: 16-byte loads,
// grid-stride, no LDS; a lane stores only a vector it changed, so a canonical trace costs what the scan costs (reads only).  The
// loop is wave-uniform (a wave leaves it as a whole), so the changed words are counted from ballots, and a wave that changed
// something issues one atomicAdd from its first lane.  Head and tail as in the scan: `w` may sit 8 bytes off a 16-byte boundary.
__global__ __launch_bounds__(256) void reduce_words_kernel(u64* __restrict__ w, size_t count, unsigned long long* reduced) {
  const size_t head = (((size_t)w & 8) && count) ? 1 : 0;
  u64x2_t* __restrict__ v = reinterpret_cast<u64x2_t*>(w + head);
  const size_t nvec = (count - head) >> 1;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const size_t lane = threadIdx.x & 63;
  unsigned long long changed = 0;   // wave-uniform
  for (size_t i0 = tid - lane; i0 < nvec; i0 += stride) {
    const size_t i = i0 + lane;
    bool b0 = false, b1 = false;
    if (i < nvec) {
      u64x2_t x = v[i];
      b0 = x.x >= GLP; b1 = x.y >= GLP;
      if (b0 | b1) { if (b0) x.x -= GLP; if (b1) x.y -= GLP; v[i] = x; }
    }
    if (__any(b0 | b1)) changed += (unsigned long long)(__popcll(__ballot(b0)) + __popcll(__ballot(b1)));
  }
  if (tid == 0) {   // (lane 0 of the grid's first wave: what it adds here its atomicAdd below carries)
    const size_t last = head + 2 * nvec;   // < count iff one word is left behind the vectors
    if (last < count && w[last] >= GLP) { w[last] -= GLP; changed++; }
    if (head && w[0] >= GLP) { w[0] -= GLP; changed++; }
  }
  if (lane == 0 && changed) atomicAdd(reduced, changed);
}
