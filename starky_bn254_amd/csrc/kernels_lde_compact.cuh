// HIP kernels of the compact LDE storage (gfx950; include/sbn.h SBN_LDE_COMPACT).  One header, included once by lde_compact.hip.
// A compact context keeps, of the coset LDE of a wide matrix, only the rows the quotient reads; the rows a query opens are
// evaluated again from the coefficients.  Matrices are COLUMN-MAJOR [col][row] u64, LDE rows in NATURAL order (kernels.cuh).
#pragma once
#include "poseidon.cuh"
#include "air.cuh"

// dense[c][j] = slot[c][j << row_log], j < qn, c = blockIdx.y: the quotient's rows of one LDE chunk, behind the sponge that read
// the chunk.  Lanes are consecutive j: coalesced stores, loads 2^row_log words apart out of a chunk sized to the Infinity Cache.
// Algorithmic bytes: 8 qn read + 8 qn written per column.
__global__ __launch_bounds__(256) void lde_keep_rows_kernel(const u64* __restrict__ slot, size_t m, u64* __restrict__ dense, size_t qn, u32 row_log) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= qn) return;
  const size_t c = blockIdx.y;
  dense[c * qn + j] = slot[c * m + (j << row_log)];
}

// The powers of the opened points of one slice of queries: table[q][j] = x_q^j = 7^j w_m^(rho_q j mod m), j < n, q = blockIdx.y,
// with rho_q = bitrev(idx[q0 + q]) the natural LDE row of leaf idx (shift[j] = 7^j, tw[e] = w_m^e for every e < m).
__global__ __launch_bounds__(256) void query_rows_table_kernel(u64* __restrict__ table, size_t n, u32 lde_log, const u64* __restrict__ shift,
                                                               const u64* __restrict__ tw, const u32* __restrict__ idx, u32 q0) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const u32 q = blockIdx.y;
  const u64 rho = bitrev32(idx[q0 + q], lde_log);
  const u64 e = (rho * (u64)j) & (((u64)1 << lde_log) - 1);   // rho, j < 2^23
  table[(size_t)q * n + j] = (F(shift[j]) * F(tw[e])).v;
}

// out[(q0 + q) * qstride + off + c] = sum_j coef[c][j] table[q][j]: QR_COLS columns x QR_QUERIES queries per workgroup, so that a
// coefficient serves QR_QUERIES products and a table word QR_COLS (one column per workgroup would read ncols * nq * n table words).
// Lanes stride j; the sums stay unreduced (Acc<F>, air.cuh) until the end, as in openings1_kernel; exact field arithmetic, so the
// canonical word is the one the transform stored.  n is a multiple of 512.  Columns / queries past the end repeat the last one
// and are not written.
static constexpr u32 QR_COLS = 4, QR_QUERIES = 4, QR_UNROLL = 2;
__global__ __launch_bounds__(256) void query_rows_eval_kernel(const u64* __restrict__ coef, size_t ncols, size_t n, const u64* __restrict__ table, u32 q0, u32 nq_slice,
                                                              u64* __restrict__ out, size_t qstride, size_t off) {
  __shared__ u64 sh[4][QR_COLS * QR_QUERIES];
  const size_t cbase = (size_t)blockIdx.x * QR_COLS;
  const u32 qbase = blockIdx.y * QR_QUERIES;
  const u64* cp[QR_COLS];
  const u64* tp[QR_QUERIES];
#pragma unroll
  for (u32 a = 0; a < QR_COLS; a++) cp[a] = coef + (cbase + a < ncols ? cbase + a : ncols - 1) * n;
#pragma unroll
  for (u32 b = 0; b < QR_QUERIES; b++) tp[b] = table + (size_t)(qbase + b < nq_slice ? qbase + b : nq_slice - 1) * n;
  Acc<F> acc[QR_COLS][QR_QUERIES];
#pragma unroll
  for (u32 a = 0; a < QR_COLS; a++)
#pragma unroll
    for (u32 b = 0; b < QR_QUERIES; b++) acc[a][b].clear();
  for (size_t i = threadIdx.x; i < n; i += 256 * QR_UNROLL) {
    u64 cv[QR_UNROLL][QR_COLS], tv[QR_UNROLL][QR_QUERIES];
#pragma unroll
    for (u32 k = 0; k < QR_UNROLL; k++) {
#pragma unroll
      for (u32 a = 0; a < QR_COLS; a++) cv[k][a] = cp[a][i + 256 * k];
#pragma unroll
      for (u32 b = 0; b < QR_QUERIES; b++) tv[k][b] = tp[b][i + 256 * k];
    }
    __builtin_amdgcn_sched_barrier(0);   // all the loads first
#pragma unroll
    for (u32 k = 0; k < QR_UNROLL; k++)
#pragma unroll
      for (u32 a = 0; a < QR_COLS; a++)
#pragma unroll
        for (u32 b = 0; b < QR_QUERIES; b++) acc[a][b].macv(F{cv[k][a]}, F(tv[k][b]));
  }
  const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (u32 a = 0; a < QR_COLS; a++)
#pragma unroll
    for (u32 b = 0; b < QR_QUERIES; b++) {
      F v = acc[a][b].value();
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v = v + F(__shfl_xor((unsigned long long)v.v, d, 64));
      if (lane == 0) sh[wv][a * QR_QUERIES + b] = v.v;
    }
  __syncthreads();
  if (threadIdx.x < QR_COLS * QR_QUERIES) {
    const u32 a = threadIdx.x / QR_QUERIES, b = threadIdx.x % QR_QUERIES;
    const F t = F(sh[0][threadIdx.x]) + F(sh[1][threadIdx.x]) + F(sh[2][threadIdx.x]) + F(sh[3][threadIdx.x]);
    if (cbase + a < ncols && qbase + b < nq_slice) out[(size_t)(q0 + qbase + b) * qstride + off + cbase + a] = t.v;
  }
}
