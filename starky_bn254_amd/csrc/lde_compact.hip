// Compact LDE storage (include/sbn.h SBN_LDE_COMPACT): the launchers of its two stages, reached from prover.hip through
// prover_ctx.hpp.  Commit side: the quotient's rows of an LDE chunk are copied out of the chunk ring behind the sponge
// (lde_keep_rows_kernel).  Query side: the rows a query opens are evaluated from the coefficients at the points
// x_q = 7 w_m^bitrev(idx[q]) (query_rows_*), in slices of QUERY_SLICE queries whose power tables share one scratch buffer.
#include "prover_ctx.hpp"
#include "kernels_lde_compact.cuh"

static constexpr u32 QUERY_SLICE = 64;   // queries per table: QUERY_SLICE * n words (the prover lends d_part, 64 n words)

void launch_lde_keep_rows(const u64* slot, size_t m, u64* dense, size_t qn, u32 row_log, size_t nc, hipStream_t s) {
  if (nc == 0) return;
  hipLaunchKernelGGL(lde_keep_rows_kernel, dim3((unsigned)((qn + 255) / 256), (unsigned)nc), dim3(256), 0, s, slot, m, dense, qn, row_log);
}

int launch_query_rows(const u64* coef, size_t ncols, size_t n, u32 lde_log, const u64* shift, const u64* tw_f, const u32* d_idx, u32 nq, u64* table,
                      u64* out, size_t qstride, size_t off, hipStream_t s) {
  if (ncols == 0 || nq == 0) return 0;
  if (n % (256 * QR_UNROLL)) return fail(SBN_ERR_UNSUPPORTED, "query rows need a multiple of %u coefficients", 256 * QR_UNROLL);
  for (u32 q0 = 0; q0 < nq; q0 += QUERY_SLICE) {
    const u32 cnt = std::min(QUERY_SLICE, nq - q0);
    hipLaunchKernelGGL(query_rows_table_kernel, dim3((unsigned)((n + 255) / 256), cnt), dim3(256), 0, s, table, n, lde_log, shift, tw_f, d_idx, q0);
    hipLaunchKernelGGL(query_rows_eval_kernel, dim3((unsigned)((ncols + QR_COLS - 1) / QR_COLS), (cnt + QR_QUERIES - 1) / QR_QUERIES), dim3(256), 0, s, coef, ncols, n,
                       table, q0, cnt, out, qstride, off);
  }
  HIPC(hipGetLastError());
  return 0;
}
