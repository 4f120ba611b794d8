// The explain kernel (trace_explain.hip says what it does) and its parameter block, shared by the two units that instantiate it:
// trace_explain.hip (the driver, the Z kernels, the curve and small tables) and trace_explain_fq12.hip (the three tables with the
// Fq12 gadget, which take as long to compile as all the others together).
#pragma once
#include "air_record.cuh"

struct ExplainParams {
  const u64* trace; const u64* zval; size_t n;
  const u64* xs; const u64* lag_first; const u64* lag_last; u64 last;   // the trace domain: g^i, [i == 0], [i == n - 1]; g^-1
  u64 alpha[SBN_NCH], gamma0, gamma1;
  int kind, num_io, nconstraints, num_zs;
  const u64* rows; size_t n_rows;                       // listed-rows form; rows == null: every row of the trace
  unsigned long long* stats; u32 nblk;                  // whole-trace form: [2][nblk] failing rows, first row
  unsigned long long* zstats;                           //                   [2][num_zs]
  unsigned char* bits; u32 bbytes;                      // listed-rows form: [n_rows][bbytes]
  unsigned char* zbits; u32 zbytes;                     //                   [n_rows][zbytes]
};

struct RecDevRow {
  const u64* base; size_t m; size_t i, inext;
  __device__ __forceinline__ RF l(int c) const { return RF(F(base[(size_t)c * m + i])); }
  __device__ __forceinline__ RF n(int c) const { return RF(F(base[(size_t)c * m + inext])); }
};

// The alpha-power tables and the public-input constants are `const __restrict__` arguments of their own, as in quotient_kernel:
// the uniformly indexed entries come through scalar loads.
template <int KIND>
__global__ __launch_bounds__(256) void explain_kernel(ExplainParams p, const u64* __restrict__ apow0, const u64* __restrict__ apow1,
                                                      const void* __restrict__ pic) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t cnt = p.rows ? p.n_rows : p.n;
  const bool live = gid < cnt;                          // a padding lane walks row 0 with the others (the ballots need the whole wave) and notes nothing
  const size_t i = live ? (p.rows ? (size_t)p.rows[gid] : gid) : 0;
  Cons<RF> cs;
  cs.alpha[0] = RF(F(p.alpha[0])); cs.alpha[1] = RF(F(p.alpha[1]));
  cs.apow[0] = (const RF*)apow0; cs.apow[1] = (const RF*)apow1;
  cs.z_last = RF(F(p.xs[i]) - F(p.last));
  cs.l_first = RF(F(p.lag_first[i]));
  cs.l_last = RF(F(p.lag_last[i]));
  cs.counts = nullptr;
  cs.stats = p.rows ? nullptr : p.stats; cs.nblk = p.nblk;
  cs.bits = p.rows ? p.bits + (live ? gid : 0) * p.bbytes : nullptr;
  cs.rowi = i; cs.live = live;
  const RecDevRow row{p.trace, p.n, i, (i + 1) & (p.n - 1)};
  record_row<KIND>(cs, row, p.num_io, p.nconstraints, pic);
}

// trace_explain_fq12.hip: explain_kernel<4 / 6 / 8> (FQ12_EXP, FQ12_EXP_U64, FQ12_MUL)
void launch_explain_kernel_fq12(int kind, dim3 grid, hipStream_t st, const ExplainParams& ep, const u64* apow0, const u64* apow1, const void* pic);
