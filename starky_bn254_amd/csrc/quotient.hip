// The constraint kernels (kernels_quotient.cuh) as their own translation unit, built with the ordinary flags (the max-ILP scheduler of
// ntt.hip makes them spill, kernels_ntt.cuh).
#include "kernels_quotient.cuh"

// =================================================================================================
// K5  constraint / quotient evaluation (starky prover.rs `compute_quotient_polys`; P3)
// One thread per point i of the quotient's domain (2n points); local row = i, next row = (i + 2^quotient_degree_bits) mod 2n,
// each at LDE row (i << row_log).  At rate_bits 1 lanes are consecutive rows, so every column access is a coalesced 512-byte
// wave segment and the "next" access re-hits the same lines; at rate_bits r a wave's segment is 2^(r-1) times as long.  Output: quotient values acc_j / Z_H(x_i) for j < 2.
// Algorithmic bytes: 8*M*(C + Zc) read once, 16*M written.
// =================================================================================================
// `base` holds the local rows, `nbase` the next rows (the same matrix on one GPU; in the oversized-trace split a rank
// holds the LDE rows i = j * R + rho of its Merkle subtrees and, from R = 4 ranks up, a second plane with the rows i + 2).
struct DevRow {
  const u64* base; const u64* nbase; size_t m; size_t i, inext;
  __device__ __forceinline__ F l(int c) const { return F(base[(size_t)c * m + i]); }
  __device__ __forceinline__ F n(int c) const { return F(nbase[(size_t)c * m + inext]); }
};
struct DevZRow {
  const u64* base; const u64* nbase; size_t m; size_t i, inext;
  __device__ __forceinline__ F zl(int z) const { return F(base[(size_t)z * m + i]); }
  __device__ __forceinline__ F zn(int z) const { return F(nbase[(size_t)z * m + inext]); }
};
// The alpha-power tables and the public-input constants come in as `const __restrict__` kernel arguments of their own (not
// inside the parameter struct): only then does the compiler know that the kernel never writes them and fetches the
// uniformly indexed entries with SCALAR loads (s_load through the scalar cache, operand straight into the multiply-add);
// through the struct they were vector loads + v_readfirstlane with a memory latency in front of every term.
template <int KIND, int PART>
__global__ __launch_bounds__(256, 2) void quotient_kernel(QuotientParams p, const u64* __restrict__ apow0, const u64* __restrict__ apow1,
                                                          const void* __restrict__ pic_arg) {   // at least two waves per SIMD: at most 256 VGPRs
  const u32 seg = PART == 2 ? 2 + blockIdx.y : (u32)PART;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.m || !((p.seg_mask >> seg) & 1)) return;
  const size_t inext = (i + p.next_step) & (p.m - 1);
  const size_t ig = (i << p.row_shift) | p.row_rho;   // LDE point of local row i
  Cons<F> cs;
#pragma unroll
  for (int j = 0; j < SBN_NCH; j++) cs.alpha[j] = F(p.alpha[j]);
  cs.apow[0] = (const F*)apow0; cs.apow[1] = (const F*)apow1;
  cs.start(p.seg_count[seg]);
  cs.z_last = F(p.xs[ig]) - F(p.last);
  cs.l_first = F(p.lag_first[ig]);
  cs.l_last = F(p.lag_last[ig]);
  DevRow row{p.lde, p.lde_next, p.lde_stride, i << p.row_log, inext << p.row_log};
  DevZRow zrow{p.zlde, p.zlde_next, p.lde_stride, i << p.row_log, inext << p.row_log};
  if (KIND == 1) {
    if (PART == 0) g1op_eval(cs, row);
    else if (PART == 2) {
      if (seg == 2) permutation_checks(cs, row, zrow, G1OpShape(), p.num_zs, F(p.gamma0), F(p.gamma1), 0, p.zsplit);
      else permutation_checks(cs, row, zrow, G1OpShape(), p.num_zs, F(p.gamma0), F(p.gamma1), p.zsplit, p.num_zs);
    }
  } else if (KIND == 9) {   // MyStark: two lookup constraints, two permutation pairs
    if (PART == 0) lookup_eval(cs, row);
    else if (PART == 2) {
      if (seg == 2) permutation_checks(cs, row, zrow, LookupShape(), p.num_zs, F(p.gamma0), F(p.gamma1), 0, p.zsplit);
      else permutation_checks(cs, row, zrow, LookupShape(), p.num_zs, F(p.gamma0), F(p.gamma1), p.zsplit, p.num_zs);
    }
  } else if (KIND == 10) {  // FlagStark: no permutation pairs, segments 1-3 are empty
    if (PART == 0) flag_eval(cs, row, FlagShape(p.num_io));
  } else if (KIND == 11) {  // the u64 FlagStark
    if (PART == 0) flag_u64_eval(cs, row, FlagU64Shape(p.num_io));
  } else if (KIND == 7 || KIND == 8) {   // ModularStark / Fq12Stark: everything but the permutation checks is the head segment
    const OpShape sh(KIND);
    if (PART == 0) op_eval<KIND>(cs, row, sh);
    else if (PART == 2) {
      if (seg == 2) permutation_checks(cs, row, zrow, sh, p.num_zs, F(p.gamma0), F(p.gamma1), 0, p.zsplit);
      else permutation_checks(cs, row, zrow, sh, p.num_zs, F(p.gamma0), F(p.gamma1), p.zsplit, p.num_zs);
    }
  } else {
    constexpr int E = air_exp_e(KIND);
    ExpShape sh(E, p.num_io);
    // u16 range check (G1 / G2 / Fq tables), SBN_QUOTIENT_LOOKUPS=1 (experiment switch): the lookup constraints beside the permutation
    // checks, which load the same columns (air.cuh lookups_beside_permutation).  Measured in round 4: the tail segment loses 0.8 GB of
    // reads, but the permutation segments -- the longest of the three concurrent kernels -- get the work: 1.18 -> 1.25 ms for the stage.
    const bool moved = (E == 0 || E == 1 || E == 2) && p.lookups_in_perm;
    if (PART < 2) exp_eval<E>(cs, row, sh, (const ExpPiConsts<F>*)pic_arg, (PART == 1 && moved) ? 3 : 1 + PART);
    else {
      const int z0 = seg == 2 ? 0 : p.zsplit, z1 = seg == 2 ? p.zsplit : p.num_zs;
      permutation_checks(cs, row, zrow, sh, p.num_zs, F(p.gamma0), F(p.gamma1), z0, z1);
      if (moved) lookups_beside_permutation(cs, row, sh, p.num_zs, (z0 + 1) / 2, (z1 + 1) / 2);
    }
  }
#pragma unroll
  for (int j = 0; j < SBN_NCH; j++) p.part[((size_t)seg * SBN_NCH + j) * p.m + i] = cs.result(j).v;
}

// The order of these explicit instantiations is the kernels' order in the code object, and the order quotient_eval was measured with:
// the table kinds as launch_quotient_parts (prover.hip) lists them, its default (kind 4) last; PART 2, 1, 0 within a kind.
#define SBN_QUOTIENT_KIND(K)                                                                                                                \
  template __global__ void quotient_kernel<K, 2>(QuotientParams, const u64* __restrict__, const u64* __restrict__, const void* __restrict__); \
  template __global__ void quotient_kernel<K, 1>(QuotientParams, const u64* __restrict__, const u64* __restrict__, const void* __restrict__); \
  template __global__ void quotient_kernel<K, 0>(QuotientParams, const u64* __restrict__, const u64* __restrict__, const void* __restrict__);
SBN_QUOTIENT_KIND(1) SBN_QUOTIENT_KIND(2) SBN_QUOTIENT_KIND(3) SBN_QUOTIENT_KIND(5) SBN_QUOTIENT_KIND(6) SBN_QUOTIENT_KIND(7)
SBN_QUOTIENT_KIND(8) SBN_QUOTIENT_KIND(9) SBN_QUOTIENT_KIND(10) SBN_QUOTIENT_KIND(11) SBN_QUOTIENT_KIND(4)
#undef SBN_QUOTIENT_KIND
