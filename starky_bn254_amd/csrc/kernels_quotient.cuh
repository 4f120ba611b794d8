// K5, the part every launcher sees: the parameter block of the constraint / quotient kernels and the declaration of
// quotient_kernel<KIND, PART>.  Included by kernels.cuh (prover.hip launches the kernels) and by quotient.hip, which defines the
// template and instantiates its 33 forms: a minute of compile time that depends on nothing else in the prover.
#pragma once
#include "air.cuh"

struct QuotientParams {
  const u64* lde; const u64* zlde; size_t m; u32 next_step;
  // m = points evaluated.  Point j reads row j << row_log of matrices whose columns are lde_stride words apart: the quotient's
  // domain is every 2^(rate_bits - 1)-th row of the LDE (row_log = 0 and lde_stride = m at rate_bits 1 and on the trace domain).
  size_t lde_stride; u32 row_log;
  // Row sharding (all zero / equal to lde, zlde on one GPU): m = LOCAL point count, local point j is LDE point
  // (j << row_shift) | row_rho (tables xs / lag_* / zh_inv are indexed by the LDE point), its next row is local row
  // (j + next_step) mod m of lde_next / zlde_next.
  const u64* lde_next; const u64* zlde_next; u32 row_shift, row_rho;
  u32 seg_mask;     // segments whose kernels are launched (all four; a diagnostic switch for per-segment counter passes)
  const u64* xs; const u64* lag_first; const u64* lag_last;  // per LDE point
  u64 zh_inv[2];   // 1/Z_H on the two residues of i mod 2
  u64 last;        // g^-1
  u64 alpha[SBN_NCH];
  const u64* apow[SBN_NCH];
  u64 gamma0, gamma1;
  int num_zs, num_io;
  const void* pic;  // ExpPiConsts<F>*
  u64* qout;        // [SBN_NCH][m]
  u64* part;        // [QSEG segments][SBN_NCH][m] partial accumulators
  u64 seg_shift[4][SBN_NCH];  // alpha_j^(number of constraints that follow the segment)
  int seg_count[4];           // constraints of each segment (its first one is weighted alpha^(count-1) inside the segment)
  int zsplit;       // both permutation constraints of the Z columns [0, zsplit) go with segment 2, those of [zsplit, num_zs) with segment 3
  int lookups_in_perm;   // u16-range-check tables: the lookup constraints go with the permutation segments (their columns are loaded there anyway)
};

// The constraint stream is one Horner sum in alpha, so it splits exactly into four segments: 0 = AIR sections [1]-[8]
// (public inputs, transitions, flags, the add / double gadget), 1 = AIR sections [9]-[10] (io pulses, range check),
// 2 / 3 = the permutation checks of the first / second half of the Z columns (first-row constraint and transition of a column together);
// quotient_combine_kernel joins them as sum_s acc_s * alpha^(constraints after segment s).  With one lane per LDE point
// there are only two waves per SIMD at 2^17 points and one long dependent chain per lane (2.65 ms); four segments in
// flight give eight waves and quarter the chain (1.56 ms).  Each PART is its own kernel (0: segment 0, 1: segment 1,
// 2: segments 2 and 3 on grid.y) so that it gets its own register allocation -- as one kernel the gadget code of segment
// 0 set the VGPR count, and with it the occupancy, of the permutation checks too -- and the prover launches PART 0 + 1
// on its main stream and PART 2 on its second stream, so the parts still overlap.
// Tried and measured (profiles/r2_quotient_ab.txt): an XCD-aware order that runs the four segments of a 256-point block
// back to back on one XCD: traffic 7.50 -> 6.81 GB per launch but 1.56 -> 2.13 ms (tail imbalance); the re-reads were
// not between segments but inside segment 0 (3.0 GB for 0.45 GB of columns: every limb re-read for each convolution
// coefficient it feeds), which the factored gadgets of air.cuh removed (profiles/r2_quotient_segments.txt).
static constexpr u32 QSEG = 4;
// Declared only: no unit but quotient.hip can instantiate it (as ntt_fast_pass_kernel of kernels_ntt.cuh and ntt.hip).
template <int KIND, int PART>
__global__ void quotient_kernel(QuotientParams p, const u64* __restrict__ apow0, const u64* __restrict__ apow1, const void* __restrict__ pic_arg);
