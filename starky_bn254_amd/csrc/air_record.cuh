// The RECORDING form of the constraint consumer (include/sbn.h, sbn_explain_*): the evaluators of air.cuh, untouched, run over
// a distinct element type RF -- a base-field element with the same operators and lift -- for which Cons is specialised below.
// Cons<F> and Cons<E2>, which the prover, the verifier and the trace check instantiate, are not edited and gain no member.
//
// Every emission of an evaluator -- one call of c / ct / cf / cl (a single constraint) or of merge (a gadget's local sum over
// `count` consecutive constraints) -- is one BLOCK.  The sequence of emissions depends on (kind, num_io) only.  Where Cons<F>
// adds the emission to its two running sums, the recording form reduces the emission's own contribution, x alpha_j^rem or
// filter h_j alpha_j^rem, for both challenges and notes "block b is non-zero on this row" when either is; the weights only
// scale, so a block is flagged exactly when the fold of its own constraints is non-zero under one of the challenges.
// RF uses the generic Acc (one canonical multiply and add per term): the unreduced accumulators of Acc<F> are tied to F.
#pragma once
#include "air.cuh"

struct RF {
  F f;
  GL_HD RF() {}
  GL_HD explicit RF(F x) : f(x) {}
};
GL_HD RF operator+(RF a, RF b) { return RF(a.f + b.f); }
GL_HD RF operator-(RF a, RF b) { return RF(a.f - b.f); }
GL_HD RF operator-(RF a) { return RF(-a.f); }
GL_HD RF operator*(RF a, RF b) { return RF(a.f * b.f); }
GL_HD RF& operator+=(RF& a, RF b) { a = a + b; return a; }
GL_HD RF& operator-=(RF& a, RF b) { a = a - b; return a; }
GL_HD RF& operator*=(RF& a, RF b) { a = a * b; return a; }
template <> GL_HD RF lift<RF>(u64 v) { return RF(F(v)); }
static_assert(sizeof(RF) == sizeof(u64), "tables of F are read as tables of RF");

// Where the "non-zero" notes of one row go.  Exactly one of the three sinks is set:
//   counts  (host)          counts[b] = constraints of block b: the block table of a table, recorded over a zero row;
//   bits    (host, device)  bit b of this row's own bitmap;
//   stats   (device)        stats[b] += failing rows, stats[nblk + b] = min(failing row), over the whole trace: the emission
//                           sequence is the same in every lane, so the wave ballots the bit and ONE lane -- the first failing
//                           one, whose row is the wave's smallest -- issues one atomicAdd of the population count and one
//                           atomicMin per (wave, failing block); a clean block costs no memory operation.
template <>
struct Cons<RF> {
  RF alpha[SBN_NCH];
  int rem;
  const RF* apow[SBN_NCH];
  RF z_last, l_first, l_last;
  int blk;                        // emissions so far = the index of the next block
  u32* counts;
  unsigned char* bits;
  unsigned long long* stats; u32 nblk;
  unsigned long long rowi;        // the row of this lane
  bool live;                      // false: a padding lane (it evaluates a valid row, and notes nothing)
  GL_HD void start(int n) { rem = n; blk = 0; }
  GL_HD void note(bool nz, int count) {
#if defined(__HIP_DEVICE_COMPILE__)
    nz = nz && live && (u32)blk < nblk;   // (the block count is recorded from this very evaluator: the bound is a guard, not a case)
    if (stats) {
      const unsigned long long b = __ballot(nz);
      if (b && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) {
        atomicAdd(&stats[blk], (unsigned long long)__popcll(b));
        atomicMin(&stats[nblk + blk], rowi);
      }
    } else if (nz) bits[blk >> 3] |= (unsigned char)(1u << (blk & 7));
#else
    if (counts) counts[blk] = (u32)count;
    else if (nz) bits[blk >> 3] |= (unsigned char)(1u << (blk & 7));
#endif
    ++blk;
  }
  GL_HD void c(RF x) {
    --rem;
    note((x * apow[0][rem]).f.v != 0 || (x * apow[1][rem]).f.v != 0, 1);
  }
  GL_HD void ct(RF x) { c(x * z_last); }
  GL_HD void cf(RF x) { c(x * l_first); }
  GL_HD void cl(RF x) { c(x * l_last); }
  GL_HD void merge(const RF* h, RF filter, int count) {
    rem -= count;
    note((filter * h[0] * apow[0][rem]).f.v != 0 || (filter * h[1] * apow[1][rem]).f.v != 0, count);
  }
};
static_assert(SBN_NCH == 2, "Cons<RF> reduces two challenges");

// One row through the evaluator of table `KIND` (the sbn_air_kind values), the whole AIR stream in emission order.
// cs: alpha, apow, the selectors and a sink set by the caller; pic: the ExpPiConsts of the Exp tables (read as RF).
template <int KIND, class Row>
GL_HD void record_row(Cons<RF>& cs, const Row& row, int num_io, int nconstraints, const void* pic) {
  cs.start(nconstraints);
  if (KIND == 1) g1op_eval(cs, row);
  else if (KIND == 9) lookup_eval(cs, row);
  else if (KIND == 10) flag_eval(cs, row, FlagShape(num_io));
  else if (KIND == 11) flag_u64_eval(cs, row, FlagU64Shape(num_io));
  else if (KIND == 7 || KIND == 8) op_eval<KIND>(cs, row, OpShape(KIND));
  else {
    constexpr int E = air_exp_e(KIND);
    exp_eval<E>(cs, row, ExpShape(E, num_io), (const ExpPiConsts<RF>*)pic, 0);
  }
}
