// What the host forms of the trace diagnostics share (defined in trace_check.hip): the argument checks, and the state a host check
// or a host explain evaluates its rows against.  Included by trace_check.hip, trace_explain.hip and perm_diff.hip.
#pragma once
#include "host_common.hpp"

// Everything but the flags is set by host_setup; the pointers look into the caller's trace and into the HostStore beside it.
struct HostCheck {
  sbn::AirShape as; size_t n; u32 degree_bits;
  const u64* trace; const u64* zval;   // [ncols][n], [nzs][n]
  F gamma0, gamma1, alpha[SBN_NCH];
  const F* apow[SBN_NCH];
  const ExpPiConsts<F>* pic;
  int seg_count[4]; int zsplit;        // the segments of the quotient stage (prover.hip quotient_segments)
  uint8_t* flags;
};
// What a host form owns while it runs: the alpha powers, the public-input constants of the Exp tables, the Z columns.
struct HostStore { std::vector<F> apow[SBN_NCH]; std::vector<ExpPiConsts<F>> pic; std::vector<u64> zval; };
static constexpr size_t HOST_TILE = 64;   // rows of one task of the whole-trace forms
// Tables and heights as sbn_prover_create accepts them
int host_table_check(const sbn_air_desc* air, uint32_t degree_bits, sbn::AirShape& as);
// The canonical-form scan on the host pool, SBN_ERR_NON_CANONICAL naming the smallest index
int host_canonical_check(const uint64_t* trace, size_t words);
// The argument checks of the host forms after their own null checks (the table, the public inputs, canonical form), then the
// challenges of `seed`, the alpha tables and Z
int host_setup(const sbn_air_desc* air, const uint64_t* trace, uint32_t degree_bits, const uint64_t* pi, size_t n_pi, uint64_t seed,
               HostCheck& hc, HostStore& hs);
