// Host-side pieces shared by the prover and verifier: error reporting, the Fiat-Shamir transcript
// (plonky2 iop/challenger.rs `Challenger`, duplex/overwrite mode), FRI parameters
// (fri/reduction_strategies.rs ConstantArityBits) and the table shapes.
#pragma once
#include "../../include/sbn.h"
#include "poseidon.cuh"
#include "air.cuh"
#include <string>
#include <vector>
#include <cstdarg>
#include <cstdio>
#include <functional>

namespace sbn {

extern thread_local std::string g_last_error;
static inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_last_error = buf;
  return code;
}

static constexpr u64 PROOF_MAGIC = 0x31564f5250424e53ULL;  // "SNBPROV1"

struct Challenger {
  F st[12];
  std::vector<F> in, out;
  Challenger() { for (auto& x : st) x = F(0); }
  void duplex() {
    for (size_t i = 0; i < in.size(); i++) st[i] = in[i];
    in.clear();
    poseidon_permute(st);
    out.assign(st, st + P_RATE);
  }
  void observe(F e) { out.clear(); in.push_back(e); if (in.size() == (size_t)P_RATE) duplex(); }
  void observe(E2 e) { observe(e.a); observe(e.b); }
  void observe_words(const u64* w, size_t n) { for (size_t i = 0; i < n; i++) observe(F(w[i])); }
  F challenge() {
    if (!in.empty() || out.empty()) duplex();
    F r = out.back(); out.pop_back(); return r;
  }
  E2 ext_challenge() { F a = challenge(); F b = challenge(); return E2(a, b); }
};

struct FriShape {
  std::vector<u32> arity_bits;  // per reduction layer
  u32 degree_bits, rate_bits, cap_height;
  u32 lde_bits() const { return degree_bits + rate_bits; }
  u32 total_arity() const { u32 s = 0; for (auto a : arity_bits) s += a; return s; }
  size_t final_poly_len() const { return (size_t)1 << (degree_bits - total_arity()); }
};
static inline FriShape fri_shape(const sbn_config& c, u32 degree_bits) {
  FriShape f; f.degree_bits = degree_bits; f.rate_bits = c.rate_bits; f.cap_height = c.cap_height;
  u32 d = degree_bits;
  while (d > c.fri_final_poly_bits && d + c.rate_bits - c.fri_arity_bits >= c.cap_height) { f.arity_bits.push_back(c.fri_arity_bits); d -= c.fri_arity_bits; }
  return f;
}

struct AirShape {
  int kind; u32 num_io;
  size_t ncols, npi, npairs, nzs, nconstraints;
};
static inline bool air_shape(const sbn_air_desc* air, const sbn_config* cfg, AirShape& s) {
  if (!air) return false;
  s.kind = air->kind; s.num_io = air->num_io;
  u32 nch = cfg ? cfg->num_challenges : 2;
  if (air->kind == SBN_AIR_G1_OP) {
    s.ncols = G1OpShape::NUM_COLS; s.npi = 0; s.npairs = G1OpShape::NUM_PAIRS; s.nconstraints = G1OpShape::NUM_CONSTRAINTS;
  } else if (air->kind == SBN_AIR_MODULAR || air->kind == SBN_AIR_FQ12_MUL) {
    OpShape sh(air->kind);
    s.ncols = sh.num_cols(); s.npi = 0; s.npairs = sh.num_pairs(); s.nconstraints = sh.num_constraints();
  } else if (air->kind == SBN_AIR_LOOKUP) {
    s.ncols = LookupShape::NUM_COLS; s.npi = 0; s.npairs = LookupShape::NUM_PAIRS; s.nconstraints = LookupShape::NUM_CONSTRAINTS;
  } else if (air->kind == SBN_AIR_FLAGS) {
    if (air->num_io == 0 || air->num_io > (u32)G1EXP_MAX_IO || (air->num_io & (air->num_io - 1))) return false;
    FlagShape sh((int)air->num_io);
    s.ncols = sh.num_cols(); s.npi = 0; s.npairs = 0; s.nconstraints = sh.num_constraints();
  } else if (air->kind == SBN_AIR_FLAGS_U64) {
    if (air->num_io < 4 || air->num_io > 4 * (u32)G1EXP_MAX_IO || (air->num_io & (air->num_io - 1))) return false;
    FlagU64Shape sh((int)air->num_io);
    s.ncols = sh.num_cols(); s.npi = 0; s.npairs = 0; s.nconstraints = sh.num_constraints();
  } else if (air->kind == SBN_AIR_G1_EXP || air->kind == SBN_AIR_G2_EXP || air->kind == SBN_AIR_FQ12_EXP || air->kind == SBN_AIR_FQ_EXP || air->kind == SBN_AIR_FQ12_EXP_U64) {
    if (air->num_io == 0 || air->num_io > (u32)G1EXP_MAX_IO || (air->num_io & (air->num_io - 1))) return false;
    ExpShape sh(air_exp_e(air->kind), (int)air->num_io);
    s.ncols = sh.num_cols; s.npi = sh.num_pi; s.npairs = sh.num_pairs(); s.nconstraints = sh.num_constraints();
  } else return false;
  // num_permutation_batches = ceil(pairs*num_challenges / (constraint_degree-1)), constraint_degree = 3
  s.nzs = (s.npairs * nch + 1) / 2;
  return true;
}
static inline bool is_op_air(int kind) { return kind == SBN_AIR_MODULAR || kind == SBN_AIR_FQ12_MUL; }   // OpShape tables (air.cuh)
static inline bool is_exp_air(int kind) { return kind == SBN_AIR_G1_EXP || kind == SBN_AIR_G2_EXP || kind == SBN_AIR_FQ12_EXP || kind == SBN_AIR_FQ_EXP || kind == SBN_AIR_FQ12_EXP_U64; }
static inline size_t exp_rows_per_instance(int kind) { return (kind == SBN_AIR_FQ12_EXP_U64 || kind == SBN_AIR_FLAGS_U64) ? 128 : 512; }   // (FLAGS: 512)
// The word counts of an Exp table, the only place that states them.  An instance row of the `ios` arrays of include/sbn.h is x[xw]
// offset[xw] exp_val[ew] u32 words; a term (`terms`, `starts`) is such a row without its offset.  The public inputs of one instance
// (g1_exp_io_to_columns, src/curves/g1/exp.rs:124-135, and its twins) are x[W] offset[W] exp[EW] output[W]: u32 limbs on the curves
// and in Fq, 16-bit limbs in Fq12 (exponent: eight u32 limbs, or one u64 in FQ12_EXP_U64).
struct PiLayout {
  size_t W, EW, xw, ew;   // W / EW: public inputs per value / exponent; xw / ew: u32 words of the same in an instance row of `ios`
  bool limb16;
  int E;                  // 1 / 2 on the curves (G1 / the twist), 0 in the fields
  size_t per() const { return 3 * W + EW; }
  size_t T() const { return xw + ew; }
  size_t IOW() const { return 2 * xw + ew; }
  int values() const { return (int)(xw / 8); }   // Fq elements of a value
  bool field() const { return xw && !E; }        // a field Exp table (FQ_EXP, FQ12_EXP, FQ12_EXP_U64)
};
static inline bool pi_layout(int kind, PiLayout& L) {
  switch (kind) {
    case SBN_AIR_G1_EXP: L = {16, 8, 16, 8, false, 1}; return true;
    case SBN_AIR_G2_EXP: L = {32, 8, 32, 8, false, 2}; return true;
    case SBN_AIR_FQ_EXP: L = {8, 8, 8, 8, false, 0}; return true;
    case SBN_AIR_FQ12_EXP: L = {192, 8, 96, 8, true, 0}; return true;
    case SBN_AIR_FQ12_EXP_U64: L = {192, 1, 96, 2, true, 0}; return true;
    default: L = {0, 0, 0, 0, false, 0}; return false;
  }
}
static inline PiLayout pi_layout(int kind) { PiLayout L; pi_layout(kind, L); return L; }
static inline PiLayout curve_layout(int E) { return pi_layout(E == 1 ? SBN_AIR_G1_EXP : SBN_AIR_G2_EXP); }   // E = 1 / 2
// u32 words of one instance in `ios` (0: not an Exp table)
static inline size_t exp_io_words(int kind) { return pi_layout(kind).IOW(); }
// a value (xw u32 words) as the W public inputs that carry it, and an exponent (ew words) as its EW
static inline void value_to_pi(const PiLayout& L, const uint32_t* w, uint64_t* out) {
  if (!L.limb16) { for (size_t i = 0; i < L.W; i++) out[i] = w[i]; return; }
  for (size_t i = 0; i < L.W; i++) out[i] = (w[i >> 1] >> (16 * (i & 1))) & 0xffff;
}
static inline void exp_to_pi(const PiLayout& L, const uint32_t* w, uint64_t* out) {
  if (L.EW == 1) { out[0] = (uint64_t)w[0] | ((uint64_t)w[1] << 32); return; }
  for (size_t i = 0; i < L.EW; i++) out[i] = w[i];
}
// the inverses: false and *bad = the index of the first public input wider than its limb (a u64 exponent takes any word)
static inline bool value_from_pi(const PiLayout& L, const uint64_t* p, uint32_t* w, size_t* bad) {
  const uint64_t lim = L.limb16 ? 0xffffULL : 0xffffffffULL;
  for (size_t i = 0; i < L.W; i++) if (p[i] > lim) { *bad = i; return false; }
  if (!L.limb16) for (size_t i = 0; i < L.W; i++) w[i] = (uint32_t)p[i];
  else for (size_t i = 0; i < L.xw; i++) w[i] = (uint32_t)(p[2 * i] | (p[2 * i + 1] << 16));
  return true;
}
static inline bool exp_from_pi(const PiLayout& L, const uint64_t* p, uint32_t* w, size_t* bad) {
  if (L.EW == 1) { w[0] = (uint32_t)p[0]; w[1] = (uint32_t)(p[0] >> 32); return true; }
  for (size_t i = 0; i < L.EW; i++) { if (p[i] > 0xffffffffULL) { *bad = i; return false; } w[i] = (uint32_t)p[i]; }
  return true;
}
static inline ExpShape exp_shape(const AirShape& a) { return ExpShape(air_exp_e(a.kind), (int)a.num_io); }
// the columns of permutation pair z of a table (air.cuh air_pair)
static inline void air_pair(const AirShape& a, size_t z, int& l, int& r) { air_pair(a.kind, exp_shape(a), (int)z, l, r); }
// The shape-constant columns [f0, f1) of a table: functions of the row index, the height and num_io alone, so every trace the
// generators write for one shape holds the same words there.  Exp tables: the periodic pulse (counter and witness; absent in the u64
// table), the io-pulse counter, 2 num_io (witness, pulse) pairs and the range check's table column -- what tg::periodic_kernel and
// tg::io_pulse_kernel write without reading the instance list.  Every other table: empty.
static inline void fixed_columns_range(const AirShape& a, size_t& f0, size_t& f1) {
  f0 = f1 = 0;
  if (!is_exp_air(a.kind)) return;
  const ExpShape sh = exp_shape(a);
  f0 = (size_t)(sh.start_periodic >= 0 ? sh.start_periodic : sh.start_io_pulses);
  f1 = (size_t)sh.start_lookups + 1;
}
// the last entry of that table column (tracegen.hip: 0 .. max, then max repeated): the split range check's table has 256 entries
static inline u64 exp_table_max(const ExpShape& sh) { return sh.split_rc ? 255 : 65535; }
// rate_bits: 1 (standard_fast_config) and 3 (plonky2's standard_recursion_config, the blowup of 8).  The code is general in
// rate_bits >= 1; 2 is exercised through sbn_commit_values only and stays refused here (include/sbn.h).
static inline bool config_supported(const sbn_config* c) {
  return c && c->num_challenges == SBN_NCH && (c->rate_bits == 1 || c->rate_bits == 3) && c->cap_height >= 1 && c->cap_height <= 8 &&
         c->fri_arity_bits >= 1 && c->fri_arity_bits <= 4 && c->num_query_rounds >= 1 && c->num_query_rounds <= 512 &&
         c->proof_of_work_bits <= 32 && c->fri_variant <= SBN_FRI_PLAIN;
}
// The largest LDE a prover or a device verifier is created for: 2^23 points (2^22 rows at rate_bits 1, 2^20 at rate_bits 3).
static constexpr u32 SBN_MAX_LDE_BITS = 23;
static inline bool height_supported(const sbn_config* c, u32 degree_bits) { return degree_bits >= 9 && degree_bits + c->rate_bits <= SBN_MAX_LDE_BITS; }
// Device witness generation of the u16-range-check tables (G1_EXP, G2_EXP, FQ_EXP): the table column 0..65535 needs 2^16 rows; above
// that every height a context can be created for (the kernels are written for n <= 2^22, the largest trace any config admits).  The
// one predicate of trace_gate, derived_columns_covered (tracegen_device.hip) and sbn_prover_diff_witness (witness_diff.hip).
static inline bool u16_device_witness_covers(size_t n) { return n >= 65536 && n <= ((size_t)1 << (SBN_MAX_LDE_BITS - 1)); }
static constexpr const char* U16_DEVICE_WITNESS_ROWS = "covers 2^16 .. 2^22 rows";
static constexpr const char* HEIGHT_REFUSAL = "degree_bits out of range (9 <= degree_bits and degree_bits + rate_bits <= 23: the largest LDE is 2^23 points)";
// sbn_config.fri_variant: 0 selects the default (the 0.1.x line: final polynomial times X)
static inline u32 fri_times_x(const sbn_config& c) { return c.fri_variant == SBN_FRI_PLAIN ? 0u : 1u; }

// tracegen.hip: Jacobian curve chains of every G1ExpStark instance on host threads (layout: bn254w.cuh g1_chains)
int tracegen_host_chains(int E, const uint32_t* ios, size_t K, u64* ja, u64* jb, int form = 0);   // form: tracegen.hip
// tracegen.hip: square-and-multiply chains of every Fq12ExpStark / Fq12ExpU64Stark instance, standard form, [K][steps+1][12][4] each
int tracegen_host_chains_fq12(const uint32_t* ios, size_t iow, int steps, size_t K, u64* ca, u64* cb);
// the same for FqExpStark: [K][257][4] each
int tracegen_host_chains_fq(const uint32_t* ios, size_t K, u64* ca, u64* cb);
// tracegen.hip: threads of the host worker pool (the caller's included): SBN_HOST_THREADS, else one per visible CPU (<= 64)
unsigned tracegen_host_threads();
// tracegen.hip: f(0) .. f(n - 1) on that pool (the caller's thread takes part; a call from inside a pool task runs serially)
void host_parallel_for(size_t n, const std::function<void(size_t)>& f);
// tracegen.hip: the columns [num_main, num_columns) of an Exp table of n rows from its main columns in `trace` (column-major), by
// the code the host generators end with: the pulses, then the u16 or the split range check.  false: a range-checked column holds a
// word >= 2^16
bool derived_columns_host(const ExpShape& sh, uint64_t* trace, size_t n);
// trace_load.hip: the refusals of sbn_prove_rows that need no prover (include/sbn.h, the list at sbn_host_rows, 1 .. 8), and
// *degree_bits_out = log2 of the row count
int host_rows_precheck(const sbn_air_desc* air, const sbn_host_rows* rows, uint32_t flags, const uint64_t* pi, size_t n_pi, uint32_t* degree_bits_out);
// tracegen.hip: the curve chains run eight instances per AVX-512 IFMA register on this CPU (0.15 ms per group of eight)
bool tracegen_host_chains_vectorized();
// The instance-list units (instance_lists.hpp says what they share), as tracegen_device.hip and capi.hip call them.
// chain_instances.hip: sbn_chain_instances behind its argument checks, and its refusals alone for the curve tables
int chain_instances_host(int kind, const uint32_t* terms, size_t K, const uint32_t* start, uint32_t* ios, uint32_t* final_out);
int chain_terms_check_curve(int E, const uint32_t* terms, size_t K, const uint32_t* start);
// scalar_mul.hip (E = 1 / 2): the generator ([16E] u32) and 2p - r; the refusals of the points and the offset; the explicit list of
// `total` >= count rows; SBN_ERR_WITNESS naming the first of K instances the table cannot walk (SBN_OK: none); product = output +
// (-offset) for K affine outputs ([K][16E] u32; flag 1 and zero words = infinity)
const uint32_t* curve_generator_words(int E);
const uint32_t* g2_cofactor_words();
const uint32_t* curve_start_candidate_words(int E, unsigned j);   // sbn_start_candidate, j < SBN_START_CANDIDATES
int scalar_mul_check_points(int E, const uint32_t* points, size_t count, const uint32_t* offset);
void scalar_mul_explicit_list(int E, const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t count, size_t total,
                              const uint32_t* offset, uint32_t* ios);
int scalar_mul_name_degenerate(int E, const uint32_t* ios, size_t K);
void scalar_mul_unoffset_host(int E, const uint32_t* outputs, const uint32_t* offset, size_t K, uint32_t* products, uint8_t* infinity);
// powers.hip: the refusals of the bases and exponents of a field Exp table, naming the tower
int power_check_inputs(int kind, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count);
// program.hip (include/sbn.h, "Field programs"): refusals 1 to 4 of the header in its order, and the schedule: level[g], and the
// nodes sorted by level (order; the nodes of level l are order[level_start[l] .. level_start[l + 1]), in node order)
struct ProgramPlan {
  std::vector<uint32_t> level, order, level_start;
  size_t depth() const { return level_start.size() - 1; }
};
int program_plan(int kind, const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values, const uint32_t* exps, size_t n_exps,
                 size_t num_io, ProgramPlan& plan, const uint32_t* maps = nullptr);
// sbn_program_instances / sbn_program_m_instances: maps (optional, [count]) = the fourth word of every sbn_program_node_m
int program_instances(int kind, const sbn_program_node* nodes, const uint32_t* maps, size_t count, const uint32_t* values, size_t n_values,
                      const uint32_t* exps, size_t n_exps, size_t num_io, uint32_t* ios_out, uint32_t* outs_out);
// curve_program.hip (include/sbn.h, "Curve programs"): refusals 1 to 4 of the header in its order and the schedule of
// sbn_program_levels as a ProgramPlan; the negated blinds -T_g of the nodes from candidate `choice` ([count][16E] u32 affine words,
// zero where flag[g] = 1: T_g is the point at infinity), level by level on the host pool
int curve_program_plan(int kind, const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points, const uint32_t* exps, size_t n_exps,
                       size_t num_io, ProgramPlan& plan);
void curve_program_neg_blinds(int E, const ProgramPlan& plan, const sbn_program_node* nodes, const uint32_t* exps, unsigned choice, uint32_t* neg_blinds,
                              uint8_t* flag);
// msm_batch.hip (segmented chained lists; a chained list is one segment): the argument refusals in the header's order (a null
// `*starts` becomes the generator / one with *start_count = 1; *M_out = the sum of the lengths); the refusals of the values, naming
// the global instance and its segment; the derivation of `total` >= M rows of ios (rows past M repeat row M - 1), the finals and on
// the curves the sums and their flags -- segmented_derive sets NO message: false and *why = what it cannot derive and the global
// instance, for the entry point to word; msm_batch_derive = the refusals of the values, the derivation and the segmented wording
struct ListRefusal { enum What { OFFSET_AT_INFINITY = 1, OUTPUT_AT_INFINITY, DEGENERATE_WALK, UNNAMED_WALK } what; size_t at; };
int msm_batch_check_args(int kind, const void* terms, const uint64_t* lengths, size_t segments, const uint32_t** starts, size_t* start_count, size_t num_io,
                         const void* sums_out, const void* infinity_out, size_t* M_out);
int msm_batch_check_inputs(int kind, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts, size_t start_count, size_t M);
bool segmented_derive(int kind, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts, size_t start_count, size_t M,
                      size_t total, uint32_t* ios, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out, ListRefusal* why);
int msm_batch_derive(int kind, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts, size_t start_count, size_t M,
                     size_t total, uint32_t* ios, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out);
// msm_batch.hip, the complete sums (include/sbn.h, "Complete sums"; G1_EXP / G2_EXP only).  msm_batch_complete_args: the refusals of
// the kind and the arguments, *M_out as above.  msm_batch_effective_terms: terms_eff [M][T] = the caller's terms with (generator,
// exponent 0) where term_infinity says so (those words are not read), then the refusals of the values.  msm_batch_complete_choose:
// per segment the smallest start candidate the table's walk takes (every failing segment of a candidate found in one pass), the
// list of `total` >= M rows, and what msm_batch_derive gives on (terms_eff, starts_out); SBN_ERR_WITNESS when a segment exhausts the
// candidates.  Every output pointer is optional.
int msm_batch_complete_args(int kind, const void* terms, const uint64_t* lengths, size_t segments, size_t num_io, size_t* M_out);
int msm_batch_effective_terms(int kind, const uint32_t* terms, const uint8_t* term_infinity, const uint64_t* lengths, size_t segments, size_t M, uint32_t* terms_eff);
int msm_batch_complete_choose(int kind, const uint32_t* terms_eff, const uint64_t* lengths, size_t segments, size_t M, size_t total, uint32_t* ios,
                              uint32_t* starts_out, uint8_t* choice_out, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out);
// prover.hip: device memory the context allocated, in bytes (the one-shot cache of capi.hip counts it against its budget)
size_t prover_device_bytes(const sbn_prover* p);
// prover.hip: the device sbn_set_device / sbn_set_thread_device selected for the calling thread (else the process default)
int current_device();
// prover.hip: SBN_ERR_NO_DEVICE ("no HIP device available: <why>") unless the process has a HIP device; else current_device() becomes
// HIP's current device of the calling thread
int use_current_device(const char* why);

}  // namespace sbn

struct sbn_proof {
  std::vector<u64> words;
  u32 degree_bits;
};
