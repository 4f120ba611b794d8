// Explain (include/sbn.h, sbn_air_constraint_blocks / sbn_prover_explain_* / sbn_explain_*_host): which constraint BLOCKS the rows
// of a trace break, through the RECORDING consumer of air_record.cuh.  First the block table of a table, then the two forms.
// Device form: one thread per trace row reads the column-major d_trace as the check kernels do (row i against row
// i + 1 mod N, lanes = consecutive rows: coalesced) and runs the table's evaluator of air.cuh through the recording consumer.
// The emission sequence is the same in every lane, so in the whole-trace form a wave ballots the "non-zero" bit
// of every block and one lane issues one atomicAdd and one atomicMin per (wave, failing block): a trace on which every row
// fails costs one pair of atomics per wave and block, a clean block nothing.  The listed-rows form runs the same code with
// uncoalesced loads (the list is short) and every thread sets bits in the bitmap of its own row.
// The Z columns need no evaluator: a second kernel forms (Z_z - 1) L_first and the transition of every (row, z) directly.
// Shared with the check (trace_check.hip): the way in and the TraceDomain setup -- challenges, Z, the tables of H, the alpha tables.
// Scratch is per-proof scratch only: the tables of H in d_zpow, the statistics in d_open / h_open, the listed rows and their
// bitmaps in d_part (free once Z is written); a context that never explains allocates nothing for it.
// Host form: the setup of the host check (trace_host.hpp: the same argument checks, challenges and Z), then the same evaluators
// through the recording consumer over host rows, the Z columns by the same two expressions.
#include "prover_ctx.hpp"
#include "trace_host.hpp"
#include "kernels_explain.cuh"

// ---- the block table --------------------------------------------------------------------------------------------------------
// RECORDED, not counted by hand: the evaluator of the table runs once over a zero row and leaves the constraint count of every
// emission; what each emission is (section, instance, columns) is attached from the table's Shape by walking the evaluator's
// sections in their order, and a walk whose length differs from the recorded one is an error, not a table.
enum BlockSection {
  BS_OUTPUT_PULSE_SUM, BS_PUBLIC_INPUTS, BS_TRANSITION_DOUBLE, BS_TRANSITION_ADD, BS_TRANSITION_HOLD, BS_FLAGS, BS_GADGET_ADD,
  BS_GADGET_DOUBLE, BS_GADGET_SQ, BS_GADGET_MUL, BS_FLAGS_REPEAT, BS_ROTATION_PULSE, BS_IO_PULSE, BS_RC_RECOMPOSITION, BS_RC_LOOKUP,
  BS_RANGE_TABLE, BS_LOOKUP, BS_COUNT
};
static const char* SECTION_NAMES[BS_COUNT] = {
  "output_pulse_sum", "public_inputs", "transition_double", "transition_add", "transition_hold", "flags", "gadget_add",
  "gadget_double", "gadget_sq", "gadget_mul", "flags_repeat", "rotation_pulse", "io_pulse", "range_check_recomposition",
  "range_check_lookup", "range_table", "lookup"};
extern "C" const char* sbn_constraint_section_name(int s) { return (s >= 0 && s < (int)BS_COUNT) ? SECTION_NAMES[s] : ""; }

extern "C" int sbn_air_permutation_pair(const sbn_air_desc* air, size_t z, uint32_t* lhs_col, uint32_t* rhs_col) {
  AirShape as;
  if (!air || !lhs_col || !rhs_col) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (!air_shape(air, nullptr, as)) return fail(SBN_ERR_BAD_ARG, "unknown air kind / num_io");
  if (z >= as.nzs) return fail(SBN_ERR_BAD_ARG, "the table has %zu Z columns", as.nzs);
  int l, r;
  air_pair(as, z, l, r);
  *lhs_col = (uint32_t)l; *rhs_col = (uint32_t)r;
  return SBN_OK;
}

namespace {
struct RecRow {
  const u64* lv; const u64* nv;
  RF l(int c) const { return RF(F(lv[c])); }
  RF n(int c) const { return RF(F(nv[c])); }
};
struct ZeroRow {
  RF l(int) const { return RF(F(0)); }
  RF n(int) const { return RF(F(0)); }
};
template <class Row>
static void record_row_kind(int kind, Cons<RF>& cs, const Row& row, int num_io, int ncons, const void* pic) {
  for_air_kind(kind, [&](auto K) { record_row<decltype(K)::value>(cs, row, num_io, ncons, pic); });
}

struct BlockLabel { uint32_t section, instance, col_first, col_count; };
static constexpr uint32_t NO_INSTANCE = UINT32_MAX;
struct Labels {
  std::vector<BlockLabel> v;
  void add(uint32_t s, uint32_t inst, int c0, int cn) { v.push_back(BlockLabel{s, inst, (uint32_t)c0, (uint32_t)cn}); }
  // eval_split_u16_range_check over num_rc targets whose (lo, sorted lo, table, hi, sorted hi, table) columns start at mc + 1
  void split_range_check(int mc, int num_rc) {
    for (int i = 0; i < num_rc; i++) add(BS_RC_RECOMPOSITION, (uint32_t)i, mc + 1 + 6 * i, 6);
    for (int i = 0; i < num_rc; i++)
      for (int half = 0; half < 2; half++) { add(BS_RC_LOOKUP, (uint32_t)i, mc + 2 + 6 * i + 3 * half, 2); add(BS_RC_LOOKUP, (uint32_t)i, mc + 2 + 6 * i + 3 * half, 2); }
    for (int k = 0; k < 3; k++) add(BS_RANGE_TABLE, NO_INSTANCE, mc, 1);
  }
  // eval_pulse: the counter's two constraints, then two per position
  void io_pulses(int st, int positions) {
    add(BS_IO_PULSE, NO_INSTANCE, st, 1); add(BS_IO_PULSE, NO_INSTANCE, st, 1);
    for (int i = 0; i < positions; i++) { add(BS_IO_PULSE, (uint32_t)i, st + 1 + 2 * i, 2); add(BS_IO_PULSE, (uint32_t)i, st + 1 + 2 * i, 2); }
  }
};
// The emissions of the table's evaluator in their order (air.cuh g1op_eval, op_eval, lookup_eval, flag_eval, flag_u64_eval, exp_eval)
static void block_labels(const AirShape& as, Labels& L) {
  const int num_io = (int)as.num_io;
  if (as.kind == SBN_AIR_G1_OP) {
    typedef G1OpShape S;
    L.split_range_check(S::MAIN_COLS, S::NUM_RC);
    L.add(BS_GADGET_ADD, NO_INSTANCE, 0, S::MAIN_COLS - 2); L.add(BS_GADGET_DOUBLE, NO_INSTANCE, 0, S::MAIN_COLS - 2);
  } else if (is_op_air(as.kind)) {
    const OpShape S(as.kind);
    L.split_range_check(S.main_cols, S.num_rc);
    L.add(BS_GADGET_MUL, NO_INSTANCE, 0, S.main_cols - 1);
  } else if (as.kind == SBN_AIR_LOOKUP) {
    L.add(BS_LOOKUP, 0, 2, 2); L.add(BS_LOOKUP, 0, 2, 2);
  } else if (as.kind == SBN_AIR_FLAGS) {
    const FlagShape S(num_io);
    L.add(BS_OUTPUT_PULSE_SUM, NO_INSTANCE, FlagShape::START_IO_PULSES + 1, 4 * num_io);
    L.add(BS_FLAGS, NO_INSTANCE, 0, FlagShape::MAIN_COLS);
    for (int k = 0; k < 5; k++) L.add(BS_ROTATION_PULSE, (uint32_t)k, FlagShape::START_PERIODIC, 2);
    L.io_pulses(FlagShape::START_IO_PULSES, 2 * num_io);
  } else if (as.kind == SBN_AIR_FLAGS_U64) {
    L.add(BS_OUTPUT_PULSE_SUM, NO_INSTANCE, FlagU64Shape::MAIN_COLS + 1, 4 * num_io);
    L.add(BS_FLAGS, NO_INSTANCE, 0, FlagU64Shape::MAIN_COLS);
    L.io_pulses(FlagU64Shape::MAIN_COLS, 2 * num_io);
  } else {
    const ExpShape S = exp_shape(as);
    const bool field = S.E == 0 || S.E == 12 || S.E == 13;   // square-and-multiply tables: sq / mul where the curves double / add
    const int nflags = S.num_main - S.start_flags, gcols = S.start_flags - S.gadget_col, tcols = S.nx_col + S.W;
    L.add(BS_OUTPUT_PULSE_SUM, NO_INSTANCE, S.start_io_pulses + 1, 4 * num_io);                      // [1]
    L.add(BS_PUBLIC_INPUTS, NO_INSTANCE, 0, 2 * S.W);                                                  // [2]
    L.add(BS_TRANSITION_DOUBLE, NO_INSTANCE, 0, tcols); L.add(BS_TRANSITION_ADD, NO_INSTANCE, 0, tcols);   // [3]
    L.add(BS_TRANSITION_HOLD, NO_INSTANCE, 0, 2 * S.W);
    L.add(BS_FLAGS, NO_INSTANCE, S.start_flags, nflags);                                               // [4]
    if (field) { L.add(BS_GADGET_SQ, NO_INSTANCE, S.gadget_col, gcols); L.add(BS_GADGET_MUL, NO_INSTANCE, S.gadget_col, gcols); }   // [5] [6]
    else { L.add(BS_GADGET_ADD, NO_INSTANCE, S.gadget_col, gcols); L.add(BS_GADGET_DOUBLE, NO_INSTANCE, S.gadget_col, gcols); }
    L.add(BS_FLAGS_REPEAT, NO_INSTANCE, S.start_flags, nflags);                                        // [7]
    if (S.E != 13) for (int k = 0; k < 5; k++) L.add(BS_ROTATION_PULSE, (uint32_t)k, S.start_periodic, 2);   // [8]
    L.io_pulses(S.start_io_pulses, 2 * num_io);                                                        // [9]
    if (S.split_rc) L.split_range_check(S.start_lookups, S.num_rc);                                    // [10]
    else {
      for (int k = 0; k < S.num_rc; k++) { L.add(BS_RC_LOOKUP, (uint32_t)k, S.start_lookups + 1 + 2 * k, 2); L.add(BS_RC_LOOKUP, (uint32_t)k, S.start_lookups + 1 + 2 * k, 2); }
      for (int k = 0; k < 3; k++) L.add(BS_RANGE_TABLE, NO_INSTANCE, S.start_lookups, 1);
    }
  }
}
static int block_table(const AirShape& as, std::vector<sbn_constraint_block>& out) {
  const size_t ncons = as.nconstraints;
  std::vector<u32> counts(ncons + 1, 0);
  std::vector<F> ones(apow_len(ncons, as.nzs), F(1));
  std::vector<ExpPiConsts<F>> pic(is_exp_air(as.kind) ? 1 : 0);
  Cons<RF> cs{};
  for (int j = 0; j < SBN_NCH; j++) { cs.alpha[j] = RF(F(1)); cs.apow[j] = (const RF*)ones.data(); }
  cs.z_last = cs.l_first = cs.l_last = RF(F(0));
  cs.counts = counts.data();
  record_row_kind(as.kind, cs, ZeroRow(), (int)as.num_io, (int)ncons, pic.empty() ? nullptr : (const void*)pic.data());
  if (cs.rem != 0) return fail(SBN_ERR_BAD_ARG, "the evaluator emitted %zu constraints, not %zu", ncons - (size_t)cs.rem, ncons);
  Labels L;
  block_labels(as, L);
  if (L.v.size() != (size_t)cs.blk) return fail(SBN_ERR_BAD_ARG, "%zu block labels for %d emissions", L.v.size(), cs.blk);
  const size_t n_tail = is_exp_air(as.kind) ? (size_t)exp_shape(as).num_tail_constraints() : 0;
  out.resize((size_t)cs.blk);
  uint32_t first = 0;
  for (size_t b = 0; b < out.size(); b++) {
    out[b].first = first; out[b].count = counts[b];
    out[b].segment = first >= ncons - n_tail ? 1u : 0u;
    out[b].section = L.v[b].section; out[b].instance = L.v[b].instance; out[b].col_first = L.v[b].col_first; out[b].col_count = L.v[b].col_count;
    first += counts[b];
  }
  return SBN_OK;
}
}  // namespace

extern "C" size_t sbn_air_constraint_blocks(const sbn_air_desc* air, sbn_constraint_block* out, size_t cap) {
  AirShape as;
  if (!air_shape(air, nullptr, as)) { fail(SBN_ERR_BAD_ARG, "unknown air kind / num_io"); return 0; }
  std::vector<sbn_constraint_block> blocks;
  if (block_table(as, blocks)) return 0;
  if (out) for (size_t b = 0; b < blocks.size() && b < cap; b++) out[b] = blocks[b];
  return blocks.size();
}

// ---- device form ------------------------------------------------------------------------------------------------------------
// permutation.rs eval_permutation_checks for Z column z on row i: the first-row constraint or the transition is non-zero
__device__ __forceinline__ bool explain_z_nonzero(const ExplainParams& p, size_t i, int z, int lc, int rc) {
  const size_t n = p.n, inext = (i + 1) & (n - 1);
  const F g0(p.gamma0), g1(p.gamma1), one(1);
  const F l(p.trace[(size_t)lc * n + i]), r(p.trace[(size_t)rc * n + i]), zl(p.zval[(size_t)z * n + i]), zn(p.zval[(size_t)z * n + inext]);
  const F t = zn * ((r + g0) * (r + g1)) - zl * ((l + g0) * (l + g1));
  const F f = (zl - one) * F(p.lag_first[i]);
  return t.v != 0 || f.v != 0;
}
// whole-trace form: grid (n / 256, Z columns); the same ballot-and-atomic reduction as the blocks
__global__ __launch_bounds__(256) void explain_z_trace_kernel(ExplainParams p) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < p.n;
  const ExpShape es(air_exp_e(p.kind), p.num_io);
  for (int z = blockIdx.y; z < p.num_zs; z += gridDim.y) {
    int lc, rc;
    air_pair(p.kind, es, z, lc, rc);
    const bool nz = live && explain_z_nonzero(p, live ? i : 0, z, lc, rc);
    const unsigned long long b = __ballot(nz);
    if (b && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) {
      atomicAdd(&p.zstats[z], (unsigned long long)__popcll(b));
      atomicMin(&p.zstats[p.num_zs + z], (unsigned long long)i);
    }
  }
}
// listed-rows form: one thread per listed row walks the Z columns and owns the bytes it writes
__global__ __launch_bounds__(256) void explain_z_rows_kernel(ExplainParams p) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.n_rows) return;
  const size_t i = (size_t)p.rows[k];
  const ExpShape es(air_exp_e(p.kind), p.num_io);
  unsigned char* out = p.zbits + k * p.zbytes;
  for (int z0 = 0; z0 < p.num_zs; z0 += 8) {
    u32 byte = 0;
    for (int z = z0; z < z0 + 8 && z < p.num_zs; z++) {
      int lc, rc;
      air_pair(p.kind, es, z, lc, rc);
      if (explain_z_nonzero(p, i, z, lc, rc)) byte |= 1u << (z - z0);
    }
    out[z0 >> 3] = (unsigned char)byte;
  }
}

static void launch_explain_kernel(int kind, dim3 grid, hipStream_t st, const ExplainParams& ep, const u64* apow0, const u64* apow1, const void* pic) {
  for_air_kind(kind, [&](auto K) {
    constexpr int KIND = decltype(K)::value;
    if constexpr (KIND == 4 || KIND == 6 || KIND == 8) launch_explain_kernel_fq12(kind, grid, st, ep, apow0, apow1, pic);   // a unit of their own for the compile time
    else hipLaunchKernelGGL(explain_kernel<KIND>, grid, dim3(256), 0, st, ep, apow0, apow1, pic);
  });
}

// rows == null: the whole-trace form into bstats / zstats; else the listed-rows form into bflags / zflags
static int explain_device(sbn_prover* P, uint64_t seed, const uint64_t* rows, size_t n_rows, uint8_t* bflags, uint8_t* zflags,
                          sbn_block_stat* bstats, sbn_block_stat* zstats) {
  if (int rc = diag_enter(P, "explain", false)) return rc;
  hipStream_t st = P->stream;
  hipEvent_t* ev = P->ev;
  const size_t n = P->n, Z = P->air.nzs, C = P->air.ncols;
  for (size_t k = 0; k < n_rows; k++) if (rows[k] >= n) return fail(SBN_ERR_BAD_ARG, "row %llu of a trace of %zu rows", (unsigned long long)rows[k], n);
  const sbn_air_desc desc{P->air.kind, P->air.num_io};
  const size_t B = sbn_air_constraint_blocks(&desc, nullptr, 0);
  if (!B) return SBN_ERR_BAD_ARG;
  if (2 * (B + Z) > (C + Z + 4) * 4) return fail(SBN_ERR_UNSUPPORTED, "%zu blocks do not fit the scratch of this context", B);
  TraceDomain td;
  if (int rc = trace_domain_setup(P, seed, td)) return rc;

  ExplainParams ep{};
  ep.trace = P->d_trace; ep.zval = P->d_zval; ep.n = n;
  ep.xs = td.xs; ep.lag_first = td.lag_first; ep.lag_last = td.lag_last; ep.last = td.last;
  for (int j = 0; j < SBN_NCH; j++) ep.alpha[j] = td.alphas[j].v;
  ep.gamma0 = td.gamma0.v; ep.gamma1 = td.gamma1.v;
  ep.kind = P->air.kind; ep.num_io = (int)P->air.num_io; ep.nconstraints = (int)P->air.nconstraints; ep.num_zs = (int)Z;
  const u64 *apow0 = P->d_apow, *apow1 = P->d_apow + P->apow_n;
  ep.nblk = (u32)B; ep.bbytes = (u32)((B + 7) / 8); ep.zbytes = (u32)((Z + 7) / 8);

  if (!rows) {
    unsigned long long* d_stats = (unsigned long long*)P->d_open;   // [B counts][B first rows][Z counts][Z first rows]
    ep.stats = d_stats; ep.zstats = d_stats + 2 * B;
    HIPC(hipMemsetAsync(d_stats, 0, B * sizeof(u64), st));
    HIPC(hipMemsetAsync(d_stats + B, 0xff, B * sizeof(u64), st));
    if (Z) {
      HIPC(hipMemsetAsync(ep.zstats, 0, Z * sizeof(u64), st));
      HIPC(hipMemsetAsync(ep.zstats + Z, 0xff, Z * sizeof(u64), st));
    }
    launch_explain_kernel(ep.kind, dim3((unsigned)((n + 255) / 256)), st, ep, apow0, apow1, P->d_pic);
    HIPC(hipGetLastError());
    if (Z) {
      hipLaunchKernelGGL(explain_z_trace_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)std::min<size_t>(Z, 65535)), dim3(256), 0, st, ep);
      HIPC(hipGetLastError());
    }
    HIPC(hipEventRecord(ev[2], st));
    HIPC(hipMemcpyAsync(P->h_open, d_stats, 2 * (B + Z) * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPC(hipEventRecord(ev[3], st));
    HIPC(hipStreamSynchronize(st));
    const u64* h = P->h_open;
    for (size_t b = 0; b < B; b++) bstats[b] = sbn_block_stat{h[b], h[B + b]};
    if (zstats) for (size_t z = 0; z < Z; z++) zstats[z] = sbn_block_stat{h[2 * B + z], h[2 * B + Z + z]};
  } else {
    // the listed rows and their bitmaps in d_part (64 n words; Z is written, the chunk products of launch_perm_z are done with it
    // on this stream), a chunk of the list at a time
    const size_t per_row = sizeof(u64) + ep.bbytes + ep.zbytes, room = (size_t)64 * n * sizeof(u64);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(room / per_row, 65536));
    for (size_t k0 = 0; k0 < n_rows; k0 += chunk) {
      const size_t cnt = std::min(chunk, n_rows - k0);
      u64* d_rows = P->d_part;
      unsigned char* d_bits = (unsigned char*)(d_rows + cnt);
      unsigned char* d_zbits = d_bits + cnt * ep.bbytes;
      HIPC(hipMemcpyAsync(d_rows, rows + k0, cnt * sizeof(u64), hipMemcpyHostToDevice, st));
      HIPC(hipMemsetAsync(d_bits, 0, cnt * (ep.bbytes + ep.zbytes), st));
      ep.rows = d_rows; ep.n_rows = cnt; ep.bits = d_bits; ep.zbits = d_zbits;
      launch_explain_kernel(ep.kind, dim3((unsigned)((cnt + 255) / 256)), st, ep, apow0, apow1, P->d_pic);
      HIPC(hipGetLastError());
      if (Z && zflags) {
        hipLaunchKernelGGL(explain_z_rows_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, ep);
        HIPC(hipGetLastError());
      }
      HIPC(hipStreamSynchronize(st));
      HIPC(hipMemcpy(bflags + k0 * ep.bbytes, d_bits, cnt * ep.bbytes, hipMemcpyDeviceToHost));   // the caller's memory is pageable: plain copies
      if (Z && zflags) HIPC(hipMemcpy(zflags + k0 * ep.zbytes, d_zbits, cnt * ep.zbytes, hipMemcpyDeviceToHost));
    }
    HIPC(hipEventRecord(ev[2], st));
    HIPC(hipEventRecord(ev[3], st));
    HIPC(hipStreamSynchronize(st));
  }
  for (int k = 0; k < 3; k++) HIPC(hipEventElapsedTime(&P->diag_ms[DIAG_EXPLAIN][k], ev[k], ev[k + 1]));
  return SBN_OK;
}

extern "C" int sbn_prover_explain_rows(sbn_prover* P, uint64_t seed, const uint64_t* rows, size_t n_rows, uint8_t* block_flags_out, uint8_t* z_flags_out) {
  if (!P || (n_rows && (!rows || !block_flags_out))) return fail(SBN_ERR_BAD_ARG, "null argument");
  static const uint64_t none = 0;
  return explain_device(P, seed, rows ? rows : &none, n_rows, block_flags_out, z_flags_out, nullptr, nullptr);
}
extern "C" int sbn_prover_explain_trace(sbn_prover* P, uint64_t seed, sbn_block_stat* block_stats_out, sbn_block_stat* z_stats_out) {
  if (!P || !block_stats_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  return explain_device(P, seed, nullptr, 0, nullptr, nullptr, block_stats_out, z_stats_out);
}
extern "C" int sbn_prover_explain_times(const sbn_prover* P, float* ms, int cap) { return P ? copy_times(P->diag_ms[DIAG_EXPLAIN], 3, ms, cap) : 0; }

// ---- host form --------------------------------------------------------------------------------------------------------------
namespace {
// Rows [r0, r0 + cnt) of the trace through the recording consumer; sink(i, block bits, z bits) once per row.
template <class Sink>
static void explain_span(const HostCheck& hc, size_t B, size_t r0, size_t cnt, const Sink& sink) {
  const size_t n = hc.n, C = hc.as.ncols, Z = hc.as.nzs;
  std::vector<u64> rows((cnt + 1) * C), zrows((cnt + 1) * std::max<size_t>(Z, 1));
  for (size_t c = 0; c < C; c++) {
    const u64* col = hc.trace + c * n;
    for (size_t r = 0; r <= cnt; r++) rows[r * C + c] = col[(r0 + r) & (n - 1)];
  }
  for (size_t z = 0; z < Z; z++) {
    const u64* col = hc.zval + z * n;
    for (size_t r = 0; r <= cnt; r++) zrows[r * Z + z] = col[(r0 + r) & (n - 1)];
  }
  const F g = f_root_of_unity(hc.degree_bits), last = f_inv(g), one(1);
  F x = f_pow(g, (u64)r0);
  std::vector<uint8_t> bb((B + 7) / 8), zb((Z + 7) / 8);
  const ExpShape es = exp_shape(hc.as);
  for (size_t r = 0; r < cnt; r++, x = x * g) {
    const size_t i = r0 + r;
    std::fill(bb.begin(), bb.end(), 0); std::fill(zb.begin(), zb.end(), 0);
    const F l_first(i == 0 ? 1 : 0), l_last(i == n - 1 ? 1 : 0);
    Cons<RF> cs{};
    for (int j = 0; j < SBN_NCH; j++) { cs.alpha[j] = RF(hc.alpha[j]); cs.apow[j] = (const RF*)hc.apow[j]; }
    cs.z_last = RF(x - last); cs.l_first = RF(l_first); cs.l_last = RF(l_last);
    cs.bits = bb.data();
    const RecRow row{rows.data() + r * C, rows.data() + (r + 1) * C};
    record_row_kind(hc.as.kind, cs, row, (int)hc.as.num_io, (int)hc.as.nconstraints, hc.pic);
    const u64 *zl = zrows.data() + r * Z, *zn = zl + Z;
    for (size_t z = 0; z < Z; z++) {   // permutation.rs eval_permutation_checks for Z column z: the first-row constraint and the transition
      int lc, rc;
      air_pair(hc.as.kind, es, (int)z, lc, rc);
      const F lv(row.lv[lc]), rv(row.lv[rc]);
      const F t = F(zn[z]) * ((rv + hc.gamma0) * (rv + hc.gamma1)) - F(zl[z]) * ((lv + hc.gamma0) * (lv + hc.gamma1));
      const F f = (F(zl[z]) - one) * l_first;
      if (t.v != 0 || f.v != 0) zb[z >> 3] |= (uint8_t)(1u << (z & 7));
    }
    sink(i, bb.data(), zb.data());
  }
}
}  // namespace

extern "C" int sbn_explain_rows_host(const sbn_air_desc* air, const uint64_t* trace, uint32_t degree_bits, const uint64_t* pi, size_t n_pi,
                                     uint64_t seed, const uint64_t* rows, size_t n_rows, uint8_t* block_flags_out, uint8_t* z_flags_out) {
  if (!air || !trace || (n_rows && (!rows || !block_flags_out))) return fail(SBN_ERR_BAD_ARG, "null argument");
  HostCheck hc{};
  HostStore hs;
  if (int rc = host_setup(air, trace, degree_bits, pi, n_pi, seed, hc, hs)) return rc;
  for (size_t k = 0; k < n_rows; k++) if (rows[k] >= hc.n) return fail(SBN_ERR_BAD_ARG, "row %llu of a trace of %zu rows", (unsigned long long)rows[k], hc.n);
  std::vector<sbn_constraint_block> blocks;
  if (int rc = block_table(hc.as, blocks)) return rc;
  const size_t B = blocks.size(), bbytes = (B + 7) / 8, zbytes = (hc.as.nzs + 7) / 8;
  host_parallel_for(n_rows, [&](size_t k) {
    explain_span(hc, B, (size_t)rows[k], 1, [&](size_t, const uint8_t* bb, const uint8_t* zb) {
      std::copy(bb, bb + bbytes, block_flags_out + k * bbytes);
      if (z_flags_out) std::copy(zb, zb + zbytes, z_flags_out + k * zbytes);
    });
  });
  return SBN_OK;
}

extern "C" int sbn_explain_trace_host(const sbn_air_desc* air, const uint64_t* trace, uint32_t degree_bits, const uint64_t* pi, size_t n_pi,
                                      uint64_t seed, sbn_block_stat* block_stats_out, sbn_block_stat* z_stats_out) {
  if (!air || !trace || !block_stats_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  HostCheck hc{};
  HostStore hs;
  if (int rc = host_setup(air, trace, degree_bits, pi, n_pi, seed, hc, hs)) return rc;
  std::vector<sbn_constraint_block> blocks;
  if (int rc = block_table(hc.as, blocks)) return rc;
  const size_t B = blocks.size(), Z = hc.as.nzs, tiles = hc.n / HOST_TILE;
  // failing rows per tile and block, summed in tile order afterwards: the first row of a block is its first tile's
  std::vector<std::vector<std::pair<u32, u64>>> hits(tiles);   // (index: block b, or B + z; row), rows ascending inside a tile
  host_parallel_for(tiles, [&](size_t t) {
    explain_span(hc, B, t * HOST_TILE, HOST_TILE, [&](size_t i, const uint8_t* bb, const uint8_t* zb) {
      for (size_t b = 0; b < B; b++) if ((bb[b >> 3] >> (b & 7)) & 1) hits[t].emplace_back((u32)b, (u64)i);
      for (size_t z = 0; z < Z; z++) if ((zb[z >> 3] >> (z & 7)) & 1) hits[t].emplace_back((u32)(B + z), (u64)i);
    });
  });
  for (size_t b = 0; b < B; b++) block_stats_out[b] = sbn_block_stat{0, UINT64_MAX};
  if (z_stats_out) for (size_t z = 0; z < Z; z++) z_stats_out[z] = sbn_block_stat{0, UINT64_MAX};
  for (size_t t = 0; t < tiles; t++)
    for (const auto& h : hits[t]) {
      sbn_block_stat* s = h.first < B ? &block_stats_out[h.first] : (z_stats_out ? &z_stats_out[h.first - B] : nullptr);
      if (!s) continue;
      if (!s->failing_rows++) s->first_row = h.second;
    }
  return SBN_OK;
}
