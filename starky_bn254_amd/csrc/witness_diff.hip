// A loaded trace against the canonical witness of its instance list, cell by cell (include/sbn.h, sbn_instances_from_public_inputs /
// sbn_prover_diff_witness / sbn_diff_witness_host).  The canonical witness is what the generators write for the list: the host
// generators of tracegen.hip for the host twin, sbn_prover_generate_trace for the device form -- called with P->d_trace and
// P->d_coef exchanged, so that the existing drivers of tracegen_device.hip write into the coefficient buffer ([C][n] words, idle
// between proofs) and the caller's trace is never touched.  Their scratch stays where LdeScratch carves it, at the front of the LDE
// buffer; the counters and the listed cells live in P->d_part (64 n words).  Nothing is allocated beyond the memory plan.
// Everything that is not a kernel or a refusal is witness_diff.hpp (plain C++), shared by both forms.
#include "prover_ctx.hpp"
#include "witness_diff.hpp"
#include "kernels_witdiff.cuh"
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>

static_assert(sizeof(WitDiff) == sizeof(sbn_witness_diff) && sizeof(WitCell) == sizeof(sbn_witness_cell), "witness_diff.hpp mirrors include/sbn.h");
static_assert(sizeof(wd::Job) == sizeof(WitJob) && sizeof(wd::Cell) == sizeof(WitCell), "kernels_witdiff.cuh mirrors witness_diff.hpp");

namespace {
// refusal 1 of both forms (the header's order)
int check_outputs(const sbn_witness_diff* report, const sbn_witness_cell* cells_out, size_t cells_cap) {
  if (!report) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (report->struct_size != sizeof(sbn_witness_diff)) return fail(SBN_ERR_BAD_ARG, "sbn_witness_diff.struct_size is %u, this library's is %zu", report->struct_size, sizeof(sbn_witness_diff));
  if (cells_cap > WIT_MAX_CELLS) return fail(SBN_ERR_BAD_ARG, "cells_cap is %zu, at most %zu cells are listed", cells_cap, WIT_MAX_CELLS);
  if (cells_cap && !cells_out) return fail(SBN_ERR_BAD_ARG, "null cells_out with a cap of %zu", cells_cap);
  return SBN_OK;
}
const char* const NOT_EXP = "the witness diff covers the five Exp tables: no other table carries its instance list in its public inputs";

// the instances of `pi` (n_pi = num_io instances of L.per() words); outputs optional
int instances_from_pi(const PiLayout& L, const uint64_t* pi, size_t num_io, uint32_t* ios, uint32_t* outputs) {
  const size_t per = L.per(), IOW = 2 * L.xw + L.ew;
  std::vector<uint32_t> scratch(L.xw);
  for (size_t k = 0; k < num_io; k++) {
    const uint64_t* p = pi + per * k;
    uint32_t* io = ios + IOW * k;
    size_t bad = 0;
    if (!value_from_pi(L, p, io, &bad)) return fail(SBN_ERR_BAD_ARG, "public input %zu (instance %zu, x) is out of the range of its limb", per * k + bad, k);
    if (!value_from_pi(L, p + L.W, io + L.xw, &bad)) return fail(SBN_ERR_BAD_ARG, "public input %zu (instance %zu, offset) is out of the range of its limb", per * k + L.W + bad, k);
    if (!exp_from_pi(L, p + 2 * L.W, io + 2 * L.xw, &bad)) return fail(SBN_ERR_BAD_ARG, "public input %zu (instance %zu, exponent) is out of the range of its limb", per * k + 2 * L.W + bad, k);
    if (!value_from_pi(L, p + 2 * L.W + L.EW, outputs ? outputs + L.xw * k : scratch.data(), &bad))
      return fail(SBN_ERR_BAD_ARG, "public input %zu (instance %zu, output) is out of the range of its limb", per * k + 2 * L.W + L.EW + bad, k);
  }
  return SBN_OK;
}

int host_generate(int kind, const uint32_t* ios, size_t num_io, uint64_t* trace, uint64_t* pi) {
  switch (kind) {
    case SBN_AIR_G1_EXP: return sbn_generate_trace_g1_exp(ios, num_io, trace, pi);
    case SBN_AIR_G2_EXP: return sbn_generate_trace_g2_exp(ios, num_io, trace, pi);
    case SBN_AIR_FQ12_EXP: return sbn_generate_trace_fq12_exp(ios, num_io, trace, pi);
    case SBN_AIR_FQ12_EXP_U64: return sbn_generate_trace_fq12_exp_u64(ios, num_io, trace, pi);
    default: return sbn_generate_trace_fq_exp(ios, num_io, trace, pi);
  }
}
// refusal 6: the generator's own words behind the prefix (fail() formats before it assigns)
int no_witness(int rc) { return fail(rc, "no canonical witness: %s", g_last_error.c_str()); }

void pi_difference(const uint64_t* loaded, const uint64_t* canonical, size_t n_pi, WitDiff& d) {
  d.pi_words = 0; d.first_pi_word = WIT_NONE;
  for (size_t i = 0; i < n_pi; i++)
    if (loaded[i] != canonical[i]) { if (!d.pi_words++) d.first_pi_word = i; }
}
void write_columns(const uint32_t* col_cells, const uint32_t* col_first, size_t C, uint64_t* cells_out, uint64_t* first_out) {
  for (size_t c = 0; c < C; c++) {
    if (cells_out) cells_out[c] = col_cells[c];
    if (first_out) first_out[c] = col_cells[c] ? (uint64_t)col_first[c] : WIT_NONE;
  }
}
}  // namespace

extern "C" int sbn_instances_from_public_inputs(int32_t kind, const uint64_t* public_inputs, size_t n_pi, size_t num_io, uint32_t* ios_out, uint32_t* outputs_out) {
  if (!public_inputs || !ios_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  PiLayout L;
  if (!pi_layout((int)kind, L)) return fail(SBN_ERR_BAD_ARG, "kind %d is not an Exp table", (int)kind);
  if (num_io == 0 || n_pi / num_io != L.per() || n_pi % num_io) return fail(SBN_ERR_BAD_ARG, "%zu public inputs are not %zu instances of %zu words", n_pi, num_io, L.per());
  return instances_from_pi(L, public_inputs, num_io, ios_out, outputs_out);
}

extern "C" int sbn_diff_witness_host(const sbn_air_desc* air, const uint64_t* trace, uint32_t degree_bits, const uint64_t* public_inputs, size_t n_pi,
                                     const uint32_t* ios, size_t num_io, sbn_witness_diff* report, uint64_t* column_cells_out, uint64_t* column_first_row_out,
                                     sbn_witness_cell* cells_out, size_t cells_cap) {
  if (!air || !trace || !public_inputs) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (int rc = check_outputs(report, cells_out, cells_cap)) return rc;
  AirShape as;
  if (!air_shape(air, nullptr, as)) return fail(SBN_ERR_BAD_ARG, "unknown table");
  if (num_io != as.num_io) return fail(SBN_ERR_BAD_ARG, "the table has %u instances, got %zu", as.num_io, num_io);
  if (!is_exp_air(as.kind)) return fail(SBN_ERR_UNSUPPORTED, "%s", NOT_EXP);
  if (degree_bits >= 8 * sizeof(size_t) || ((size_t)1 << degree_bits) != exp_rows_per_instance(as.kind) * num_io) return fail(SBN_ERR_BAD_ARG, "degree_bits does not match the rows per instance");
  if (n_pi != as.npi) return fail(SBN_ERR_BAD_ARG, "the table has %zu public inputs, got %zu", as.npi, n_pi);
  const size_t n = (size_t)1 << degree_bits, C = as.ncols, num_main = (size_t)exp_shape(as).num_main;
  const PiLayout L = pi_layout(as.kind);
  std::vector<uint32_t> own;
  if (!ios) {
    own.resize(exp_io_words(as.kind) * num_io);
    if (int rc = instances_from_pi(L, public_inputs, num_io, own.data(), nullptr)) return rc;
    ios = own.data();
  }
  // the temporary: zero pages as the generators' callers hand them in, untouched until written
  const std::unique_ptr<uint64_t, decltype(&free)> want_mem((uint64_t*)calloc(C * n, sizeof(uint64_t)), free);
  if (!want_mem) return fail(SBN_ERR_BAD_ARG, "no memory for the canonical witness (%zu words)", C * n);
  const uint64_t* const want = want_mem.get();
  std::vector<uint64_t> pi(n_pi);
  if (int rc = host_generate(as.kind, ios, num_io, want_mem.get(), pi.data())) return no_witness(rc);

  // tiles of WIT_TILE x WIT_TILE; a task owns WIT_TILE rows, so their counters are its own; the column counters of a tile that
  // differs are merged under a lock (integer adds and minima: any order gives the same words; a clean trace never locks)
  std::vector<uint32_t> col_cells(C, 0), col_first(C, WIT_NO_ROW), row_main(n, 0), row_total(n, 0);
  std::mutex merge;
  host_parallel_for((n + WIT_TILE - 1) / WIT_TILE, [&](size_t t) {
    const size_t r0 = t * WIT_TILE, r1 = std::min(n, r0 + WIT_TILE);
    for (size_t c0 = 0; c0 < C; c0 += WIT_TILE) {
      const size_t c1 = std::min(C, c0 + WIT_TILE);
      uint32_t cc[WIT_TILE] = {}, cf[WIT_TILE];
      for (size_t i = 0; i < WIT_TILE; i++) cf[i] = WIT_NO_ROW;
      if (!wit_compare_tile(trace, want, n, r0, r1, c0, c1, num_main, cc, cf, row_main.data() + r0, row_total.data() + r0)) continue;
      std::lock_guard<std::mutex> lock(merge);
      for (size_t c = c0; c < c1; c++) { col_cells[c] += cc[c - c0]; col_first[c] = std::min(col_first[c], cf[c - c0]); }
    }
  });
  WitDiff d{};
  d.struct_size = sizeof(WitDiff);
  wit_statistics(col_cells.data(), col_first.data(), C, num_main, row_total.data(), n, d);
  std::vector<WitJob> jobs;
  d.listed = d.cells ? wit_select_rows(row_main.data(), row_total.data(), n, num_main, C, cells_cap, jobs) : 0;
  host_parallel_for(jobs.size(), [&](size_t j) { wit_list_row(trace, want, n, jobs[j], (WitCell*)cells_out); });
  pi_difference(public_inputs, pi.data(), n_pi, d);
  write_columns(col_cells.data(), col_first.data(), C, column_cells_out, column_first_row_out);
  memcpy(report, &d, sizeof d);
  return SBN_OK;
}

// The canonical witness of `ios` into P->d_coef, its public inputs into `pi`: sbn_prover_generate_trace between two exchanges of
// d_trace and d_coef.  Whatever the generator does to the loaded state -- it unloads first, its finish() sets loaded, pi and
// fixed_match for the buffer it wrote, a failure leaves no trace loaded -- is put back on every return path: after the exchange
// back those words would describe the caller's trace wrongly.  fixed_valid is cleared: d_coef has been overwritten.
static int canonical_witness(sbn_prover* P, const uint32_t* ios, size_t num_io, std::vector<u64>& pi, float* ms) {
  struct Guard {
    sbn_prover* P; const bool loaded, fixed_match; std::vector<u64> pi; const float tracegen_ms;
    explicit Guard(sbn_prover* P) : P(P), loaded(P->loaded), fixed_match(P->fixed_match), pi(P->pi), tracegen_ms(P->stage_ms[ST_COUNT + EX_TRACEGEN_MS]) { std::swap(P->d_trace, P->d_coef); }
    ~Guard() {
      std::swap(P->d_trace, P->d_coef);
      P->loaded = loaded; P->fixed_match = fixed_match; P->pi.swap(pi);
      P->stage_ms[ST_COUNT + EX_TRACEGEN_MS] = tracegen_ms;
      P->fixed_valid = false;
    }
  } guard(P);
  const int rc = sbn_prover_generate_trace(P, ios, num_io, nullptr);
  *ms = P->stage_ms[ST_COUNT + EX_TRACEGEN_MS];
  if (rc == SBN_OK) pi = P->pi;
  return rc;
}

extern "C" int sbn_prover_diff_witness(sbn_prover* P, const uint32_t* ios, size_t num_io, sbn_witness_diff* report, uint64_t* column_cells_out,
                                       uint64_t* column_first_row_out, sbn_witness_cell* cells_out, size_t cells_cap) {
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (int rc = check_outputs(report, cells_out, cells_cap)) return rc;
  if (num_io != P->air.num_io) return fail(SBN_ERR_BAD_ARG, "prover was created for %u instances, got %zu", P->air.num_io, num_io);
  if (!P->loaded) return fail(SBN_ERR_BAD_ARG, "no trace loaded");
  const int kind = P->air.kind;
  if (!is_exp_air(kind)) return fail(SBN_ERR_UNSUPPORTED, "%s", NOT_EXP);
  if (int rc = diag_refuse_split(P, "the witness diff", true)) return rc;
  const size_t n = P->n, C = P->air.ncols, num_main = (size_t)exp_shape(P->air).num_main;
  const bool fq12 = kind == SBN_AIR_FQ12_EXP || kind == SBN_AIR_FQ12_EXP_U64;
  if (!fq12 && !u16_device_witness_covers(n))
    return fail(SBN_ERR_UNSUPPORTED, "the device witness of the u16-range-check tables %s, this context has %zu (sbn_diff_witness_host takes any height)", U16_DEVICE_WITNESS_ROWS, n);
  if (n != exp_rows_per_instance(kind) * num_io) return fail(SBN_ERR_BAD_ARG, "degree_bits does not match the rows per instance");
  if (P->pi.size() != P->air.npi) return fail(SBN_ERR_BAD_ARG, "the loaded trace carries %zu public inputs, the table has %zu", P->pi.size(), P->air.npi);
  float* const times = P->diag_ms[DIAG_WITDIFF];
  for (int i = 0; i < 3; i++) times[i] = 0;
  std::vector<uint32_t> own;
  if (!ios) {
    own.resize(exp_io_words(kind) * num_io);
    if (int rc = instances_from_pi(pi_layout(kind), P->pi.data(), num_io, own.data(), nullptr)) return rc;
    ios = own.data();
  }
  // d_part: [col_cells u32 C][col_first u32 C][row_main u32 n][row_total u32 n], then per launch of the list [jobs][cells]
  const size_t counters = 2 * (C + n) * sizeof(uint32_t), list_at = (counters + 31) & ~(size_t)31, part_bytes = (size_t)64 * n * sizeof(u64);
  if (n % wd::COMPARE_THREADS || (C + wd::TILE_COLS - 1) / wd::TILE_COLS > 65535 || n > 0xffffffffu || list_at + sizeof(WitJob) + sizeof(WitCell) > part_bytes)
    return fail(SBN_ERR_UNSUPPORTED, "internal: the counters of this table do not fit the scratch");

  std::vector<u64> pi;
  if (int rc = canonical_witness(P, ios, num_io, pi, &times[0])) return no_witness(rc);
  HIPC(hipSetDevice(P->device));
  hipStream_t st = P->stream;
  hipEvent_t* ev = P->ev;   // the stage events are idle outside prove()
  char* const base = (char*)P->d_part;
  unsigned *d_col_cells = (unsigned*)base, *d_col_first = d_col_cells + C, *d_row_main = d_col_first + C, *d_row_total = d_row_main + n;
  const wd::ull *got = (const wd::ull*)P->d_trace, *want = (const wd::ull*)P->d_coef;
  HIPC(hipEventRecord(ev[0], st));
  HIPC(hipMemsetAsync(base, 0, counters, st));
  HIPC(hipMemsetAsync(d_col_first, 0xff, C * sizeof(unsigned), st));
  hipLaunchKernelGGL(wd::compare_kernel, dim3((unsigned)(n / wd::COMPARE_THREADS), (unsigned)((C + wd::TILE_COLS - 1) / wd::TILE_COLS)), dim3(wd::COMPARE_THREADS), 0, st, got, want, n,
                     (unsigned)C, (unsigned)num_main, d_col_cells, d_col_first, d_row_main, d_row_total);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(ev[1], st));
  HIPC(hipStreamSynchronize(st));
  HIPC(hipEventElapsedTime(&times[1], ev[0], ev[1]));

  const auto t0 = std::chrono::steady_clock::now();
  // the column counters first: of a clean trace nothing else comes back (the caller's memory and these vectors are pageable: plain copies)
  std::vector<uint32_t> col(2 * C), row;
  HIPC(hipMemcpy(col.data(), d_col_cells, 2 * C * sizeof(uint32_t), hipMemcpyDeviceToHost));
  bool any = false;
  for (size_t c = 0; c < C && !any; c++) any = col[c] != 0;
  if (any) {
    row.resize(2 * n);
    HIPC(hipMemcpy(row.data(), d_row_main, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  WitDiff d{};
  d.struct_size = sizeof(WitDiff);
  wit_statistics(col.data(), col.data() + C, C, num_main, any ? row.data() + n : nullptr, n, d);
  std::vector<WitJob> jobs;
  d.listed = any ? wit_select_rows(row.data(), row.data() + n, n, num_main, C, cells_cap, jobs) : 0;
  // the cells of the chosen rows, as many launches as the scratch behind the counters asks for
  for (size_t j0 = 0; j0 < jobs.size();) {
    const size_t j1 = wit_next_launch(jobs, j0, part_bytes - list_at);
    if (j1 == j0) return fail(SBN_ERR_UNSUPPORTED, "internal: a chosen row does not fit the scratch");
    const size_t first = jobs[j0].offset, count = (size_t)jobs[j1 - 1].offset + jobs[j1 - 1].count - first;
    wd::Cell* d_cells = (wd::Cell*)(base + list_at);
    wd::Job* d_jobs = (wd::Job*)(d_cells + count);
    HIPC(hipMemcpyAsync(d_jobs, jobs.data() + j0, (j1 - j0) * sizeof(WitJob), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(wd::list_kernel, dim3((unsigned)(j1 - j0)), dim3(wd::LIST_THREADS), 0, st, got, want, n, d_jobs, (unsigned)first, d_cells);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(cells_out + first, d_cells, count * sizeof(WitCell), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));   // the next launch reuses the scratch; `jobs` is pageable anyway
    j0 = j1;
  }
  pi_difference(P->pi.data(), pi.data(), pi.size(), d);
  write_columns(col.data(), col.data() + C, C, column_cells_out, column_first_row_out);
  memcpy(report, &d, sizeof d);
  times[2] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SBN_OK;
}

extern "C" int sbn_prover_diff_witness_times(const sbn_prover* P, float* ms, int cap) { return P ? copy_times(P->diag_ms[DIAG_WITDIFF], 3, ms, cap) : 0; }
