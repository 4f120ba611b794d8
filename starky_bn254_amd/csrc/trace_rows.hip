// Row-major traces (include/sbn.h sbn_host_rows): the reference's `rows` as they stand in front of its `transpose`, into the
// column-major trace of a prover.  The argument refusals, the host twin (sbn_trace_from_rows_host), the upload of the pieces
// through the pinned ring of prove_host_trace, the device transposition (kernels_rows.cuh) and, in main-row mode, the hand-over
// to the derived-column kernels of the device witness (tracegen_device.hip launch_derived_columns).
#include "prover_ctx.hpp"
#include "kernels_rows.cuh"
#include "host_rows.hpp"
#include <atomic>
#include <vector>

namespace {

// Columns in front of the derived ones, for every table that has any: the Exp tables' num_main (the one count main-row mode takes),
// and the counts of the other tables, which only serve to tell their main-row request (refusal 8) from a wrong n_cols (refusal 4).
size_t main_columns_of(const AirShape& as) {
  switch (as.kind) {
    case SBN_AIR_G1_OP: return G1OpShape::MAIN_COLS;
    case SBN_AIR_MODULAR: case SBN_AIR_FQ12_MUL: return (size_t)OpShape(as.kind).main_cols;
    case SBN_AIR_LOOKUP: return 2;
    case SBN_AIR_FLAGS: return FlagShape::MAIN_COLS;
    case SBN_AIR_FLAGS_U64: return FlagU64Shape::MAIN_COLS;
    default: return is_exp_air(as.kind) ? (size_t)exp_shape(as).num_main : 0;
  }
}
bool is_fq12_kind(int kind) { return kind == SBN_AIR_FQ12_EXP || kind == SBN_AIR_FQ12_EXP_U64; }

// what the refusals leave behind for the data path
struct RowsCall {
  bool main_mode = false, reduce = false;
  std::vector<u64> pi;   // the public inputs, reduced where the flag says so
};

// refusal 3 of the calls without a prover: the height must be a power of two, and the one the table's num_io fixes
int rows_height(const AirShape& as, size_t n_rows, uint32_t* degree_bits) {
  if (n_rows == 0 || (n_rows & (n_rows - 1))) return fail(SBN_ERR_BAD_ARG, "n_rows = %zu is no power of two", n_rows);
  if ((is_exp_air(as.kind) || as.kind == SBN_AIR_FLAGS || as.kind == SBN_AIR_FLAGS_U64) && n_rows != exp_rows_per_instance(as.kind) * as.num_io)
    return fail(SBN_ERR_BAD_ARG, "n_rows = %zu, the table has %zu rows", n_rows, exp_rows_per_instance(as.kind) * (size_t)as.num_io);
  uint32_t b = 0; while (((size_t)1 << b) < n_rows) b++;
  *degree_bits = b;
  return 0;
}
// refusal 4, first half: whole rows, main rows, or neither
int rows_mode(const AirShape& as, size_t n_cols, bool* main_mode) {
  const size_t main = main_columns_of(as);
  if (n_cols != as.ncols && (main == 0 || n_cols != main))
    return fail(SBN_ERR_BAD_ARG, "n_cols = %zu: whole rows of this table have %zu columns, main rows %zu", n_cols, as.ncols, main);
  *main_mode = n_cols != as.ncols;
  return 0;
}
// refusals 6 and 7
int rows_flags_and_pi(const AirShape& as, uint32_t flags, bool with_pi, const uint64_t* pi, size_t n_pi, RowsCall& call) {
  if (flags & ~SBN_TRACE_REDUCE) return fail(SBN_ERR_BAD_ARG, "unknown flag bits 0x%x", flags & ~SBN_TRACE_REDUCE);
  call.reduce = (flags & SBN_TRACE_REDUCE) != 0;
  if (!with_pi) return 0;
  if (n_pi != as.npi) return fail(SBN_ERR_BAD_ARG, "expected %zu public inputs, got %zu", as.npi, n_pi);
  if (n_pi && !pi) return fail(SBN_ERR_BAD_ARG, "null public inputs");
  call.pi.assign(pi, pi + n_pi);
  for (size_t i = 0; i < n_pi; i++) {
    if (call.pi[i] < GLP) continue;
    if (!call.reduce) return fail(SBN_ERR_NON_CANONICAL, "public input %zu is not canonical", i);
    call.pi[i] -= GLP;
  }
  return 0;
}
// refusal 8: on the device the gate of the device witness; on the host the u16 tables from 2^16 rows (the generators' own limit)
int rows_mode_covered(const AirShape& as, size_t n, bool main_mode, bool device) {
  if (!main_mode) return 0;
  if (device || !is_exp_air(as.kind)) return derived_columns_covered(as, n);
  if (!is_fq12_kind(as.kind) && n < 65536) return fail(SBN_ERR_UNSUPPORTED, "the table needs >= 2^16 rows (u16 range check, range_check.rs:26)");
  return 0;
}
// refusals 1 (struct_size) .. 8 of a sbn_host_rows; n: the prover's height, or 0 for the calls without a prover (*degree_bits then
// receives the height's logarithm)
int rows_refused(const AirShape& as, size_t n, const sbn_host_rows* rows, uint32_t flags, bool with_pi, const uint64_t* pi, size_t n_pi, bool device,
                 RowsCall& call, uint32_t* degree_bits = nullptr) {
  if (!rows) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (rows->struct_size != sizeof(sbn_host_rows)) return fail(SBN_ERR_BAD_ARG, "sbn_host_rows.struct_size is %u, expected %zu", rows->struct_size, sizeof(sbn_host_rows));
  if ((rows->flat != nullptr) == (rows->row_ptrs != nullptr)) return fail(SBN_ERR_BAD_ARG, "exactly one of flat and row_ptrs must be set");
  if (n) { if (rows->n_rows != n) return fail(SBN_ERR_BAD_ARG, "n_rows = %zu, the prover has %zu rows", rows->n_rows, n); }
  else { uint32_t b = 0; if (int rc = rows_height(as, rows->n_rows, &b)) return rc; if (degree_bits) *degree_bits = b; }
  if (int rc = rows_mode(as, rows->n_cols, &call.main_mode)) return rc;
  const size_t bad = host_rows_refused(HostRows{rows->flat, rows->row_stride, rows->row_ptrs, rows->n_rows, rows->n_cols});
  if (bad == 2) return fail(SBN_ERR_BAD_ARG, "row_stride = %zu is below n_cols = %zu (or n_rows * row_stride overflows)", rows->row_stride, rows->n_cols);
  if (bad >= 3) return fail(SBN_ERR_BAD_ARG, "row %zu is null or not 8-byte aligned", bad - 3);
  if (int rc = rows_flags_and_pi(as, flags, with_pi, pi, n_pi, call)) return rc;
  return rows_mode_covered(as, rows->n_rows, call.main_mode, device);
}

// the two data errors, named by the smallest row-major index
int rows_data_error(const unsigned long long err[3], size_t n_cols) {
  if (err[0] != ~0ull) return fail(SBN_ERR_NON_CANONICAL, "trace word at row %zu, column %zu is not canonical", (size_t)(err[0] / n_cols), (size_t)(err[0] % n_cols));
  if (err[2] != ~0ull)
    return fail(SBN_ERR_WITNESS, "range-checked column holds a value >= 2^16 at row %zu, column %zu", (size_t)(err[2] / n_cols), (size_t)(err[2] % n_cols));
  return 0;
}

// ---- the device path --------------------------------------------------------------------------------------------------------
// host != null: the rows cross PCIe in pieces of whole rows.  Host threads pack piece k into a slot of the pinned ring (copy_rows of
// host_rows.hpp), the copy stream sends it to staging buffer k & 1, and the main stream transposes it into d_trace behind the copy's
// event; the copy of piece k + 2 waits for the transposition of piece k, so piece k + 1 is packed and sent while piece k is
// transposed.  host == null: the rows are at d_rows already, one launch.  Scratch, carved from the front of the LDE buffer by the
// carver of the device witness (prover_ctx.hpp LdeScratch): the error words, then the one or two staging buffers.
int rows_into_trace(sbn_prover* P, const HostRows* host, const u64* d_rows, size_t d_stride, size_t n_cols, const RowsCall& call, unsigned long long err[3]) {
  const size_t n = P->n;
  size_t per = n, pieces = 1, nbuf = 0;
  if (host) {
    per = rows_per_piece(n, n_cols, UPLOAD_SLOT_WORDS);
    if (per == 0) return fail(SBN_ERR_UNSUPPORTED, "a row of %zu words does not fit a slot of the upload ring", n_cols);
    pieces = (n + per - 1) / per;
    nbuf = pieces < 2 ? pieces : 2;
  }
  LdeScratch scratch(P);
  unsigned long long* d_err = (unsigned long long*)scratch.take(3);
  const size_t stage_words = (per * n_cols + 7) & ~(size_t)7;
  u64* const stage = scratch.take(nbuf * stage_words);
  if (int rc = scratch.fits()) return rc;
  if (host) if (int rc = upload_setup(P)) return rc;
  HIPC(hipMemsetAsync(d_err, 0xff, 3 * sizeof(unsigned long long), P->stream));
  HIPC(hipMemsetAsync(d_err + 1, 0, sizeof(unsigned long long), P->stream));
  rowsk::RowsParams q{};
  q.n_cols = n_cols; q.n = n; q.trace = P->d_trace; q.reduce = call.reduce ? 1 : 0; q.err = d_err;
  if (call.main_mode) { const ExpShape sh = exp_shape(P->air); q.rc0 = sh.rc_start; q.rc1 = sh.rc_start + sh.num_rc; }
  auto launch = [&](const u64* src, size_t stride, size_t r0, size_t R) {
    q.src = src; q.src_stride = stride; q.r0 = r0; q.R = R;
    const dim3 grid((unsigned)((R + rowsk::RT_TILE - 1) / rowsk::RT_TILE), (unsigned)((n_cols + rowsk::RT_TILE - 1) / rowsk::RT_TILE));
    hipLaunchKernelGGL(rowsk::rows_to_columns_kernel, grid, dim3(rowsk::RT_THREADS), 0, P->stream, q);
  };
  if (!host) launch(d_rows, d_stride, 0, n);
  else {
    hipEvent_t* const copied = P->upload_done + ROWS_EV_COPIED;           // [b]: the copy into staging buffer b has landed (copy stream)
    hipEvent_t* const transposed = P->upload_done + ROWS_EV_TRANSPOSED;   // [b]: the kernel has left staging buffer b (main stream)
    const size_t threads = std::min<size_t>(tracegen_host_threads(), 16);
    for (size_t k = 0; k < pieces; k++) {
      size_t r0 = 0, r1 = 0;
      if (!piece_rows(n, per, k, &r0, &r1)) return fail(SBN_ERR_HIP, "internal: piece %zu of %zu", k, pieces);
      const size_t R = r1 - r0, len = R * n_cols, b = k & 1;
      const unsigned s = P->slot_next; P->slot_next = (s + 1) % UPLOAD_SLOTS;
      if (P->slot_used[s]) HIPC(hipEventSynchronize(P->slot_copied[s]));
      u64* slot = P->h_ring + (size_t)s * UPLOAD_SLOT_WORDS;
      const size_t parts = std::max<size_t>(1, std::min(std::min(threads, len >> 15), R)), rows_per = (R + parts - 1) / parts;   // >= 256 KiB per thread
      host_parallel_for(parts, [&](size_t t) { const size_t a = r0 + t * rows_per, e = std::min(r1, a + rows_per); if (a < e) copy_rows(*host, a, e, slot + (a - r0) * n_cols); });
      if (k >= 2) HIPC(hipStreamWaitEvent(P->ustream, transposed[b], 0));
      HIPC(hipMemcpyAsync(stage + b * stage_words, slot, len * sizeof(u64), hipMemcpyHostToDevice, P->ustream));
      HIPC(hipEventRecord(P->slot_copied[s], P->ustream));
      P->slot_used[s] = true;
      HIPC(hipEventRecord(copied[b], P->ustream));
      HIPC(hipStreamWaitEvent(P->stream, copied[b], 0));
      launch(stage + b * stage_words, n_cols, r0, R);
      HIPC(hipEventRecord(transposed[b], P->stream));
    }
  }
  HIPC(hipGetLastError());
  // the error words in one small copy; the derived-column kernels run only behind a clean result (they index LDS by the value)
  HIPC(hipMemcpyAsync(err, d_err, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, P->stream));
  HIPC(hipStreamSynchronize(P->stream));
  if (P->ustream) HIPC(hipStreamSynchronize(P->ustream));
  return 0;
}

// behind the refusals: d_trace from the rows, the data errors, then the derived columns or the fixed-columns comparison
int load_rows(sbn_prover* P, const HostRows* host, const u64* d_rows, size_t d_stride, size_t n_cols, const RowsCall& call, uint64_t* reduced_out) {
  if (P->sp) return fail(SBN_ERR_UNSUPPORTED, "row-major loads cover single-GPU provers");
  P->pi = call.pi;
  HIPC(hipSetDevice(P->device));
  unsigned long long err[3] = {~0ull, 0, ~0ull};
  int rc = rows_into_trace(P, host, d_rows, d_stride, n_cols, call, err);
  if (!rc) rc = rows_data_error(err, n_cols);
  if (!rc) rc = call.main_mode ? launch_derived_columns(P) : fixed_columns_check(P);
  if (rc) {   // whatever was enqueued ends before the caller sees the error: idle streams, a free ring, no trace loaded
    const std::string msg = g_last_error;
    for (hipStream_t s : {P->ustream, P->stream, P->hstream, P->nstream}) if (s) (void)hipStreamSynchronize(s);
    g_last_error = msg;
    P->loaded = false; P->fixed_match = false;
    return rc;
  }
  if (reduced_out) *reduced_out = call.reduce ? err[1] : 0;
  P->loaded = true;
  return SBN_OK;
}

int unload(sbn_prover* P, uint64_t* reduced_out) {
  if (reduced_out) *reduced_out = 0;
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  P->loaded = false;   // before any check: a refused call must not leave the previous trace provable
  P->fixed_match = false;
  return 0;
}

}  // namespace

namespace sbn {
int host_rows_precheck(const sbn_air_desc* air, const sbn_host_rows* rows, uint32_t flags, const uint64_t* pi, size_t n_pi, uint32_t* degree_bits_out) {
  AirShape as;
  if (!air_shape(air, nullptr, as)) return fail(SBN_ERR_BAD_ARG, "null or unknown table");
  RowsCall call;
  return rows_refused(as, 0, rows, flags, true, pi, n_pi, true, call, degree_bits_out);
}
}  // namespace sbn

extern "C" size_t sbn_air_num_main_columns(const sbn_air_desc* air) {
  AirShape as;
  return air_shape(air, nullptr, as) && is_exp_air(as.kind) ? (size_t)exp_shape(as).num_main : 0;
}

// The host twin: the same refusals, the transposition with its scans on the host pool in tiles of 64 rows x 64 columns (a tile of
// the source stays in the first-level cache while its columns are written 64 consecutive words at a time), then the derived columns
// by the code of the host generators (tracegen.hip derived_columns_host).
extern "C" int sbn_trace_from_rows_host(const sbn_air_desc* air, const sbn_host_rows* rows, uint32_t flags, uint64_t* out, uint64_t* reduced_out) {
  if (reduced_out) *reduced_out = 0;
  if (!air || !rows || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  AirShape as;
  if (!air_shape(air, nullptr, as)) return fail(SBN_ERR_BAD_ARG, "unknown table");
  RowsCall call;
  if (int rc = rows_refused(as, 0, rows, flags, false, nullptr, 0, false, call)) return rc;
  const HostRows m{rows->flat, rows->row_stride, rows->row_ptrs, rows->n_rows, rows->n_cols};
  const size_t n = m.n_rows, C = m.n_cols, T = 64;
  size_t rc0 = 0, rc1 = 0;
  if (call.main_mode) { const ExpShape sh = exp_shape(as); rc0 = (size_t)sh.rc_start; rc1 = rc0 + (size_t)sh.num_rc; }
  std::atomic<unsigned long long> bad(~0ull), bad_range(~0ull), changed(0);
  auto fold_min = [](std::atomic<unsigned long long>& a, unsigned long long v) { unsigned long long cur = a.load(); while (v < cur && !a.compare_exchange_weak(cur, v)) {} };
  host_parallel_for((n + T - 1) / T, [&](size_t t) {
    const size_t r0 = t * T, r1 = std::min(n, r0 + T);
    unsigned long long my_bad = ~0ull, my_range = ~0ull, my_changed = 0;
    for (size_t c0 = 0; c0 < C; c0 += T) {
      const size_t c1 = std::min(C, c0 + T);
      for (size_t c = c0; c < c1; c++) {
        u64* dst = out + c * n;
        const bool ranged = c >= rc0 && c < rc1;
        for (size_t r = r0; r < r1; r++) {
          u64 w = m.row(r)[c];
          if (w >= GLP) {
            if (call.reduce) { w -= GLP; my_changed++; }
            else my_bad = std::min<unsigned long long>(my_bad, r * C + c);
          }
          if (ranged && w >= 65536) my_range = std::min<unsigned long long>(my_range, r * C + c);
          dst[r] = w;
        }
      }
    }
    if (my_bad != ~0ull) fold_min(bad, my_bad);
    if (my_range != ~0ull) fold_min(bad_range, my_range);
    if (my_changed) changed += my_changed;
  });
  const unsigned long long err[3] = {bad.load(), changed.load(), bad_range.load()};
  if (int rc = rows_data_error(err, C)) return rc;
  if (call.main_mode && !derived_columns_host(exp_shape(as), out, n)) return fail(SBN_ERR_WITNESS, "range-checked column holds a value >= 2^16");
  if (reduced_out) *reduced_out = err[1];
  return SBN_OK;
}

extern "C" int sbn_prover_load_trace_rows(sbn_prover* P, const sbn_host_rows* rows, uint32_t flags, const uint64_t* pi, size_t n_pi, uint64_t* reduced_out) {
  if (int rc = unload(P, reduced_out)) return rc;
  RowsCall call;
  if (int rc = rows_refused(P->air, P->n, rows, flags, true, pi, n_pi, true, call)) return rc;
  const HostRows m{rows->flat, rows->row_stride, rows->row_ptrs, rows->n_rows, rows->n_cols};
  return load_rows(P, &m, nullptr, 0, m.n_cols, call, reduced_out);
}

extern "C" int sbn_prover_load_trace_rows_device(sbn_prover* P, const uint64_t* d_rows, size_t row_stride, size_t n_cols, uint32_t flags, const uint64_t* pi,
                                                 size_t n_pi, uint64_t* reduced_out) {
  if (int rc = unload(P, reduced_out)) return rc;
  if (!d_rows) return fail(SBN_ERR_BAD_ARG, "null argument");
  RowsCall call;
  if (int rc = rows_mode(P->air, n_cols, &call.main_mode)) return rc;
  if (row_stride < n_cols || (row_stride && P->n > (size_t)-1 / sizeof(u64) / row_stride)) return fail(SBN_ERR_BAD_ARG, "row_stride = %zu is below n_cols = %zu (or n_rows * row_stride overflows)", row_stride, n_cols);
  if ((uintptr_t)d_rows & 7) return fail(SBN_ERR_BAD_ARG, "row 0 is null or not 8-byte aligned");
  if (int rc = rows_flags_and_pi(P->air, flags, true, pi, n_pi, call)) return rc;
  if (int rc = rows_mode_covered(P->air, P->n, call.main_mode, true)) return rc;
  return load_rows(P, nullptr, d_rows, row_stride, n_cols, call, reduced_out);
}

extern "C" int sbn_prover_prove_host_rows(sbn_prover* P, const sbn_host_rows* rows, uint32_t flags, const uint64_t* pi, size_t n_pi, uint64_t* reduced_out,
                                          sbn_proof** out) {
  if (out) *out = nullptr;
  if (int rc = unload(P, reduced_out)) return rc;
  if (!out) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (int rc = sbn_prover_load_trace_rows(P, rows, flags, pi, n_pi, reduced_out)) return rc;
  const int rc = sbn_prover_prove(P, out);
  if (rc) { P->loaded = false; P->fixed_match = false; }   // a failing call leaves no trace loaded
  return rc;
}
