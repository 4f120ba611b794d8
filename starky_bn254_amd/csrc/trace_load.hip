// The trace intake: every call that makes a trace resident in a prover, and the pieces they share.
//   column-major  sbn_prover_load_trace / _load_trace_device (a copy, then the comparison of the shape-constant columns),
//                 sbn_prover_read_trace, sbn_prover_trace_device_ptr; sbn_prover_prove_host_trace / _prove_host_columns, which stream
//                 the trace into the trace commitment of prover.hip chunk by chunk (HostUpload below, prove_streamed)
//   row-major     (include/sbn.h sbn_host_rows: the reference's `rows` as they stand in front of its `transpose`)
//                 sbn_prover_load_trace_rows / _load_trace_rows_device / _prove_host_rows: the argument refusals, the host twin
//                 (sbn_trace_from_rows_host), the device transposition (kernels_load.cuh) and, in main-row mode, the hand-over to the
//                 derived-column kernels of the device witness (tracegen_device.hip launch_derived_columns)
//   shared        one pinned ring in front of the copy stream (pinned_ring.hpp), one public-input routine (take_public_inputs), one
//                 way into a load (unload) and one way out of a failed one (abandon_load)
//   building blocks for the tests: sbn_first_non_canonical, sbn_gather_columns, sbn_reduce_words
#include "prover_ctx.hpp"
#include "kernels_load.cuh"
#include "host_columns.hpp"
#include "host_rows.hpp"
#include <atomic>
#include <thread>
#include <vector>

// the caller's trace (one flat allocation or one allocation per column); reduce (SBN_TRACE_REDUCE): reduce_words_kernel takes the
// scan's place, and d_first_bad counts the words it changed instead of holding the first one refused
struct HostUpload { HostColumns src; bool reduce; };

namespace {

// ---- shared by every load ---------------------------------------------------------------------------------------------------
// In front of a call's checks: a refused call must not leave the previous trace provable, and whatever the call leaves in d_trace
// is not known to hold the generators' words.
void unload(sbn_prover* P) { P->loaded = false; P->fixed_match = false; }
// A load that failed behind its first enqueue: whatever is in flight (the rest of an upload, transforms of a refused trace) ends
// before the caller sees the error, its message intact: the next call finds idle streams, a free ring and no trace loaded.
void abandon_load(sbn_prover* P) {
  const std::string msg = g_last_error;
  for (hipStream_t s : {P->ustream, P->stream, P->hstream, P->nstream}) if (s) (void)hipStreamSynchronize(s);
  g_last_error = msg;
  unload(P);
}
// The public inputs of a call: the count, the pointer, then every word canonical -- or, under `reduce`, taken mod p (one
// subtraction: 2^64 - 1 - p < p).  `out` is written on success only.
int take_public_inputs(const AirShape& as, const uint64_t* pi, size_t n_pi, bool reduce, std::vector<u64>& out) {
  if (n_pi != as.npi) return fail(SBN_ERR_BAD_ARG, "expected %zu public inputs, got %zu", as.npi, n_pi);
  if (n_pi && !pi) return fail(SBN_ERR_BAD_ARG, "null public inputs");
  std::vector<u64> v(pi, pi + n_pi);
  for (size_t i = 0; i < n_pi; i++) {
    if (v[i] < GLP) continue;
    if (!reduce) return fail(SBN_ERR_NON_CANONICAL, "public input %zu is not canonical", i);
    v[i] -= GLP;
  }
  out.swap(v);
  return 0;
}
// The copy stream, the pinned ring, the events of both upload forms and the scans' result word, created by the first call that
// uploads.  Idempotent: a call that failed half way is completed by the next one.
int upload_setup(sbn_prover* P) {
  if (!P->ustream) HIPC(hipStreamCreate(&P->ustream));
  for (auto& e : P->upload_done) if (!e) HIPC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (hipEvent_t* ev : {P->rows_copied, P->rows_transposed})
    for (int b = 0; b < 2; b++) if (!ev[b]) HIPC(hipEventCreateWithFlags(&ev[b], hipEventDisableTiming));
  HIPC(P->upload_ring.create(UPLOAD_SLOTS, UPLOAD_SLOT_WORDS));
  if (!P->h_first_bad) HIPC(hipHostMalloc((void**)&P->h_first_bad, sizeof(unsigned long long), hipHostMallocDefault));
  if (!P->d_first_bad) return alloc_buffers(P, {BufReq{(void**)&P->d_first_bad, sizeof(unsigned long long)}});   // lazy, outside the plan (include/sbn.h)
  return 0;
}
// the grid of the scan and of its reducing twin: two words per thread, grid-stride beyond 8 waves per CU
inline dim3 scan_grid(size_t count) { return dim3((unsigned)std::min<size_t>(std::max<size_t>((count / 2 + 255) / 256, 1), 2048)); }
void launch_first_non_canonical(const u64* d_words, size_t count, u64 base, unsigned long long* d_first_bad, hipStream_t st) {
  hipLaunchKernelGGL(first_non_canonical_kernel, scan_grid(count), dim3(256), 0, st, d_words, count, base, d_first_bad);
}
void launch_reduce_words(u64* d_words, size_t count, unsigned long long* d_reduced, hipStream_t st) {
  hipLaunchKernelGGL(reduce_words_kernel, scan_grid(count), dim3(256), 0, st, d_words, count, d_reduced);
}
// Behind a copy into d_trace: do its shape-constant columns hold the generators' words (P->fixed_match)?  The caller owns the trace,
// and a valid witness may hold other words there, so the device compares: one launch over (fixed_f1 - fixed_f0) n words and one
// word back.  The mismatch word borrows the start of d_tmp, which only prove() and the checks use, none of them in flight here.
int fixed_columns_check(sbn_prover* P) {
  P->fixed_match = false;
  if (P->fixed_f1 <= P->fixed_f0) return 0;
  unsigned long long* d_word = (unsigned long long*)P->d_tmp;
  unsigned long long mismatch = 1;
  if (int rc = launch_fixed_columns_check(P->d_trace + P->fixed_f0 * P->n, P->fixed_f1 - P->fixed_f0, P->n, exp_shape(P->air), d_word, P->stream)) return rc;
  HIPC(hipMemcpyAsync(&mismatch, d_word, sizeof mismatch, hipMemcpyDeviceToHost, P->stream));
  HIPC(hipStreamSynchronize(P->stream));
  P->fixed_match = mismatch == 0;
  return 0;
}

}  // namespace

void upload_destroy(sbn_prover* P) {
  P->upload_ring.destroy();
  if (P->h_first_bad) (void)hipHostFree(P->h_first_bad);
  for (auto& e : P->upload_done) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t* ev : {P->rows_copied, P->rows_transposed}) for (int b = 0; b < 2; b++) if (ev[b]) (void)hipEventDestroy(ev[b]);
  if (P->ustream) (void)hipStreamDestroy(P->ustream);
}

// ---- column-major traces: the resident loads --------------------------------------------------------------------------------
extern "C" int sbn_prover_load_trace(sbn_prover* P, const uint64_t* trace, const uint64_t* pi, size_t n_pi) {
  if (!P || !trace) return fail(SBN_ERR_BAD_ARG, "null argument");
  P->fixed_match = false;   // before any check: whatever this call leaves in d_trace, it is no longer known
  int rc = take_public_inputs(P->air, pi, n_pi, false, P->pi); if (rc) return rc;
  size_t words = P->air.ncols * P->n;
  {  // canonical-form check on several host threads (the copy below is the PCIe-bound part)
    unsigned nt = tracegen_host_threads(); if (nt == 0) nt = 1; if (nt > 16) nt = 16;   // (honours SBN_HOST_THREADS)
    std::atomic<size_t> bad(words);
    std::vector<std::thread> th;
    size_t per = (words + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++)
      th.emplace_back([&, t] {
        size_t a = t * per, b = std::min(words, a + per);
        for (size_t i = a; i < b; i++) if (trace[i] >= GLP) { size_t cur = bad.load(); while (i < cur && !bad.compare_exchange_weak(cur, i)) {} break; }
      });
    for (auto& x : th) x.join();
    if (bad.load() < words) return fail(SBN_ERR_NON_CANONICAL, "trace word %zu is not canonical", bad.load());
  }
  HIPC(hipSetDevice(P->device));
  HIPC(hipMemcpy(P->d_trace, trace, words * sizeof(u64), hipMemcpyHostToDevice));
  if ((rc = fixed_columns_check(P))) return rc;
  P->loaded = true;
  return SBN_OK;
}
extern "C" int sbn_prover_load_trace_device(sbn_prover* P, const uint64_t* d_trace, const uint64_t* pi, size_t n_pi) {
  if (!P || !d_trace) return fail(SBN_ERR_BAD_ARG, "null argument");
  P->fixed_match = false;   // (the caller may have written through sbn_prover_trace_device_ptr already)
  int rc = take_public_inputs(P->air, pi, n_pi, false, P->pi); if (rc) return rc;
  HIPC(hipSetDevice(P->device));
  if (d_trace != P->d_trace) HIPC(hipMemcpy(P->d_trace, d_trace, P->air.ncols * P->n * sizeof(u64), hipMemcpyDeviceToDevice));
  if ((rc = fixed_columns_check(P))) return rc;
  P->loaded = true;
  return SBN_OK;
}

extern "C" int sbn_prover_read_trace(sbn_prover* P, uint64_t* out) {
  if (!P || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (!P->loaded) return fail(SBN_ERR_BAD_ARG, "no trace loaded");
  HIPC(hipSetDevice(P->device));
  HIPC(hipMemcpy(out, P->d_trace, P->air.ncols * P->n * sizeof(u64), hipMemcpyDeviceToHost));
  return SBN_OK;
}
extern "C" uint64_t* sbn_prover_trace_device_ptr(sbn_prover* P) {
  if (!P) return nullptr;
  (void)hipSetDevice(P->device);
  return P->d_trace;
}

// ---- column-major traces: streamed into the trace commitment ----------------------------------------------------------------
// The trace of sbn_prover_prove_host_trace crosses PCIe in the commit pipeline's own column chunks: host threads copy a piece of
// the caller's (pageable, possibly read-only) matrix into a slot of the pinned ring (through gather_columns of host_columns.hpp),
// a hipMemcpyAsync on the copy stream moves it to its place in d_trace, and after the last piece of chunk k the copy stream scans
// the chunk for words >= p and records upload_done[k].  A piece never spans two column chunks; a chunk larger than a slot crosses
// in several pieces.  What the trace commitment of prover.hip sees of all this are the four calls below, in this order.
// Begin: the scans' result word, reset on the copy stream in front of the first scan.
int upload_begin(sbn_prover* P, const HostUpload& up) {
  HIPC(hipMemsetAsync(P->d_first_bad, up.reduce ? 0 : 0xff, sizeof(unsigned long long), P->ustream));
  return 0;
}
// Chunk k = columns [c0, c0 + nc): sent and scanned on the copy stream; the main stream, which runs the first transform pass of
// the chunk, waits for it.
int upload_chunk(sbn_prover* P, const HostUpload& up, size_t k, size_t c0, size_t nc) {
  const size_t w0 = c0 * P->n, w1 = w0 + nc * P->n;
  const size_t threads = std::min<size_t>(tracegen_host_threads(), 16);
  for (size_t a = w0; a < w1; a += UPLOAD_SLOT_WORDS) {
    const size_t len = std::min(UPLOAD_SLOT_WORDS, w1 - a);
    u64* slot; unsigned s;
    HIPC(P->upload_ring.claim(&slot, &s));
    const size_t parts = std::max<size_t>(1, std::min(threads, len >> 15)), per = (len + parts - 1) / parts;   // >= 256 KiB per thread
    host_parallel_for(parts, [&](size_t t) { const size_t b0 = t * per, b1 = std::min(len, b0 + per); if (b0 < b1) gather_columns(up.src, a + b0, b1 - b0, slot + b0); });
    HIPC(hipMemcpyAsync(P->d_trace + a, slot, len * sizeof(u64), hipMemcpyHostToDevice, P->ustream));
    HIPC(P->upload_ring.sent(s, P->ustream));
  }
  if (up.reduce) launch_reduce_words(P->d_trace + w0, w1 - w0, P->d_first_bad, P->ustream);
  else launch_first_non_canonical(P->d_trace + w0, w1 - w0, (u64)w0, P->d_first_bad, P->ustream);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(P->upload_done[k], P->ustream));
  HIPC(hipStreamWaitEvent(P->stream, P->upload_done[k], 0));
  return 0;
}
// The result rides back: 8 bytes on the main stream, behind the copy of the trace cap and under the same host wait.
int upload_result_to_host(sbn_prover* P) {
  HIPC(hipMemcpyAsync(P->h_first_bad, P->d_first_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, P->stream));
  return 0;
}
// Verdict, behind that wait: the first word refused, if any (under `reduce` the word is the count, which prove_upload reports).
int upload_verdict(const sbn_prover* P, const HostUpload& up) {
  if (!up.reduce && *P->h_first_bad != ~0ull) return fail(SBN_ERR_NON_CANONICAL, "trace word %zu is not canonical", (size_t)*P->h_first_bad);
  return 0;
}

// load + prove in one call (include/sbn.h): the upload runs inside the trace commitment, the canonical-form check on the device
static int prove_upload(sbn_prover* P, const HostColumns& src, bool reduce, uint64_t* reduced_out, sbn_proof** out) {
  HIPC(hipSetDevice(P->device));
  if (int rc = upload_setup(P)) return rc;
  const HostUpload up{src, reduce};
  const int rc = prove_streamed(P, &up, out);
  if (rc && !guard_refused(P, rc)) { abandon_load(P); return rc; }
  if (reduce && reduced_out) *reduced_out = *P->h_first_bad;   // (the counter came back with the trace cap)
  P->loaded = true;   // (also behind a guard's refusal: the upload and every stage ran, the trace is there for the diagnostics)
  return rc;
}
extern "C" int sbn_prover_prove_host_trace(sbn_prover* P, const uint64_t* trace, const uint64_t* pi, size_t n_pi, sbn_proof** out) {
  if (!P || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  *out = nullptr;
  unload(P);   // (the upload writes d_trace and compares nothing)
  if (!trace) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (P->sp) return fail(SBN_ERR_UNSUPPORTED, "sbn_prover_prove_host_trace covers single-GPU provers");
  if (int rc = take_public_inputs(P->air, pi, n_pi, false, P->pi)) return rc;
  return prove_upload(P, HostColumns{nullptr, trace, P->n}, false, nullptr, out);
}
// the same for a trace held as one allocation per column (csrc/host_columns.hpp); SBN_TRACE_REDUCE: words and public inputs >= p
// are taken mod p (the words on the device, behind the upload) instead of refused
extern "C" int sbn_prover_prove_host_columns(sbn_prover* P, const uint64_t* const* columns, size_t n_columns, uint32_t flags, const uint64_t* pi, size_t n_pi,
                                             uint64_t* reduced_out, sbn_proof** out) {
  if (!P || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  *out = nullptr;
  unload(P);
  if (reduced_out) *reduced_out = 0;
  if (n_columns != P->air.ncols) return fail(SBN_ERR_BAD_ARG, "expected %zu columns, got %zu", P->air.ncols, n_columns);
  if (!columns) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (const size_t bad = gather_columns_refused(columns, n_columns, P->n, 0, n_columns * P->n))
    return fail(SBN_ERR_BAD_ARG, "column %zu is null or not 8-byte aligned", bad - 2);
  if (flags & ~SBN_TRACE_REDUCE) return fail(SBN_ERR_BAD_ARG, "unknown flag bits 0x%x", flags & ~SBN_TRACE_REDUCE);
  const bool reduce = (flags & SBN_TRACE_REDUCE) != 0;
  if (int rc = take_public_inputs(P->air, pi, n_pi, reduce, P->pi)) return rc;
  if (P->sp) return fail(SBN_ERR_UNSUPPORTED, "sbn_prover_prove_host_columns covers single-GPU provers");
  return prove_upload(P, HostColumns{columns, nullptr, P->n}, reduce, reduced_out, out);
}

// ---- row-major traces -------------------------------------------------------------------------------------------------------
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
  return with_pi ? take_public_inputs(as, pi, n_pi, call.reduce, call.pi) : 0;
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
// host_rows.hpp), the copy stream sends it to staging buffer k & 1 and records rows_copied[k & 1], and the main stream transposes it
// into d_trace behind that event and records rows_transposed[k & 1]; the copy of piece k + 2 waits for the transposition of piece k,
// so piece k + 1 is packed and sent while piece k is transposed.  host == null: the rows are at d_rows already, one launch.
// Scratch, carved from the front of the LDE buffer by the carver of the device witness (prover_ctx.hpp LdeScratch): the error words,
// then the one or two staging buffers.
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
    const size_t threads = std::min<size_t>(tracegen_host_threads(), 16);
    for (size_t k = 0; k < pieces; k++) {
      size_t r0 = 0, r1 = 0;
      if (!piece_rows(n, per, k, &r0, &r1)) return fail(SBN_ERR_HIP, "internal: piece %zu of %zu", k, pieces);
      const size_t R = r1 - r0, len = R * n_cols, b = k & 1;
      u64* slot; unsigned s;
      HIPC(P->upload_ring.claim(&slot, &s));
      const size_t parts = std::max<size_t>(1, std::min(std::min(threads, len >> 15), R)), rows_per = (R + parts - 1) / parts;   // >= 256 KiB per thread
      host_parallel_for(parts, [&](size_t t) { const size_t a = r0 + t * rows_per, e = std::min(r1, a + rows_per); if (a < e) copy_rows(*host, a, e, slot + (a - r0) * n_cols); });
      if (k >= 2) HIPC(hipStreamWaitEvent(P->ustream, P->rows_transposed[b], 0));
      HIPC(hipMemcpyAsync(stage + b * stage_words, slot, len * sizeof(u64), hipMemcpyHostToDevice, P->ustream));
      HIPC(P->upload_ring.sent(s, P->ustream));
      HIPC(hipEventRecord(P->rows_copied[b], P->ustream));
      HIPC(hipStreamWaitEvent(P->stream, P->rows_copied[b], 0));
      launch(stage + b * stage_words, n_cols, r0, R);
      HIPC(hipEventRecord(P->rows_transposed[b], P->stream));
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
  if (rc) { abandon_load(P); return rc; }
  if (reduced_out) *reduced_out = call.reduce ? err[1] : 0;
  P->loaded = true;
  return SBN_OK;
}

// the first lines of the three calls with a prover: *reduced_out, the handle, then no trace loaded in front of every other check
int rows_call_begin(sbn_prover* P, uint64_t* reduced_out) {
  if (reduced_out) *reduced_out = 0;
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  unload(P);
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
  if (int rc = rows_call_begin(P, reduced_out)) return rc;
  RowsCall call;
  if (int rc = rows_refused(P->air, P->n, rows, flags, true, pi, n_pi, true, call)) return rc;
  const HostRows m{rows->flat, rows->row_stride, rows->row_ptrs, rows->n_rows, rows->n_cols};
  return load_rows(P, &m, nullptr, 0, m.n_cols, call, reduced_out);
}

extern "C" int sbn_prover_load_trace_rows_device(sbn_prover* P, const uint64_t* d_rows, size_t row_stride, size_t n_cols, uint32_t flags, const uint64_t* pi,
                                                 size_t n_pi, uint64_t* reduced_out) {
  if (int rc = rows_call_begin(P, reduced_out)) return rc;
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
  if (int rc = rows_call_begin(P, reduced_out)) return rc;
  if (!out) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (int rc = sbn_prover_load_trace_rows(P, rows, flags, pi, n_pi, reduced_out)) return rc;
  const int rc = sbn_prover_prove(P, out);
  if (rc && !guard_refused(P, rc)) abandon_load(P);   // a failing call leaves no trace loaded, but for a guard's refusal of the finished proof
  return rc;
}

// ---- building blocks for parity tests ---------------------------------------------------------------------------------------
// The round trip of the scan (reduce: of its reducing twin, and the words come back too): words up, one launch, *result back.  The
// device copy keeps the caller's offset from a 16-byte boundary, so the kernels' unaligned head is reachable from a test.
static int scan_round_trip(const u64* words, u64* words_back, size_t count, unsigned long long* result) {
  const size_t off = ((size_t)words & 8) ? 1 : 0;
  DevWords w;   // d[0]: the result word (the first bad index, all ones: none; or the counter); the data from d + 2 + off
  if (int rc = w.alloc(2 + off + count)) return rc;
  u64* const data = w.d + 2 + off;
  HIPC(hipMemset(w.d, words_back ? 0 : 0xff, sizeof(u64)));
  HIPC(hipMemcpy(data, words, count * sizeof(u64), hipMemcpyHostToDevice));
  if (words_back) launch_reduce_words(data, count, (unsigned long long*)w.d, 0);
  else launch_first_non_canonical(data, count, 0, (unsigned long long*)w.d, 0);
  HIPC(hipGetLastError());
  HIPC(hipMemcpy(result, w.d, sizeof *result, hipMemcpyDeviceToHost));
  if (words_back) HIPC(hipMemcpy(words_back, data, count * sizeof(u64), hipMemcpyDeviceToHost));
  return 0;
}
// Index of the first word >= p, or `count`: the scan of sbn_prover_prove_host_trace as a building block (host in, host out).
extern "C" int sbn_first_non_canonical(const uint64_t* words, size_t count, int on_device, uint64_t* index_out) {
  if (!index_out || (!words && count)) return fail(SBN_ERR_BAD_ARG, "null argument");
  *index_out = count;
  if (!on_device) {
    for (size_t i = 0; i < count; i++) if (words[i] >= GLP) { *index_out = i; break; }
    return SBN_OK;
  }
  if (int rc = use_current_device("no CPU fallback")) return rc;
  if (count == 0) return SBN_OK;
  unsigned long long first = ~0ull;
  if (int rc = scan_round_trip(words, nullptr, count, &first)) return rc;
  if (first != ~0ull) *index_out = first;
  return SBN_OK;
}

// gather_columns of csrc/host_columns.hpp as a building block: what the upload of sbn_prover_prove_host_columns copies into a ring piece
extern "C" int sbn_gather_columns(const uint64_t* const* columns, size_t n_columns, size_t n, size_t word0, size_t len, uint64_t* out) {
  if (const size_t bad = gather_columns_refused(columns, n_columns, n, word0, len)) {
    if (bad == 1) return fail(SBN_ERR_BAD_ARG, "words %zu + %zu lie beyond the %zu x %zu matrix", word0, len, n_columns, n);
    return fail(SBN_ERR_BAD_ARG, "column %zu is null or not 8-byte aligned", bad - 2);
  }
  if (len && !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  gather_columns(HostColumns{columns, nullptr, n}, word0, len, out);
  return SBN_OK;
}
// In place: words >= p become w - p; *reduced_out (optional) = how many changed.  reduce_words_kernel of SBN_TRACE_REDUCE as a
// building block (host in, host out), or the host loop.
extern "C" int sbn_reduce_words(uint64_t* words, size_t count, int on_device, uint64_t* reduced_out) {
  if (!words && count) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (reduced_out) *reduced_out = 0;
  if (!on_device) {
    const uint64_t changed = reduce_words_host(words, count);
    if (reduced_out) *reduced_out = changed;
    return SBN_OK;
  }
  if (int rc = use_current_device("no CPU fallback")) return rc;
  if (count == 0) return SBN_OK;
  unsigned long long changed = 0;
  if (int rc = scan_round_trip(words, words, count, &changed)) return rc;
  if (reduced_out) *reduced_out = changed;
  return SBN_OK;
}
