// The prover context, declarations only: what one sbn_prover holds between create and destroy.  Included by prover.hip, by
// tracegen_device.hip and trace_load.hip (which fill the trace), by trace_check.hip, trace_explain.hip, trace_explain_fq12.hip,
// perm_diff.hip and witness_diff.hip (the diagnostics of a loaded trace; what their host forms share is trace_host.hpp) and by
// lde_compact.hip (the launchers of the compact storage); every other unit reaches the prover through the C ABI of include/sbn.h.
#pragma once
#include "host_common.hpp"
#include "settings.hpp"
#include "pinned_ring.hpp"
#include <algorithm>

using namespace sbn;
struct PairCols;   // kernels.cuh

#define HIPC(expr)                                                                                   \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return fail(SBN_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// Stage k spans [ev[k], ev[k+1]) on the prover's main stream.  The commit stages overlap NTT (main
// stream) with sponge absorption (hash stream); the absorption kernels are additionally timed one by
// one with events on the hash stream (EXTRA_* entries = sum over the chunk launches of one proof).
enum Stage {
  ST_TRACE_COMMIT, ST_PERM_Z, ST_Z_COMMIT, ST_QUOTIENT_EVAL, ST_QUOTIENT_COMMIT,
  ST_OPENINGS, ST_FRI_COMBINE, ST_FRI_LAYERS, ST_POW, ST_QUERIES, ST_COUNT
};
enum Extra { EX_TRACE_ABSORB_MS, EX_TRACE_ABSORB_LAUNCHES, EX_Z_ABSORB_MS, EX_Z_ABSORB_LAUNCHES, EX_TRACEGEN_MS, EX_COMM_MS, EX_COUNT };
// The diagnostics of a loaded trace and the times each keeps of its last call (sbn_prover.diag_ms):
//   DIAG_CHECK    sbn_prover_check_trace           4: permutation Z, constraint kernels, reduction, download
//   DIAG_EXPLAIN  sbn_prover_explain_*             3: permutation Z, explain kernels, reduction / download
//   DIAG_PERMDIFF sbn_prover_explain_permutations  3: histogram, rows pass, download + host merge
//   DIAG_WITDIFF  sbn_prover_diff_witness          3: device witness, compare kernel, listing + downloads
enum Diag { DIAG_CHECK, DIAG_EXPLAIN, DIAG_PERMDIFF, DIAG_WITDIFF, DIAG_COUNT };
static constexpr int MAX_CHUNKS = 512;
// The pinned staging ring of one prover (pinned_ring.hpp; trace_load.hip): 4 slots of 16 MiB = 64 MiB of pinned host memory,
// allocated by the first call that uploads a host trace.
static constexpr unsigned UPLOAD_SLOTS = 4;
static constexpr size_t UPLOAD_SLOT_WORDS = (size_t)2 << 20;
// Function attributes are per DEVICE: one flag per device of the process (sbn_set_device may select another GPU later).
static constexpr int SBN_MAX_DEVICES = 64;
// Compact LDE storage (include/sbn.h SBN_LDE_COMPACT): slots of the LDE chunk ring at most; create_ctx picks LDE_RING_DEPTH
static constexpr int LDE_RING_MAX = 3;
static constexpr u32 LDE_RING_DEPTH = 2;

struct DevTree {  // Merkle digests, levels concatenated (leaf level first)
  u64* d = nullptr; size_t nleaf = 0; u32 nlevels = 0;  // nlevels = number of levels BELOW the cap
  u64* level(u32 l) const { return d + (2 * nleaf - ((2 * nleaf) >> l)) * 4; }
};

// Oversized-trace split (include/sbn.h, sbn_split_prover_*): this rank's share of one proof.
// The columns of a matrix are dealt to the ranks in blocks of `ob` columns, round-robin: rank r owns the blocks
// b = r, r + R, r + 2R, ... and keeps them compactly (own block k = global block k * R + r at local columns k * ob ...);
// only the globally last block can be short, and it is the last own block of its owner.  In step k of a commitment every
// rank transforms its own block k, the all-to-all of that step moves the blocks k * R .. k * R + R - 1 to their row
// owners, and the leaf sponge -- sequential over the columns of a row -- absorbs exactly those blocks next.
struct ColShare {
  size_t total = 0, ob = 64; u32 R = 1, rank = 0;
  size_t nblocks() const { return (total + ob - 1) / ob; }
  size_t steps() const { return (nblocks() + R - 1) / R; }
  size_t block_cols(size_t b) const { return b < nblocks() ? std::min(ob, total - b * ob) : 0; }
  size_t own_cols(u32 r) const { size_t s = 0; for (size_t b = r; b < nblocks(); b += R) s += block_cols(b); return s; }
  size_t own() const { return own_cols(rank); }
  size_t max_own() const { size_t s = 0; for (u32 r = 0; r < R; r++) s = std::max(s, own_cols(r)); return s; }
  size_t global_col(u32 r, size_t local) const { return ((local / ob) * R + r) * ob + local % ob; }   // of rank r's local column
};
struct SplitCtx {
  sbn_comm comm;
  u32 log_r = 0, rho = 0;                 // world = 2^log_r; this rank owns the LDE rows i = j * world + rho
  size_t ml = 0;                          // local LDE rows = m >> log_r
  ColShare cs, zs;                        // trace / Z columns of this rank
  size_t cr = 0, zr = 0;                  // = cs.own(), zs.own()
  u32 planes = 1;                         // 2 from four ranks up: the rows i + 2 of the local rows arrive as a second plane
  u64 *lde_l = nullptr, *lde_n = nullptr, *zlde_l = nullptr, *zlde_n = nullptr, *scratch = nullptr;   // views of comm.recv_buf
  size_t scratch_words = 0;
  size_t slot_words = 0;                  // one send slot = [plane][dest][ob][ml]; two slots, used alternately by the steps
  u64* d_ldechunk = nullptr;              // [ntt_chunk][m]: one column block of this rank's LDE before it is packed
  u32* d_idx_local = nullptr;             // query leaf indices inside this rank's subtrees
  PairCols* d_pairs_own = nullptr;        // permutation pairs of the own Z columns, local order
  hipStream_t cstream = nullptr;          // the exchanges of the commit pipeline
  hipEvent_t xchg_done[MAX_CHUNKS];       // comm stream: the blocks of step k have arrived (and send slot k & 1 is free again)
  std::vector<hipEvent_t> tev;            // timing events around the exchanges (pairs), consumed in order
  size_t tev_used = 0;
};

struct sbn_prover {
  AirShape air; sbn_config cfg; FriShape fri;
  SplitCtx* sp = nullptr;                 // null: the whole proof on this GPU
  size_t lde_scratch_words = 0;           // capacity of d_lde as witness-generation scratch
  // SBN_LDE_COMPACT: a matrix of more than 4 columns keeps only the quotient's rows of its LDE, d_lde = [C][qn] and d_zlde = [Z][qn]
  // (dense, point j = LDE row j << (rate_bits - 1)); the LDE of a column chunk passes through a ring slot [ntt_chunk][m] between its
  // last transform pass and the sponge, and the opened rows are recomputed from the coefficients (lde_compact.hip)
  u32 lde_storage = 0;                    // SBN_LDE_FULL / SBN_LDE_COMPACT as asked for
  bool compact = false;                   // ... and in effect: compact storage and a table of more than 4 columns
  u32 ring_depth = 0;
  u64* d_ring = nullptr;                  // [ring_depth][ntt_chunk][m]
  hipEvent_t ring_free[MAX_CHUNKS] = {};  // hash stream: the sponge and lde_keep_rows_kernel have left the slot of chunk k (one event per chunk, as chunk_ready)
  u32 degree_bits, lde_log; size_t n, m;
  int device; hipStream_t stream;
  // matrices
  u64 *d_trace = nullptr, *d_coef = nullptr, *d_lde = nullptr, *d_tmp = nullptr;
  u64 *d_zval = nullptr, *d_zcoef = nullptr, *d_zlde = nullptr;
  u64 *d_q = nullptr, *d_qlde = nullptr;
  DevTree tree_t, tree_z, tree_q;
  std::vector<DevTree> fri_trees;
  // tables
  u64 *d_tw_f = nullptr, *d_tw_i = nullptr, *d_shift = nullptr, *d_shift_inv = nullptr;
  u64 *d_shift_odd = nullptr;   // 2^19-point LDE (1,024 x 512): 7^i w_1024^(i >> 9), the input scale of the odd half of its split first pass
  u32 lde_za_log = 0;           // rate_bits >= 2 at 2^16 / 2^17 rows: the LDE's first pass as 2^lde_za_log zero-aware 256-point passes (= rate_bits; 0: off)
  u64 *d_shift_za = nullptr;    // its input scales [2^lde_za_log][n]: 7^i w^(v * row of i), w of order 256 * 2^lde_za_log (prover.hip lde_za_tables)
  u64 *d_xs = nullptr, *d_lag_first = nullptr, *d_lag_last = nullptr;   // per QUOTIENT point: the coset of 2n points
  u64 *d_apow = nullptr;  // [2][apow_n]
  size_t apow_n = 0;
  void* d_pic = nullptr;  // ExpPiConsts<F>
  PairCols* d_pairs = nullptr;
  // openings / FRI
  u64 *d_zpow = nullptr;        // 4 planes [n]: z^i (a,b), (g z)^i (a,b)
  u64 *d_open = nullptr;        // [(ncols + nzs + 4)][4]
  u64 *d_part = nullptr;        // 2 planes [groups][n] = 64 n words; also the quotient's 8 planes of 2n and the trace check's of n
  u64 *d_w = nullptr;           // group weights
  u64 *d_fa = nullptr, *d_fb = nullptr;    // F0 / F1 scratch planes [n] each (a,b) x2
  u64 *d_fcoef = nullptr;       // final poly coefficient planes [2][m]
  u64 *d_fcoef2 = nullptr;      // ping-pong for folding [2][m/2^arity]
  std::vector<u64*> fri_vals;   // per layer value planes [2][size]
  u64 *d_pow = nullptr;
  u32 *d_idx = nullptr;
  u64 *d_qbuf = nullptr; size_t qstride = 0;
  std::vector<u64> pi;
  bool loaded = false;
  // The shape-constant trace columns [fixed_f0, fixed_f1) of an Exp table (host_common.hpp fixed_columns_range; empty: none, or a
  // context that never reuses them: the split, compact storage, SBN_FIXED_COLUMNS=0).  Their coefficients and LDE are the same words
  // in every proof of this context, so stage_trace_commit leaves them where an earlier proof put them:
  bool fixed_match = false;                  // those columns of the resident d_trace hold the generators' words (every writer of d_trace sets or clears it)
  bool fixed_valid = false;                  // those columns of d_coef and d_lde hold the transforms of the generators' words (every writer of either keeps or clears it)
  size_t fixed_f0 = 0, fixed_f1 = 0;
  size_t fixed_skipped = 0;                  // trace columns the last prove() left untransformed (sbn_prover_describe)
  hipEvent_t ev[ST_COUNT + 1];
  float stage_ms[ST_COUNT + EX_COUNT];
  size_t ntt_chunk;
  bool ntt_fused = false;                    // the inverse transform's pass B and the LDE's pass A as ONE kernel (2^16 / 2^17 rows)
  u64* d_tmp2 = nullptr;                     // its output: the fused kernel cannot work in place
  u64* d_tmp3 = nullptr;                     // 2^18 rows, two transform streams: the fused kernel's second output buffer (chunks alternate)
  bool ntt_fused512 = false;                 // 2^18-row tables: kernels_ntt.cuh ntt_fused512_inv_b_lde_a_kernel
  hipStream_t hstream = nullptr;             // sponge absorption / Merkle stream
  hipStream_t nstream = nullptr;             // second transform stream (2^19 LDE rows and up): the LDE of chunk k beside the inverse transform of chunk k+1
  hipEvent_t intt_done[MAX_CHUNKS];          // main -> second transform stream: the coefficients of chunk k are complete
  bool ntt_two_streams = false;
  Settings set;                              // the SBN_* switches this prover was created under (settings.hpp)
  int chain_mode = 0;                        // curve witness: 0 host pool, 1 one lane per instance, 2 one wave per instance
  hipEvent_t chunk_ready[MAX_CHUNKS];        // main -> hash: LDE chunk k is complete
  hipEvent_t abs_ev[2 * MAX_CHUNKS];         // hash stream: before/after each absorb launch
  hipEvent_t hash_done;                      // hash -> main
  u64* d_sponge = nullptr;                   // [12][m] sponge state carried between column chunks
  u64* h_chain = nullptr;                    // pinned staging for the host-computed curve chains (device tracegen)
  size_t h_chain_words = 0;
  u64* h_io = nullptr;                       // pinned staging of the device witness: the instance list in, the outputs + error word back
  size_t h_io_words = 0;
  u64* h_open = nullptr;                     // pinned landing buffer of the opened values [(ncols + nzs + 4)][4]
  u64* h_open2 = nullptr;                    // second landing buffer: the values at g*zeta of the trace and Z columns (the host is still reading the first)
  u64* h_w = nullptr;                        // pinned source of the FRI combine weights (d_w, at most 4,096 words)
  // Every device allocation of this context, in allocation order: alloc_buffers (prover.hip) is the one place that allocates and
  // pushes here, sbn_prover_destroy frees this list and names no device buffer.  The d_* members above are views of its entries.
  std::vector<void*> owned;
  size_t dev_bytes = 0;                      // their bytes (what sbn_prover_memory_plan predicts and the one-shot cache of capi.hip counts)
  // The host-trace uploads (trace_load.hip), created by the first of them (upload_setup): the trace crosses PCIe on the copy stream
  // through a ring of pinned slots
  hipStream_t ustream = nullptr;             // copy stream: pieces of the trace, then the canonical-form scan of each chunk
  PinnedRing upload_ring;
  hipEvent_t upload_done[MAX_CHUNKS];        // copy stream: column chunk k is resident and scanned (prove_host_trace, prove_host_columns)
  hipEvent_t rows_copied[2] = {};            // copy stream: a piece of a row-major load has landed in staging buffer b
  hipEvent_t rows_transposed[2] = {};        // main stream: its transposition has left staging buffer b
  unsigned long long* d_first_bad = nullptr; // smallest index of a trace word >= p (all ones: none), folded by the scans
  unsigned long long* h_first_bad = nullptr; // its pinned landing word
  float diag_ms[DIAG_COUNT][4] = {};         // the times of the last call of each diagnostic (enum Diag), what its *_times getter copies
  size_t permdiff_routes[3] = {};            // sbn_prover_explain_permutations: pairs of its last call answered by the bins alone, with the overflow list, from downloaded columns
  // Verified proving (include/sbn.h sbn_prover_set_guard; guard.hip): with a mode set, prove_streamed hands the assembled proof to
  // guard_check before it returns.  The device verifier (batch 1, its own stream and buffers, outside `owned` and the memory plan)
  // is created by the first proof a device guard checks and lives until the context is destroyed.
  u32 guard_mode = 0;                        // SBN_GUARD_OFF / _DEVICE / _HOST
  sbn_verifier* guard_verifier = nullptr;
  uint64_t guard_checked = 0, guard_rejected = 0, guard_ns = 0;
};

// guard.hip: the guard of a context whose guard_mode is set, on the proof prove_streamed has just assembled.  SBN_OK: *out verified.
// Otherwise *out is freed and nulled; SBN_ERR_VERIFY_FAILED carries the verifier's reason as the message.  Touches no stream of P.
int guard_check(sbn_prover* P, sbn_proof** out);
// the guard refused a finished proof: every stage ran, so the trace the call loaded is resident and stays loaded (trace_load.hip)
static inline bool guard_refused(const sbn_prover* P, int rc) { return rc == SBN_ERR_VERIFY_FAILED && P->guard_mode != SBN_GUARD_OFF; }
// guard.hip: device bytes of the context's guard; sbn_prover_destroy's share
size_t guard_device_bytes(const sbn_prover* P);
void guard_destroy(sbn_prover* P);

// Scratch of the calls that fill d_trace (the device witness generators of tracegen_device.hip, the row-major loads of
// trace_load.hip), carved from the front of the LDE buffer, which is not in use between proofs (a split prover: its receive buffer).
struct LdeScratch {
  sbn_prover* const P;
  u64* const wbase;
  u64* w;
  explicit LdeScratch(sbn_prover* P) : P(P), wbase(P->sp ? (u64*)P->sp->comm.recv_buf : P->d_lde), w(wbase) {}
  u64* take(size_t words) { u64* r = w; w += (words + 7) & ~(size_t)7; return r; }
  // after the last take().  The scratch is about to be written: resident transforms of the shape-constant columns (fixed_valid;
  // d_lde columns [fixed_f0, fixed_f1) of P->m words each) survive only if it ends in front of them.
  int fits() {
    const size_t used = (size_t)(w - wbase);
    if (!wbase || used > P->lde_scratch_words) return fail(SBN_ERR_UNSUPPORTED, "scratch does not fit");
    if (P->sp || P->compact || used > P->fixed_f0 * P->m) P->fixed_valid = false;
    return 0;
  }
};

// prover.hip, shared with trace_check.hip: the pieces of the permutation and quotient stages that the trace check runs on the
// trace domain.  All of them enqueue on the prover's streams and leave the waiting to the caller.
struct QuotientParams;   // kernels_quotient.cuh
// Z columns [0, cnt) of `pairs` from P->d_trace into out[cnt][n] on stream s (the chunked form from 2^13 rows up uses P->d_part)
void launch_perm_z(sbn_prover* P, const PairCols* pairs, size_t cnt, u64 gamma0, u64 gamma1, u64* out, hipStream_t s);
// alpha^k tables into P->d_apow and, for the Exp tables, ExpPiConsts into P->d_pic; waits for the uploads (their sources are locals)
int upload_alpha_tables(sbn_prover* P, const F alphas[SBN_NCH]);
// alpha, apow, num_zs, num_io, pic, seg_count, zsplit, seg_shift, lookups_in_perm and seg_mask = 15 of qp
void quotient_segments(const sbn_prover* P, const F alphas[SBN_NCH], QuotientParams& qp);
// quotient_kernel<kind, 0 / 1> on P->stream, <kind, 2> on P->hstream
int launch_quotient_parts(sbn_prover* P, const QuotientParams& qp, size_t qblocks);
// lde_compact.hip: the two stages of the compact LDE storage.  Both enqueue on `s` and leave the waiting to the caller.
// dense[c][j] = slot[c][j << row_log] for c < nc, j < qn (slot columns m words apart, dense columns qn)
void launch_lde_keep_rows(const u64* slot, size_t m, u64* dense, size_t qn, u32 row_log, size_t nc, hipStream_t s);
// the opened rows of `ncols` columns from their coefficients [ncols][n]: out[q * qstride + off + c] = sum_j coef[c][j] x_q^j at
// x_q = 7 w_m^bitrev(idx[q]), q < nq, what gather_rows_kernel reads out of a resident LDE.  table: 64 n words of scratch.
int launch_query_rows(const u64* coef, size_t ncols, size_t n, u32 lde_log, const u64* shift, const u64* tw_f, const u32* d_idx, u32 nq, u64* table,
                      u64* out, size_t qstride, size_t off, hipStream_t s);
// tracegen_device.hip: *d_mismatch = 0, then 1 unless `block` -- the ncols columns of fixed_columns_range() of a trace of n rows --
// holds the words the device witness writes there (kernels_tracegen.cuh fixed_columns_check_kernel).  Enqueues on `s`.
int launch_fixed_columns_check(const u64* block, size_t ncols, size_t n, const ExpShape& sh, unsigned long long* d_mismatch, hipStream_t s);
// prover.hip, for trace_load.hip.  alloc_buffers: the one place that allocates device memory of a context (P->owned, P->dev_bytes).
// prove_streamed: sbn_prover_prove with the trace still on the host (up != null): the trace commitment streams it in.
struct BufReq { void** slot; size_t bytes; };
int alloc_buffers(sbn_prover* P, const std::vector<BufReq>& L);
struct HostUpload;   // trace_load.hip
int prove_streamed(sbn_prover* P, const HostUpload* up, sbn_proof** out);
// trace_load.hip, for the trace commitment of prover.hip -- all it sees of a streamed upload, in this order: the result word reset
// (copy stream); per column chunk k = columns [c0, c0 + nc), its pieces sent and scanned (copy stream) and the main stream made to
// wait for them; the result word on its way back (main stream, behind the cap's copy); and, behind the host wait, the verdict:
// SBN_ERR_NON_CANONICAL naming the first word refused, or 0.  upload_destroy: sbn_prover_destroy's share (ring, events, copy stream).
int upload_begin(sbn_prover* P, const HostUpload& up);
int upload_chunk(sbn_prover* P, const HostUpload& up, size_t k, size_t c0, size_t nc);
int upload_result_to_host(sbn_prover* P);
int upload_verdict(const sbn_prover* P, const HostUpload& up);
void upload_destroy(sbn_prover* P);
// Device words that are freed on every return path: the buffer of the upload / run one kernel / download entry points.
struct DevWords {
  u64* d = nullptr;
  ~DevWords() { if (d) (void)hipFree(d); }
  int alloc(size_t words) { HIPC(hipMalloc((void**)&d, words * sizeof(u64))); return 0; }
};
// tracegen_device.hip: the columns [num_main, num_columns) of an Exp table from the main columns resident in d_trace, by the
// kernels of the device witness (periodic pulse, io pulses, table column, then the table's range-check launches) on P->stream;
// waits, and on success leaves the prover loaded with fixed_match set.  The caller has made sure that no range-checked main
// column holds a word >= 2^16 (the range-check kernels index LDS by the value) and that the table and height are covered
// (derived_columns_covered: SBN_OK, or SBN_ERR_UNSUPPORTED with the message).
int derived_columns_covered(const AirShape& as, size_t n);
int launch_derived_columns(sbn_prover* P);
// What every *_times getter of the C ABI does: the first min(cap, count) of src into ms_out; returns the number written.
static inline int copy_times(const float* src, int count, float* ms_out, int cap) {
  if (!ms_out) return 0;
  const int k = std::min(cap, count);
  for (int i = 0; i < k; i++) ms_out[i] = src[i];
  return k;
}
// trace_check.hip: the way into a device diagnostic of the loaded trace.  diag_refuse_split: SBN_ERR_UNSUPPORTED "<what> runs on
// single-GPU provers ..." for a split context of more than one rank, with any_split of any size.  diag_enter: the refusals the
// diagnostics share, in this order -- a null context, the split as above, no trace loaded -- then the context's device made current;
// the caller goes on with P->stream and P->ev (the stage events are idle outside prove()).
int diag_refuse_split(const sbn_prover* P, const char* what, bool any_split);
int diag_enter(sbn_prover* P, const char* what, bool any_split);
// trace_check.hip: what the trace check and explain set up on the device before their own kernels.  The challenges of `seed`; Z of
// the loaded trace into P->d_zval between ev[0] and ev[1]; the tables of H (g^i, [i == 0], [i == n - 1]) in the first three planes
// of P->d_zpow; the alpha tables (upload_alpha_tables); last = 1 / g.  All on P->stream.
struct TraceDomain {
  F gamma0, gamma1, alphas[SBN_NCH];
  const u64 *xs, *lag_first, *lag_last;
  u64 last;
};
int trace_domain_setup(sbn_prover* P, uint64_t seed, TraceDomain& td);
