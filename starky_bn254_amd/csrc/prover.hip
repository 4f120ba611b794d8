// Host orchestration of prove() on one MI355X: replaces starky prover.rs `prove` for the reference's
// G1 tables (call sites src/curves/g1/exp.rs:818-825, src/curves/g1/muladd.rs:669-676).  The host
// owns only the Fiat-Shamir transcript and proof assembly; every polynomial / hashing / constraint
// stage runs in the kernels of kernels.cuh on one HIP stream.
#include "prover_ctx.hpp"
#include "kernels.cuh"
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <thread>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>

namespace sbn { thread_local std::string g_last_error; }

// sbn_set_device: the device of the provers created afterwards by the calling thread, and the default of threads that never
// chose one; sbn_set_thread_device: the calling thread only (the ranks of a local split group are threads with one device each:
// they must not move the process default under the main thread).  Both also make it HIP's current device of the calling thread,
// so that a plain-C caller's next HIP-level step (sbn_rccl_comm_create allocates its staging buffers) lands on the same GPU.
static std::atomic<int> g_default_device{0};
static thread_local int t_device = -1;
static inline int cur_device() { return t_device >= 0 ? t_device : g_default_device.load(); }
#define g_device (cur_device())
namespace sbn {
int current_device() { return cur_device(); }   // transport.hip
int use_current_device(const char* why) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SBN_ERR_NO_DEVICE, "no HIP device available: %s", why);
  HIPC(hipSetDevice(g_device));
  return 0;
}
}  // namespace sbn

static const char* STAGE_NAMES[ST_COUNT + EX_COUNT] = {
  "trace_commit", "perm_z", "z_commit", "quotient_eval", "quotient_commit",
  "openings", "fri_combine", "fri_layers", "pow", "queries",
  "trace_absorb_kernels_ms", "trace_absorb_launches", "z_absorb_kernels_ms", "z_absorb_launches", "device_tracegen_ms",
  "split_exchange_ms"};

static inline dim3 blocks(size_t k) { return dim3((unsigned)((k + 255) / 256)); }   // workgroups of 256 threads over k items

// ---- device memory of a context ---------------------------------------------------------------------
// Every device buffer of a context -- the list of ctx_buffers, the lazy scan word of prove_host_trace (trace_load.hip), the buffers of a scratch
// context -- is allocated here and nowhere else: the pointer joins P->owned, which is all that sbn_prover_destroy frees, and the
// bytes join P->dev_bytes.  Stops at the first failure; what was allocated until then is in `owned` already.
int alloc_buffers(sbn_prover* P, const std::vector<BufReq>& L) {
  for (const BufReq& b : L) {
    const hipError_t e = hipMalloc(b.slot, b.bytes);
    if (e != hipSuccess) { *b.slot = nullptr; return fail(SBN_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(e)); }
    P->owned.push_back(*b.slot);
    P->dev_bytes += b.bytes;
  }
  return 0;
}
static inline BufReq words_req(u64** p, size_t words) { return BufReq{(void**)p, words * sizeof(u64)}; }

// ---- NTT driver -----------------------------------------------------------------------------------
static u32 pick_log_t(u32 log_r, u32 log_s) {
  u32 lt = 4;
  while (lt > 0 && ((size_t)(1u << log_r) * ((1u << lt) + 1) * 8) > 48 * 1024) lt--;
  return std::min(lt, log_s);
}
// One full n-point transform per column (two passes through `tmp`).
static int ntt_columns(sbn_prover* P, const u64* in, size_t in_cs, u64* out, size_t out_cs, u64* tmp, size_t tmp_cs, size_t ncols,
                       u32 log_n, bool inverse, size_t n_in, const u64* pre, const u64* post, u64 scale, hipStream_t st = nullptr, int which = 3) {
  if (ncols == 0) return 0;                 // which: bit 0 = pass A (in -> tmp), bit 1 = pass B (tmp -> out)
  if (!st) st = P->stream;
  u32 log_n1 = (log_n + 1) / 2, log_n2 = log_n - log_n1;
  // The coset LDE of an r-bit blowup at 2^16 / 2^17 rows (ntt_plan): rows n.. of the input are zero, so the transform is cut as
  // (256 * 2^r) x (n / 256): the first pass then has exactly 256 non-zero rows, and a 2^r * 256-point DFT of 256 inputs is 2^r
  // pre-twisted 256-point DFTs (kernels_ntt.cuh ntt_lde_first_pass_kernel on grid.z), none of which loads or butterflies a zero.
  const bool za = !inverse && P->lde_za_log && log_n == P->lde_log && n_in == P->n && pre == P->d_shift && P->d_shift_za;
  if (za) { log_n1 = 8 + P->lde_za_log; log_n2 = log_n - log_n1; }
  size_t n1 = (size_t)1 << log_n1, n2 = (size_t)1 << log_n2;
  NttPassParams a{};
  a.in = in; a.out = tmp; a.in_col_stride = in_cs; a.out_col_stride = tmp_cs;
  a.log_r = log_n1; a.log_t = pick_log_t(log_n1, log_n2); a.log_n = log_n;
  a.in_sr = n2; a.in_st = 1; a.out_sr = n2; a.out_st = 1; a.n_in = n_in;
  a.r_fast_load = 0; a.twiddle = 1; a.tw = inverse ? P->d_tw_i : P->d_tw_f; a.tw_log = P->lde_log;
  a.pre = pre; a.post = nullptr; a.scale = 1;
  NttPassParams b{};
  b.in = tmp; b.out = out; b.in_col_stride = tmp_cs; b.out_col_stride = out_cs;
  b.log_r = log_n2; b.log_t = pick_log_t(log_n2, log_n1); b.log_n = log_n;
  b.in_sr = 1; b.in_st = n2; b.out_sr = n1; b.out_st = 1; b.n_in = (size_t)1 << log_n;
  b.r_fast_load = 1; b.twiddle = 0; b.tw = a.tw; b.tw_log = P->lde_log;
  b.pre = nullptr; b.post = post; b.scale = scale;
  for (size_t c0 = 0; c0 < ncols; c0 += 32768) {
    size_t nc = std::min<size_t>(32768, ncols - c0);
    NttPassParams pa = a, pb = b;
    pa.in = a.in + c0 * in_cs; pa.out = a.out + c0 * tmp_cs;
    pb.in = b.in + c0 * tmp_cs; pb.out = b.out + c0 * out_cs;
    dim3 ga((unsigned)(n2 >> pa.log_t), (unsigned)nc), gb((unsigned)(n1 >> pb.log_t), (unsigned)nc);
    size_t la = ((size_t)1 << pa.log_r) * ((1u << pa.log_t) + 1) * 8, lb = ((size_t)1 << pb.log_r) * ((1u << pb.log_t) + 1) * 8;
    const u32 kperm = inverse ? 11u : 5u;  // omega_16 = (2^12)^13, omega_16^-1 = (2^12)^3: 13^-1 = 5, 3^-1 = 11 (mod 16)
    auto launch = [&](NttPassParams q, dim3 grid, size_t lds_bytes) {
      const bool fast = q.log_t == 4 && (q.log_r == 8 || q.log_r == 9);
      if (fast) { q.xcd_order = 1; std::swap(grid.x, grid.y); }   // (columns, tiles) grid order (kernels_ntt.cuh NttPassParams::xcd_order)
      if (fast && q.log_r == 8) hipLaunchKernelGGL(ntt_fast_pass_kernel<0>, grid, dim3(256), 16 * 272 * 8, st, q, kperm);
      else if (fast) hipLaunchKernelGGL(ntt_fast_pass_kernel<1>, grid, dim3(256), 32 * 272 * 8, st, q, kperm);
      else hipLaunchKernelGGL(ntt_pass_kernel, grid, dim3(NTT_THREADS), lds_bytes, st, q);
    };
    if (pa.log_r == 9 && log_n2 >= 4) pa.log_t = 4;  // the fast kernel always uses 16-wide tiles
    if (pb.log_r == 9 && log_n1 >= 4) pb.log_t = 4;
    // 1,024-point first pass over an input whose rows 512.. are zero (the 2^19-point coset LDE): two 512-point fast passes
    // on grid.z (kernels_ntt.cuh NttPassParams::split) instead of the generic radix-2 pass
    const bool split_a = !inverse && pa.log_r == 10 && log_n2 >= 4 && pa.in_st == 1 && n_in <= (size_t)512 * pa.in_sr && pre == P->d_shift && P->d_shift_odd;
    if (split_a) { pa.log_r = 9; pa.log_t = 4; pa.split = 1; pa.pre2 = P->d_shift_odd; }
    ga = dim3((unsigned)(n2 >> pa.log_t), (unsigned)nc, split_a ? 2u : 1u); gb = dim3((unsigned)(n1 >> pb.log_t), (unsigned)nc);
    la = ((size_t)1 << pa.log_r) * ((1u << pa.log_t) + 1) * 8; lb = ((size_t)1 << pb.log_r) * ((1u << pb.log_t) + 1) * 8;
    if (za) {   // pa as 2^r passes of 256 points: sub-pass v reads the rows scaled by d_shift_za[v] and writes the rows k * 2^r + v
      pa.log_r = 8; pa.log_t = 4; pa.split = P->lde_za_log; pa.pre = nullptr; pa.pre2 = P->d_shift_za; pa.xcd_order = 1;
      if (which & 1) hipLaunchKernelGGL(ntt_lde_first_pass_kernel, dim3((unsigned)nc, (unsigned)(n2 >> 4), 1u << P->lde_za_log), dim3(256), 16 * 272 * 8, st, pa, kperm);
    } else if (which & 1) launch(pa, ga, la);
    if (which & 2) launch(pb, gb, lb);
  }
  HIPC(hipGetLastError());
  return 0;
}

static u64 host_inv_pow2(u32 k) { return f_inv(F((u64)1 << k)).v; }
// the R = 512 fast pass needs 69,632 bytes of dynamic LDS (> the 64 KiB default)
static int ntt_fast_setup() {  // idempotent, so a race between prover threads is harmless; the flag only saves the call
  static std::atomic<bool> done[SBN_MAX_DEVICES];
  const int d = g_device >= 0 && g_device < SBN_MAX_DEVICES ? g_device : 0;
  if (!done[d].load()) {
    HIPC(hipFuncSetAttribute((const void*)ntt_fast_pass_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 32 * 272 * 8));
    HIPC(hipFuncSetAttribute((const void*)ntt_fused_inv_b_lde_a_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 32 * 272 * 8));
    HIPC(hipFuncSetAttribute((const void*)ntt_fused512_inv_b_lde_a_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 32 * 272 * 8));
    done[d].store(true);
  }
  return 0;
}
// The transform kernels of a table, a function of its height and rate_bits alone.  create_ctx and ScratchCtx both pick them
// here, so the parity tests of sbn_commit_values run the kernels the prover runs.  rate_bits 1 -- 2^16 / 2^17 rows: the fused middle
// pass (its geometry is that of a 2n-point LDE); 2^18 rows (the 2^19-point LDE): its 512-point form, and the LDE's 1,024-point
// first pass as two 512-point halves -- both read d_shift_odd, which the callers allocate exactly when ntt_fused512 is set.
// rate_bits r >= 2 -- 2^16 / 2^17 rows: the LDE's first pass skips the zero rows (ntt_columns, lde_za_log), and reads the
// pre-twisted coset tables d_shift_za, which the callers allocate and fill (lde_za_tables) exactly when lde_za_log is set.
static void ntt_plan(sbn_prover* P) {
  const u32 rate = P->lde_log - P->degree_bits;
  P->ntt_fused = rate == 1 && (P->degree_bits == 16 || P->degree_bits == 17);
  P->ntt_fused512 = P->degree_bits == 18 && P->lde_log == 19;
  P->lde_za_log = (rate >= 2 && (P->degree_bits == 16 || P->degree_bits == 17)) ? rate : 0;
}
// d_shift_za[v][i] = 7^i w^(v * (i >> log_s)), v < 2^lde_za_log, i < n, with w the root of order 2^(8 + lde_za_log) and
// log_s = lde_log - 8 - lde_za_log (the row of coefficient i in the zero-aware first pass is i >> log_s, below 256)
static void lde_za_tables(sbn_prover* P) {
  const u32 log_s = P->lde_log - 8 - P->lde_za_log;
  hipLaunchKernelGGL(shift_za_table_kernel, dim3((unsigned)((P->n + 255) / 256), 1u << P->lde_za_log), dim3(256), 0, P->stream, P->d_shift_za, P->n, P->d_shift,
                     P->d_tw_f, log_s);
}
// The tables of the transforms, on P->stream: of a real context (create_ctx) and of a scratch context alike, each table exactly
// when its buffer is allocated.
// d_tw_f / d_tw_i: FULL root tables (w^i for every i < m: the second half is the negated first): the register passes index them
// without the compare / negate of a half table (tw_full, kernels_ntt.cuh); everything else reads the first half only
static void fill_transform_tables(sbn_prover* P) {
  const size_t n = P->n, m = P->m;
  const F w = f_root_of_unity(P->lde_log);
  hipLaunchKernelGGL(pow_table_kernel, blocks(m), dim3(256), 0, P->stream, P->d_tw_f, m, w.v);
  hipLaunchKernelGGL(pow_table_kernel, blocks(m), dim3(256), 0, P->stream, P->d_tw_i, m, f_inv(w).v);
  hipLaunchKernelGGL(pow_table_kernel, blocks(m), dim3(256), 0, P->stream, P->d_shift, m, (u64)GL_GEN);
  if (P->d_shift_inv) hipLaunchKernelGGL(pow_table_kernel, blocks(m), dim3(256), 0, P->stream, P->d_shift_inv, m, f_inv(F(GL_GEN)).v);
  if (P->d_shift_odd) hipLaunchKernelGGL(shift_odd_table_kernel, blocks(n), dim3(256), 0, P->stream, P->d_shift_odd, n, P->d_shift, P->d_tw_f, 9u);
  if (P->d_shift_za) lde_za_tables(P);
}

// values [ncols][n] -> coefficients [ncols][n]
static int intt_values(sbn_prover* P, const u64* vals, u64* coef, size_t ncols) {
  for (size_t c0 = 0; c0 < ncols; c0 += P->ntt_chunk) {
    size_t nc = std::min(P->ntt_chunk, ncols - c0);
    int rc = ntt_columns(P, vals + c0 * P->n, P->n, coef + c0 * P->n, P->n, P->d_tmp, P->m, nc, P->degree_bits, true, P->n, nullptr, nullptr,
                         host_inv_pow2(P->degree_bits));
    if (rc) return rc;
  }
  return 0;
}
// coefficients [ncols][n] -> coset LDE [ncols][m]   (lde(rate_bits).coset_fft(7))
static int lde_coeffs(sbn_prover* P, const u64* coef, u64* lde, size_t ncols) {
  for (size_t c0 = 0; c0 < ncols; c0 += P->ntt_chunk) {
    size_t nc = std::min(P->ntt_chunk, ncols - c0);
    int rc = ntt_columns(P, coef + c0 * P->n, P->n, lde + c0 * P->m, P->m, P->d_tmp, P->m, nc, P->lde_log, false, P->n, P->d_shift, nullptr, 1);
    if (rc) return rc;
  }
  return 0;
}
// fused variant used for the big matrices: per chunk iNTT then LDE so the chunk stays cache resident
static int intt_then_lde(sbn_prover* P, const u64* vals, u64* coef, u64* lde, size_t ncols) {
  for (size_t c0 = 0; c0 < ncols; c0 += P->ntt_chunk) {
    size_t nc = std::min(P->ntt_chunk, ncols - c0);
    int rc = ntt_columns(P, vals + c0 * P->n, P->n, coef + c0 * P->n, P->n, P->d_tmp, P->m, nc, P->degree_bits, true, P->n, nullptr, nullptr,
                         host_inv_pow2(P->degree_bits));
    if (rc) return rc;
    rc = ntt_columns(P, coef + c0 * P->n, P->n, lde + c0 * P->m, P->m, P->d_tmp, P->m, nc, P->lde_log, false, P->n, P->d_shift, nullptr, 1);
    if (rc) return rc;
  }
  return 0;
}

// The fused middle pass: inverse pass A -> d_tmp, [inverse pass B + LDE pass A] -> coefficients and `tmp2` on the main stream
// (kernels_ntt.cuh ntt_fused_inv_b_lde_a_kernel at 2^16 / 2^17 rows; ntt_fused512_inv_b_lde_a_kernel at 2^18 rows, where the LDE's
// pass A is the 1,024-point one in two halves); the LDE's pass B follows on `lde_stream` (the main stream, or the second transform
// stream behind `handoff`).  Three launches per chunk instead of four / five.
// `before_write` (compact storage, else null): lde_out is a ring slot, and the stream of the pass that writes it waits for the event first.
static int intt_lde_cols_fused(sbn_prover* P, const u64* v, u64* cf, u64* lde_out, size_t nc, u64* tmp2, hipStream_t lde_stream, hipEvent_t handoff,
                               hipEvent_t before_write = nullptr) {
  int rc = ntt_columns(P, v, P->n, cf, P->n, P->d_tmp, P->m, nc, P->degree_bits, true, P->n, nullptr, nullptr, host_inv_pow2(P->degree_bits), nullptr, 1);
  if (rc) return rc;
  NttFusedParams f{};
  const u32 log_n1 = (P->degree_bits + 1) / 2;
  f.in = P->d_tmp; f.in_col_stride = P->m; f.coef = cf; f.coef_col_stride = P->n; f.out = tmp2; f.out_col_stride = P->m;
  f.n1 = (size_t)1 << log_n1; f.log_n = P->degree_bits; f.tw_i = P->d_tw_i; f.tw_f = P->d_tw_f; f.tw_log = P->lde_log; f.pre = P->d_shift; f.pre2 = P->d_shift_odd;
  f.scale = host_inv_pow2(P->degree_bits);
  if (P->ntt_fused512) hipLaunchKernelGGL(ntt_fused512_inv_b_lde_a_kernel, dim3((unsigned)nc, 32u), dim3(256), 32 * 272 * 8, P->stream, f);
  else hipLaunchKernelGGL(ntt_fused_inv_b_lde_a_kernel, dim3((unsigned)nc, (unsigned)(f.n1 >> 4)), dim3(256), 32 * 272 * 8, P->stream, f);
  if (lde_stream != P->stream) {
    HIPC(hipEventRecord(handoff, P->stream));
    HIPC(hipStreamWaitEvent(lde_stream, handoff, 0));
  }
  if (before_write) HIPC(hipStreamWaitEvent(lde_stream, before_write, 0));
  return ntt_columns(P, cf, P->n, lde_out, P->m, tmp2, P->m, nc, P->lde_log, false, P->n, P->d_shift, nullptr, 1, lde_stream, 2);
}
// values -> coefficients -> coset LDE of nc columns (column strides n, n, m): the unit of the commit pipelines
// coefficients -> coset LDE of nc columns on `st` through `tmp`; before_write as above: waited for between the two passes
static int lde_cols(sbn_prover* P, const u64* cf, u64* lde_out, u64* tmp, size_t nc, hipStream_t st, hipEvent_t before_write) {
  if (!before_write) return ntt_columns(P, cf, P->n, lde_out, P->m, tmp, P->m, nc, P->lde_log, false, P->n, P->d_shift, nullptr, 1, st);
  int rc = ntt_columns(P, cf, P->n, lde_out, P->m, tmp, P->m, nc, P->lde_log, false, P->n, P->d_shift, nullptr, 1, st, 1);
  if (rc) return rc;
  HIPC(hipStreamWaitEvent(st, before_write, 0));
  return ntt_columns(P, cf, P->n, lde_out, P->m, tmp, P->m, nc, P->lde_log, false, P->n, P->d_shift, nullptr, 1, st, 2);
}
static int intt_lde_cols(sbn_prover* P, const u64* v, u64* cf, u64* lde_out, size_t nc, hipEvent_t before_write = nullptr) {
  if ((P->ntt_fused || P->ntt_fused512) && P->d_tmp2) return intt_lde_cols_fused(P, v, cf, lde_out, nc, P->d_tmp2, P->stream, nullptr, before_write);
  int rc = ntt_columns(P, v, P->n, cf, P->n, P->d_tmp, P->m, nc, P->degree_bits, true, P->n, nullptr, nullptr, host_inv_pow2(P->degree_bits));
  if (rc) return rc;
  return lde_cols(P, cf, lde_out, P->d_tmp, nc, P->stream, before_write);
}

static void tree_shape(DevTree& t, size_t nleaf, u32 cap_height) {   // the digests themselves: 2 * nleaf * 4 words at t.d
  t.nleaf = nleaf;
  u32 lg = 0; while (((size_t)1 << lg) < nleaf) lg++;
  t.nlevels = lg - cap_height;
}
static int tree_build_inner(sbn_prover* P, DevTree& t, hipStream_t st) {
  // One permutation costs 27 us on a lane and 8.7 us on 16 lanes, and a single wave saturates its SIMD.  So: levels with
  // >= 2^15 parents run one lane per parent over the whole GPU; narrower levels run 16 lanes per parent, 16 parents per
  // workgroup (one wave per SIMD), one launch per level; the last <= 16 parents finish inside one workgroup.
  // The 2^14-parent level was measured both ways with the broadcast form of the 16-lane permutation: 24.9 us on 16 lanes per
  // parent (four waves per SIMD) against 31.6 us on one lane per parent (profiles/coop16_exchange_ab.txt); with the rotation
  // form it lost there, and the crossover sat one level lower.
  // Round 3: the narrow levels (<= 8192 parents) run FIVE levels per launch -- a workgroup owns 32 consecutive nodes and hashes its
  // own 16 -> 8 -> 4 -> 2 -> 1 parents through LDS (merkle_subtree_kernel, 16 lanes per permutation), so a 2^17-leaf tree takes
  // 3 + 2 launches instead of 3 + 10 and the dependent chain loses eight launch gaps.
  u32 l0 = 0;
  while (l0 < t.nlevels) {
    const size_t parents = t.nleaf >> (l0 + 1);
    if (parents <= 8192 && parents >= 16 && ((t.nleaf >> l0) % 32) == 0) {
      const u32 nlev = std::min<u32>(t.nlevels - l0, 5);
      hipLaunchKernelGGL(merkle_subtree_kernel, dim3((unsigned)((t.nleaf >> l0) / 32)), dim3(MERKLE_SUBTREE_THREADS), 0, st, t.d, t.nleaf, l0, nlev, 32u);
      l0 += nlev;
      continue;
    }
    if (parents >= 32768) {
      hipLaunchKernelGGL(merkle_level_thread_kernel, dim3((unsigned)((parents + 255) / 256)), dim3(256), 0, st, t.d, t.nleaf, l0);
      l0++;
    } else if (parents > 16) {
      hipLaunchKernelGGL(merkle_level_coop_kernel, dim3((unsigned)((parents * 16 + 255) / 256)), dim3(256), 0, st, t.d, t.nleaf, l0);
      l0++;
    } else {
      const size_t nodes = t.nleaf >> l0;
      u32 nchild = (u32)std::min<size_t>(512, nodes);   // children per workgroup
      u32 lg = 0; while ((2u << lg) < nchild) lg++;       // nchild = 2^(lg+1)
      u32 nlev = std::min(t.nlevels - l0, lg + 1);
      hipLaunchKernelGGL(merkle_subtree_kernel, dim3((unsigned)(nodes / nchild)), dim3(MERKLE_SUBTREE_THREADS), 0, st, t.d, t.nleaf, l0, nlev, nchild);
      l0 += nlev;
    }
  }
  HIPC(hipGetLastError());
  return 0;
}
// narrow matrices (quotient chunks): single-launch leaf hash + tree on the main stream
static int tree_from_matrix(sbn_prover* P, DevTree& t, const u64* lde, size_t ncols) {
  hipLaunchKernelGGL(leaf_hash_kernel, dim3((unsigned)((P->m + 255) / 256)), dim3(256), 0, P->stream, lde, P->m, P->lde_log, (u32)ncols, t.d);
  return tree_build_inner(P, t, P->stream);
}

// PolynomialBatch::from_values for a wide matrix: per column chunk iNTT + coset LDE on the main stream,
// sponge absorption of that chunk on the hash stream, then the Merkle levels; main waits at the end.
// up (prove_host_trace only; null: nothing below is enqueued that was not before): `vals` is still on the host.  Chunk k is sent
// on its way right before its transforms are enqueued (trace_load.hip upload_chunk), and the main stream -- which runs the first
// transform pass of a chunk in all three branches below (fused two-stream, plain two-stream, one stream) -- waits for it first.
// dense (compact storage of a wide matrix; null: the LDE stays whole in `lde`): [ncols][qn], the quotient's rows.  The last LDE pass
// of chunk k then writes ring slot k % ring_depth, the sponge reads the slot, lde_keep_rows_kernel behind it copies the slot's
// quotient rows to `dense`, and ring_free[k] is recorded behind that; the stream that runs the writing pass of chunk
// k + ring_depth waits for it in front of that pass -- the one dependency of the transforms on the hash stream.  (The first
// ring_depth chunks of a commitment need no wait: the main stream has waited for hash_done of the commitment before, and the
// second transform stream starts every chunk behind an event of the main stream.)
// [keep0, keep1) (stage_trace_commit; empty: none): columns whose coefficients and LDE an earlier proof left in `coef` and `lde`, the
// same words this one would write.  Nothing transforms them: a chunk is transformed in the pieces that lie outside the range (the
// transforms are per column, and the block is no multiple of the chunk at either end) -- one piece as always when it lies wholly
// outside; its columns below keep0 and those from keep1 on, two pieces at most, when it straddles an end or holds the whole range;
// none when it lies wholly inside.  The sponge launch of every chunk stays what it is and reads the LDE in place, behind
// chunk_ready[k] where this proof records it (behind the last piece) and, for a chunk without a piece, behind the launch of the
// chunk in front on the in-order hash stream alone.  keep0 > 0, so chunk 0 always has a piece and the hash stream enters the
// commitment behind the main stream as before.  *kept (optional): the columns left untransformed.
static int commit_pipeline(sbn_prover* P, const u64* vals, u64* coef, u64* lde, size_t ncols, DevTree& t, int ex_ms, int ex_launches, const HostUpload* up = nullptr,
                           u64* dense = nullptr, size_t keep0 = 0, size_t keep1 = 0, size_t* kept = nullptr) {
  size_t ch = P->ntt_chunk;
  const bool ring = dense != nullptr && ncols > 4;
  if (keep1 > keep0 && (keep0 == 0 || ring || up)) return fail(SBN_ERR_HIP, "internal: resident transforms on a path that keeps none");
  const size_t qn = 2 * P->n;
  if (ring && (!P->d_ring || P->ring_depth == 0)) return fail(SBN_ERR_HIP, "internal: compact commitment without a chunk ring");
  size_t nchunks = (ncols + ch - 1) / ch;
  if (nchunks > (size_t)MAX_CHUNKS) return fail(SBN_ERR_UNSUPPORTED, "too many column chunks");
  if (ncols <= 4) {   // hash_or_noop: a leaf of at most 4 elements is its own digest (MyStark's 4 columns and its 2 Z columns)
    if (up) {   // the whole matrix as one upload
      if (int rc = upload_chunk(P, *up, 0, 0, ncols)) return rc;
    }
    int rc = intt_then_lde(P, vals, coef, lde, ncols);
    if (rc) return rc;
    P->stage_ms[ST_COUNT + ex_launches] = 0;
    return tree_from_matrix(P, t, lde, ncols);
  }
  // Two streams: iNTT + coset LDE of chunk k on the main stream, the sponge over the chunk's LDE on the hash stream.
  // MEASURED and dropped (profiles/r2_bench_3stream.json): a third stream for the LDE, so that the iNTT of chunk k+1 hides
  // behind the LDE of chunk k -- 28.3 -> 29.6 ms per proof: the stage is bound by the VALU work of sponge + transforms
  // together, not by the latency of the transform stream, and more transform waves in flight only slow the sponge launches
  // (12.3 -> 14.8 ms of sponge kernel time).
  size_t nt = 0, two_back[2] = {0, 0};   // pieces transformed so far; the chunks of the last two, [piece number & 1]
  if (kept) *kept = 0;
  for (size_t k = 0; k < nchunks; k++) {
    size_t c0 = k * ch, nc = std::min(ch, ncols - c0);
    int rc;
    const u32 slot = ring ? (u32)(k % P->ring_depth) : 0;
    u64* const lde_k = ring ? P->d_ring + (size_t)slot * ch * P->m : lde + c0 * P->m;
    const hipEvent_t slot_free = (ring && k >= P->ring_depth) ? P->ring_free[k - P->ring_depth] : nullptr;
    // the pieces [a, a + cnt) of this chunk that are transformed: all of it, or what [ka, kb), its share of the resident range, leaves
    struct { size_t a, cnt; } piece[2] = {{c0, nc}, {0, 0}};
    int npieces = 1;
    const size_t ka = std::max(c0, keep0), kb = std::min(c0 + nc, keep1);
    if (ka < kb) {
      npieces = 0;
      if (ka > c0) piece[npieces++] = {c0, ka - c0};
      if (kb < c0 + nc) piece[npieces++] = {kb, c0 + nc - kb};
      if (kept) *kept += kb - ka;
    }
    if (up && (rc = upload_chunk(P, *up, k, c0, nc))) return rc;
    for (int pc = 0; pc < npieces; pc++) {
      const size_t a = piece[pc].a, cnt = piece[pc].cnt;
      const u64* const v_p = vals + a * P->n; u64* const cf_p = coef + a * P->n; u64* const lde_p = lde_k + (a - c0) * P->m;
      if (P->ntt_two_streams && (P->ntt_fused || P->ntt_fused512) && P->d_tmp3) {
        // the fused kernel of piece number nt writes buffer nt & 1, which the LDE pass B of piece nt - 2 (second stream) must have
        // left: chunk_ready of that piece's chunk is recorded behind it.  (Without a resident range: chunk k - 2, buffer k & 1.)
        if (nt >= 2) HIPC(hipStreamWaitEvent(P->stream, P->chunk_ready[two_back[nt & 1]], 0));
        rc = intt_lde_cols_fused(P, v_p, cf_p, lde_p, cnt, (nt & 1) ? P->d_tmp3 : P->d_tmp2, P->nstream, P->intt_done[k], slot_free);
        if (rc) return rc;
        HIPC(hipEventRecord(P->chunk_ready[k], P->nstream));
      } else if (P->ntt_two_streams && !P->ntt_fused && !P->ntt_fused512) {
        rc = ntt_columns(P, v_p, P->n, cf_p, P->n, P->d_tmp, P->m, cnt, P->degree_bits, true, P->n, nullptr, nullptr, host_inv_pow2(P->degree_bits));
        if (rc) return rc;
        HIPC(hipEventRecord(P->intt_done[k], P->stream));
        HIPC(hipStreamWaitEvent(P->nstream, P->intt_done[k], 0));
        rc = lde_cols(P, cf_p, lde_p, P->d_tmp2, cnt, P->nstream, slot_free);
        if (rc) return rc;
        HIPC(hipEventRecord(P->chunk_ready[k], P->nstream));
      } else {
        rc = intt_lde_cols(P, v_p, cf_p, lde_p, cnt, slot_free);
        if (rc) return rc;
        HIPC(hipEventRecord(P->chunk_ready[k], P->stream));
      }
      two_back[nt & 1] = k; nt++;
    }
    if (npieces) HIPC(hipStreamWaitEvent(P->hstream, P->chunk_ready[k], 0));   // (as recorded last: behind the chunk's last piece)
    HIPC(hipEventRecord(P->abs_ev[2 * k], P->hstream));
    hipLaunchKernelGGL(leaf_absorb_kernel, dim3((unsigned)((P->m + 255) / 256)), dim3(256), 0, P->hstream, lde_k, P->m, P->lde_log, (u32)nc,
                       P->d_sponge, k == 0 ? 1 : 0, k + 1 == nchunks ? 1 : 0, t.d,
                       (k + 1 < nchunks && std::min(ch, ncols - (c0 + nc)) >= 8) ? 1 : 0);
    HIPC(hipEventRecord(P->abs_ev[2 * k + 1], P->hstream));
    if (ring) {
      launch_lde_keep_rows(lde_k, P->m, dense + c0 * qn, qn, P->cfg.rate_bits - 1, nc, P->hstream);
      HIPC(hipGetLastError());
      HIPC(hipEventRecord(P->ring_free[k], P->hstream));
    }
  }
  int rc = tree_build_inner(P, t, P->hstream);
  if (rc) return rc;
  HIPC(hipEventRecord(P->hash_done, P->hstream));
  HIPC(hipStreamWaitEvent(P->stream, P->hash_done, 0));
  P->stage_ms[ST_COUNT + ex_launches] = (float)nchunks;
  (void)ex_ms;
  return 0;
}
// Host waits inside prove().  Polling hipStreamQuery / hipEventQuery instead was measured: no gain over the runtime's waits.
// A rank of a split proof (world > 1) waits with a DEADLINE instead: a peer that died leaves this rank's stream behind a
// receive that never completes, and hipStreamSynchronize would hang the whole job; polling returns hipErrorNotReady after
// SBN_COMM_TIMEOUT_S seconds (default 600), prove() fails with SBN_ERR_HIP and the caller can tear the job down.
static thread_local double t_wait_deadline_s = 0;   // 0: plain runtime waits
// (the ranks of a local group are threads that may outnumber the CPUs of the box: spin briefly, then sleep between polls)
static inline void poll_backoff(unsigned spins) {
  if (spins < 2000) std::this_thread::yield();
  else std::this_thread::sleep_for(std::chrono::microseconds(spins < 20000 ? 20 : 200));
}
static inline hipError_t stream_wait(hipStream_t st) {
  if (t_wait_deadline_s <= 0) return hipStreamSynchronize(st);
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  for (;;) {
    const hipError_t e = hipStreamQuery(st);
    if (e != hipErrorNotReady) return e;
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > t_wait_deadline_s) return hipErrorNotReady;
    poll_backoff(++spins);
  }
}
static inline hipError_t event_wait(hipEvent_t ev) {
  if (t_wait_deadline_s <= 0) return hipEventSynchronize(ev);
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > t_wait_deadline_s) return hipErrorNotReady;
    poll_backoff(++spins);
  }
}
// ---- oversized-trace split: exchange helpers ------------------------------------------------------------------------
// Every exchange is STREAM-ORDERED (include/sbn.h sbn_comm.all_to_all): it is enqueued on `st` behind the kernels that
// packed its blocks, and the kernels that consume the received blocks are enqueued on `st` (or behind an event of `st`)
// after it.  Timing: a pair of events around each call, summed after the proof (split_exchange_ms).
static int split_exchange(sbn_prover* P, hipStream_t st, const std::vector<uint64_t>& so, const std::vector<uint64_t>& sl, const std::vector<uint64_t>& ro,
                          const std::vector<uint64_t>& rl) {
  SplitCtx* S = P->sp;
  bool any = false;
  for (u32 r = 0; r < S->comm.world; r++) any = any || sl[r] || rl[r];
  if (!any) return 0;   // (every rank sees the same emptiness: the block counts are functions of the shape alone)
  const bool timed = S->tev_used + 2 <= S->tev.size();
  if (timed) HIPC(hipEventRecord(S->tev[S->tev_used], st));
  const int rc = S->comm.all_to_all(S->comm.ctx, (void*)st, so.data(), sl.data(), ro.data(), rl.data());
  if (rc) return fail(SBN_ERR_HIP, "sbn_comm.all_to_all failed (%d)", rc);
  if (timed) { HIPC(hipEventRecord(S->tev[S->tev_used + 1], st)); S->tev_used += 2; }
  return 0;
}
static int split_all_gather_host(sbn_prover* P, const void* send, void* recv, size_t bytes) {
  SplitCtx* S = P->sp;
  const int rc = S->comm.all_gather_host(S->comm.ctx, send, recv, bytes);
  if (rc) return fail(SBN_ERR_HIP, "sbn_comm.all_gather_host failed (%d)", rc);
  return 0;
}
// every rank contributes `words` u64 at the start of the send buffer; the result [world][words] lands in the receive
// scratch; ordered on the main stream
static int split_all_gather_device(sbn_prover* P, size_t words) {
  SplitCtx* S = P->sp;
  const u32 R = S->comm.world;
  if (words * R > S->scratch_words || words * sizeof(u64) > S->comm.send_bytes) return fail(SBN_ERR_HIP, "internal: split scratch too small");
  const uint64_t base = (uint64_t)((const char*)S->scratch - (const char*)S->comm.recv_buf);
  std::vector<uint64_t> so(R, 0), sl(R, words * sizeof(u64)), ro(R), rl(R, words * sizeof(u64));
  for (u32 r = 0; r < R; r++) ro[r] = base + (uint64_t)r * words * sizeof(u64);
  return split_exchange(P, P->stream, so, sl, ro, rl);
}
// PolynomialBatch::from_values for this rank's share, as a three-stage pipeline over the column blocks (ColShare):
//   main stream   step k: iNTT + coset LDE of the own block k (coefficients stay here), rows packed per destination
//   comm stream   step k: one all-to-all per plane, columns -> rows (the own rows never travel: the pack kernel writes them
//                 straight into the receive matrix)
//   hash stream   step k: the leaf sponge absorbs the blocks k*R .. k*R+R-1 of its LDE rows; then the Merkle subtrees.
// With one rank the LDE lands in the row matrix directly (local row = natural row) and nothing is exchanged.
// `vals`: [..][n] values; block b of the matrix starts at vals + (vals_global ? b : own index k) * ob * n.
static int commit_split(sbn_prover* P, const ColShare& sh, const u64* vals, bool vals_global, u64* coef_own, u64* plane_l, u64* plane_n, DevTree& t) {
  SplitCtx* S = P->sp;
  const u32 R = S->comm.world, me = S->comm.rank;
  const size_t n = P->n, m = P->m, ml = S->ml, ob = sh.ob;
  const size_t steps = sh.steps();
  if (steps > (size_t)MAX_CHUNKS) return fail(SBN_ERR_UNSUPPORTED, "too many column blocks");
  const char* rbase = (const char*)S->comm.recv_buf;
  const char* sbase = (const char*)S->comm.send_buf;
  const u32 row_log = P->lde_log - S->log_r;
  for (size_t k = 0; k < steps; k++) {
    const size_t b = k * R + me, nc = sh.block_cols(b);
    hipStream_t tstream = P->stream;                                        // the stream that completes block k's LDE (and pack)
    u64* const slot = (u64*)S->comm.send_buf + (k & 1) * S->slot_words;     // [plane][dest][ob][ml]
    u64* const slot_n = S->planes == 2 ? slot + (size_t)R * ob * ml : nullptr;
    if (nc) {
      const u64* v = vals + (vals_global ? b : k) * ob * n;
      u64* cf = coef_own + k * ob * n;
      u64* lde_out = R == 1 ? plane_l + b * ob * m : S->d_ldechunk;
      // two transform streams from 2^19 LDE rows up (as in commit_pipeline): the LDE (and the pack) of block k beside the inverse
      // transform of block k + 1
      const bool fused = P->ntt_fused || P->ntt_fused512;
      const bool two = P->ntt_two_streams && P->d_tmp2 && (!fused || P->d_tmp3);
      tstream = two ? P->nstream : P->stream;
      int rc;
      if (two && fused) {   // (as in commit_pipeline: the fused kernel's output buffers alternate)
        if (k >= 2) HIPC(hipStreamWaitEvent(P->stream, P->chunk_ready[k - 2], 0));
        rc = intt_lde_cols_fused(P, v, cf, lde_out, nc, (k & 1) ? P->d_tmp3 : P->d_tmp2, P->nstream, P->intt_done[k]);
      } else if (two) {
        rc = ntt_columns(P, v, n, cf, n, P->d_tmp, m, nc, P->degree_bits, true, n, nullptr, nullptr, host_inv_pow2(P->degree_bits));
        if (rc) return rc;
        HIPC(hipEventRecord(P->intt_done[k], P->stream));
        HIPC(hipStreamWaitEvent(P->nstream, P->intt_done[k], 0));
        rc = ntt_columns(P, cf, n, lde_out, m, P->d_tmp2, m, nc, P->lde_log, false, n, P->d_shift, nullptr, 1, P->nstream);
      } else rc = intt_lde_cols(P, v, cf, lde_out, nc);
      if (rc) return rc;
      if (R > 1 && k >= 2) HIPC(hipStreamWaitEvent(tstream, S->xchg_done[k - 2], 0));   // send slot k & 1 has left
      if (R > 1)
        hipLaunchKernelGGL(split_pack_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)nc), dim3(256), 0, tstream, S->d_ldechunk, m, (u32)nc, (u32)ob, S->log_r, me,
                           slot, slot_n, plane_l + b * ob * ml, plane_n ? plane_n + b * ob * ml : nullptr);
      HIPC(hipGetLastError());
    }
    HIPC(hipEventRecord(P->chunk_ready[k], tstream));
    hipEvent_t arrived = P->chunk_ready[k];
    if (R > 1) {
      HIPC(hipStreamWaitEvent(S->cstream, P->chunk_ready[k], 0));
      for (u32 pl = 0; pl < S->planes; pl++) {
        const u64* dst = pl ? plane_n : plane_l;
        std::vector<uint64_t> so(R, 0), sl(R, 0), ro(R, 0), rl(R, 0);
        for (u32 r = 0; r < R; r++) {
          if (r == me) continue;
          so[r] = (uint64_t)((const char*)(slot + ((size_t)pl * R + r) * ob * ml) - sbase);
          sl[r] = (uint64_t)(nc * ml * sizeof(u64));
          const size_t br = k * R + r;
          ro[r] = (uint64_t)((const char*)(dst + br * ob * ml) - rbase);
          rl[r] = (uint64_t)(sh.block_cols(br) * ml * sizeof(u64));
        }
        int rc = split_exchange(P, S->cstream, so, sl, ro, rl);
        if (rc) return rc;
      }
      HIPC(hipEventRecord(S->xchg_done[k], S->cstream));
      arrived = S->xchg_done[k];
    }
    HIPC(hipStreamWaitEvent(P->hstream, arrived, 0));
    // the sponge over the blocks of this step, in launches of one block (64 columns: the carried state stays small in L2)
    const size_t c_begin = k * R * ob, c_end = std::min(sh.total, (k + 1) * R * ob);
    for (size_t c0 = c_begin; c0 < c_end; c0 += ob) {
      const size_t ncs = std::min(ob, c_end - c0);
      hipLaunchKernelGGL(leaf_absorb_kernel, dim3((unsigned)((ml + 255) / 256)), dim3(256), 0, P->hstream, plane_l + c0 * ml, ml, row_log, (u32)ncs,
                         P->d_sponge, c0 == 0 ? 1 : 0, c0 + ncs == sh.total ? 1 : 0, t.d,
                         (c0 + ncs < sh.total && sh.total - (c0 + ncs) >= 8) ? 1 : 0);
    }
    HIPC(hipGetLastError());
  }
  int rc = tree_build_inner(P, t, P->hstream);
  if (rc) return rc;
  HIPC(hipEventRecord(P->hash_done, P->hstream));
  HIPC(hipStreamWaitEvent(P->stream, P->hash_done, 0));
  return 0;
}
// the Merkle cap: this rank's 2^(cap_height - log R) subtree roots, all-gathered in rank order = cap order
static int split_cap_to_host(sbn_prover* P, const DevTree& t, std::vector<u64>& cap) {
  SplitCtx* S = P->sp;
  const size_t capn = (size_t)1 << P->cfg.cap_height, own = capn >> S->log_r;
  std::vector<u64> mine(own * 4);
  HIPC(hipMemcpyAsync(mine.data(), t.level(t.nlevels), own * 4 * sizeof(u64), hipMemcpyDeviceToHost, P->stream));
  HIPC(stream_wait(P->stream));
  cap.resize(capn * 4);
  return split_all_gather_host(P, mine.data(), cap.data(), own * 4 * sizeof(u64));
}
static int absorb_times(sbn_prover* P, size_t ncols, int ex_ms) {
  size_t nchunks = (ncols + P->ntt_chunk - 1) / P->ntt_chunk;
  float tot = 0;
  for (size_t k = 0; k < nchunks; k++) { float ms = 0; HIPC(hipEventElapsedTime(&ms, P->abs_ev[2 * k], P->abs_ev[2 * k + 1])); tot += ms; }
  P->stage_ms[ST_COUNT + ex_ms] = tot;
  return 0;
}
// upload_result (prove_host_trace): the word the upload's scans folded rides back behind the cap, under the same wait
static int tree_cap_to_host(sbn_prover* P, const DevTree& t, std::vector<u64>& cap, bool upload_result = false) {
  size_t capn = (size_t)1 << P->cfg.cap_height;
  cap.resize(capn * 4);
  HIPC(hipMemcpyAsync(cap.data(), t.level(t.nlevels), capn * 4 * sizeof(u64), hipMemcpyDeviceToHost, P->stream));
  if (upload_result) if (int rc = upload_result_to_host(P)) return rc;
  HIPC(stream_wait(P->stream));
  return 0;
}

// ---- create / destroy -----------------------------------------------------------------------------
// Send side: two slots of one column block per plane, [plane][dest][ob][m/R] = planes * ob * m words each (one rank: no
// slot, the LDE lands in the row matrix), and room for the gathered vectors (2 m/R quotient values, 2 n partial sums).
// Receive side: the row-sharded trace and Z matrices per plane plus the gather scratch.
static constexpr size_t SPLIT_BLOCK = 64;   // columns per ownership block = the prover's NTT chunk (create_ctx checks)
static int split_sizes(const AirShape& as, u32 degree_bits, u32 rate_bits, u32 world, size_t ob, uint64_t* send_bytes, uint64_t* recv_bytes, size_t* scratch_words,
                       size_t* slot_words) {
  const size_t n = (size_t)1 << degree_bits, m = n << rate_bits;
  const u32 planes = world >= 4 ? 2 : 1;
  const size_t sw = std::max<size_t>(2 * m, 2 * n * world);   // gathered quotient values / FRI partial sums
  const size_t slot = world > 1 ? (size_t)planes * ob * m : 0;
  *send_bytes = (uint64_t)(std::max(std::max(2 * slot, 2 * (m / world)), 2 * n) * sizeof(u64));
  *recv_bytes = (uint64_t)(((as.ncols + as.nzs) * (m / world) * planes + sw) * sizeof(u64));
  *scratch_words = sw;
  if (slot_words) *slot_words = slot;
  return 0;
}
// ---- what a context is made of --------------------------------------------------------------------------------------------
// create_ctx runs in three steps so that sbn_prover_memory_plan can follow it without a device: ctx_check_args (the refusals that
// need no device), ctx_shape (every size-bearing field of the context: transform plan, chunk, FRI shape, query stride, storage
// mode) and ctx_buffers, the ONE list of (buffer, bytes) of a context.  create_ctx allocates the list (alloc_buffers: into P->owned,
// which sbn_prover_destroy frees), the plan sums it.
static int ctx_check_args(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, const sbn_comm* comm, const sbn_prover_options* opt, AirShape& as,
                          u32& lde_storage) {
  if (!air || !cfg) return fail(SBN_ERR_BAD_ARG, "null argument");
  lde_storage = SBN_LDE_FULL;
  if (opt) {
    if (opt->struct_size != sizeof(sbn_prover_options)) return fail(SBN_ERR_BAD_ARG, "sbn_prover_options.struct_size does not match this library (ABI %d)", SBN_ABI_VERSION);
    if (opt->lde_storage != SBN_LDE_FULL && opt->lde_storage != SBN_LDE_COMPACT) return fail(SBN_ERR_BAD_ARG, "unknown sbn_prover_options.lde_storage %u", opt->lde_storage);
    lde_storage = opt->lde_storage;
  }
  if (!config_supported(cfg)) return fail(SBN_ERR_UNSUPPORTED, "unsupported StarkConfig (need num_challenges=2, rate_bits 1 or 3, cap_height 1..8, fri_arity_bits 1..4)");
  if (lde_storage == SBN_LDE_COMPACT && cfg->rate_bits == 1)
    return fail(SBN_ERR_UNSUPPORTED, "SBN_LDE_COMPACT needs rate_bits > 1: at rate_bits 1 the quotient's domain is the whole LDE (qn = m), so nothing would be dropped");
  if (comm && cfg->rate_bits != 1) return fail(SBN_ERR_UNSUPPORTED, "the split prover covers rate_bits = 1 only");
  if (!air_shape(air, cfg, as)) return fail(SBN_ERR_BAD_ARG, "unknown air kind / num_io");
  if (!height_supported(cfg, degree_bits)) return fail(SBN_ERR_UNSUPPORTED, "%s", HEIGHT_REFUSAL);
  if (as.kind == SBN_AIR_FLAGS && (512 * (size_t)as.num_io) != ((size_t)1 << degree_bits)) return fail(SBN_ERR_BAD_ARG, "FlagStark needs 512*num_io rows");
  if (as.kind == SBN_AIR_FLAGS_U64 && (128 * (size_t)as.num_io) != ((size_t)1 << degree_bits)) return fail(SBN_ERR_BAD_ARG, "the u64 FlagStark needs 128*num_io rows");
  if (is_exp_air(as.kind)) {
    if ((exp_rows_per_instance(as.kind) * as.num_io) != ((size_t)1 << degree_bits)) return fail(SBN_ERR_BAD_ARG, "the Exp tables need 512*num_io rows (FQ12_EXP_U64: 128*num_io)");
    if (as.kind != SBN_AIR_FQ12_EXP && as.kind != SBN_AIR_FQ12_EXP_U64 && degree_bits < 16)
      return fail(SBN_ERR_UNSUPPORTED, "G1_EXP / G2_EXP / FQ_EXP need >= 2^16 rows (u16 range check, range_check.rs:26)");
  }
  // a wide trace beside a Z matrix of 1..4 columns would need two row strides in the quotient (no table has that shape)
  if (lde_storage == SBN_LDE_COMPACT && as.ncols > 4 && as.nzs >= 1 && as.nzs <= 4) return fail(SBN_ERR_UNSUPPORTED, "SBN_LDE_COMPACT: a wide trace with at most 4 Z columns");
  return 0;
}
static int ctx_shape(sbn_prover* P, const AirShape& as, const sbn_config* cfg, uint32_t degree_bits, u32 lde_storage) {
  P->air = as; P->cfg = *cfg; P->degree_bits = degree_bits; P->lde_log = degree_bits + cfg->rate_bits;
  P->n = (size_t)1 << degree_bits; P->m = (size_t)1 << P->lde_log;
  P->fri = fri_shape(*cfg, degree_bits);
  if (P->fri.total_arity() > degree_bits + cfg->rate_bits - cfg->cap_height) return fail(SBN_ERR_UNSUPPORTED, "FRI total reduction arity is too large");
  // Column chunk of the commit pipeline: a multiple of 8 (the sponge permutes after every 8 absorbed columns, so any other
  // chunk boundary would change the leaf digests), between 8 and 256.
  // Default 64; 48 from 2^19 LDE rows up: a chunk's LDE (chunk * M * 8 bytes) is written by the transform stream and read by the
  // sponge out of the 256 MiB Infinity Cache, and 64 columns of 2^19 rows are 268 MB (Fq12ExpStark(512): 0.708 -> 0.675 s,
  // profiles/r3_v2_fq12_chunk.txt).
  // 2^18 LDE rows: 64 columns are 134 MB and the sponge launches themselves run 17 % slower (35.7 against 30.4 ms per trace commitment of
  // G1ExpStark(256)); 48 columns: prove() 61.1 -> 56.1 ms (profiles/r4_chunk_2pow17.txt).
  P->ntt_chunk = P->lde_log >= 18 ? 48 : 64;
  {
    std::string serr;
    if (!P->set.load(serr)) return fail(SBN_ERR_BAD_ARG, "%s", serr.c_str());
  }
  const Settings& set = P->set;
  if (set.ntt_chunk) P->ntt_chunk = (size_t)set.ntt_chunk;
  ntt_plan(P);
  // with the fused middle pass the chunk also crosses the transform's second buffer: 40 columns (0.605 -> 0.589 s, profiles/r4_fused512.txt)
  if (P->ntt_fused512 && !set.ntt_chunk) P->ntt_chunk = 40;
  // curve chains of the device witness: the host pool when the CPU has AVX-512 IFMA (eight instances per register: 128 instances
  // are 16 tasks of ~0.15 ms, chains_ifma.hpp) or the pool has the threads for the scalar form (2.2 ms on 16), else one wave per
  // instance on the device (5.2 ms whatever the host share: an 8-rank node may leave a rank two CPUs, where the scalar host chains
  // take ~18 ms)
  P->chain_mode = set.device_chain >= 0 ? set.device_chain : ((tracegen_host_chains_vectorized() || tracegen_host_threads() >= 8) ? 0 : 2);
  // From 2^19 LDE rows up the transform stream, not the sum of the instruction streams, bounds the commitments (profiles/
  // r3_v8_fq12_512_kernel_stats.csv: five passes of 410 us per chunk beside a 1.19 ms sponge launch, 1.63 ms of VALU work in a 2.05 ms
  // period): the LDE passes of chunk k then run on a second stream beside the inverse passes of chunk k+1 (two streams at 2^16 rows,
  // where the stage IS at its VALU bound, were measured slower in round 2).
  P->ntt_two_streams = P->lde_log >= 19;
  // compact storage takes effect on the wide tables: a matrix of at most 4 columns (hash_or_noop) stays whole in both modes
  P->lde_storage = lde_storage;
  P->compact = lde_storage == SBN_LDE_COMPACT && as.ncols > 4;
  P->ring_depth = P->compact ? LDE_RING_DEPTH : 0;
  // the shape-constant columns whose transforms stay resident between proofs (stage_trace_commit): whole LDEs on one GPU only -- under
  // compact storage a chunk's LDE lives in the ring, and create_ctx empties the range of a split context
  if (set.fixed_columns && !P->compact) fixed_columns_range(as, P->fixed_f0, P->fixed_f1);
  P->apow_n = apow_len(as.nconstraints, as.nzs);
  // query section stride (words per query round)
  {
    const size_t C = as.ncols, Z = as.nzs;
    size_t sib = (size_t)(P->lde_log - cfg->cap_height) * 4;
    size_t s = C + sib + (Z ? Z + sib : 0) + 4 + sib;
    u32 bits = P->lde_log;
    for (u32 ab : P->fri.arity_bits) { bits -= ab; s += 2 * ((size_t)1 << ab) + (size_t)(bits - cfg->cap_height) * 4; }
    P->qstride = s;
  }
  return 0;
}
// Not a pure function of P: it also completes the shape it lists -- lde_scratch_words, the leaf and level counts of the trees, the
// lengths of fri_vals / fri_trees (whose elements the list points into) -- so it is called exactly once per context, by create_ctx
// or by the plan.
// Every device buffer a context holds from creation on, in allocation order.  Not in the list (allocated by the first call that
// needs them, include/sbn.h sbn_prover_memory_plan): d_first_bad of prove_host_trace (8 bytes; its upload ring is pinned host memory).
static void ctx_buffers(sbn_prover* P, std::vector<BufReq>& L) {
  const AirShape& as = P->air; const sbn_config* cfg = &P->cfg;
  // qn: the quotient's domain, the coset of 2n points (quotient_degree_bits = 1) whatever the rate: LDE rows k * m / qn
  const size_t n = P->n, m = P->m, qn = 2 * n, C = as.ncols, Z = as.nzs;
  auto words = [&](u64** p, size_t w) { L.push_back(words_req(p, w)); };
  auto bytes = [&](void** p, size_t b) { L.push_back(BufReq{p, b}); };
  auto tree = [&](DevTree& t, size_t nleaf, u32 cap_height) { tree_shape(t, nleaf, cap_height); words(&t.d, 2 * nleaf * 4); };
  if (SplitCtx* S = P->sp) {
    const u32 lr = S->log_r;
    words(&P->d_trace, C * n); words(&P->d_coef, std::max<size_t>(S->cr, 1) * n);
    words(&P->d_zval, std::max<size_t>(S->zr, 1) * n); words(&P->d_zcoef, std::max<size_t>(S->zr, 1) * n);
    words(&S->d_ldechunk, P->ntt_chunk * m);
    bytes((void**)&S->d_idx_local, cfg->num_query_rounds * sizeof(u32));
    tree(P->tree_t, S->ml, cfg->cap_height - lr); tree(P->tree_z, S->ml, cfg->cap_height - lr);
  } else {
    // compact: the wide matrices keep the quotient's rows only (P->compact: C > 4, and Z = 0 or Z > 4), and the LDE of a chunk
    // passes through the ring
    const size_t rows = P->compact ? qn : m;
    P->lde_scratch_words = C * rows;
    words(&P->d_trace, C * n); words(&P->d_coef, C * n); words(&P->d_lde, C * rows);
    words(&P->d_zval, std::max<size_t>(Z, 1) * n); words(&P->d_zcoef, std::max<size_t>(Z, 1) * n); words(&P->d_zlde, Z > 4 ? Z * rows : std::max<size_t>(Z, 1) * m);
    if (P->compact) words(&P->d_ring, (size_t)P->ring_depth * P->ntt_chunk * m);
    tree(P->tree_t, m, cfg->cap_height); tree(P->tree_z, m, cfg->cap_height);
  }
  words(&P->d_tmp, std::max(P->ntt_chunk, (size_t)4) * m);
  if (P->ntt_fused || P->ntt_fused512 || P->ntt_two_streams) words(&P->d_tmp2, std::max(P->ntt_chunk, (size_t)4) * m);
  if ((P->ntt_fused || P->ntt_fused512) && P->ntt_two_streams) words(&P->d_tmp3, std::max(P->ntt_chunk, (size_t)4) * m);
  words(&P->d_q, 2 * qn); words(&P->d_qlde, 4 * m);
  tree(P->tree_q, m, cfg->cap_height);
  words(&P->d_tw_f, m); words(&P->d_tw_i, m); words(&P->d_shift, m); words(&P->d_shift_inv, m);
  if (P->ntt_fused512) words(&P->d_shift_odd, n);   // (ntt_plan)
  if (P->lde_za_log) words(&P->d_shift_za, n << P->lde_za_log);   // (ntt_plan)
  words(&P->d_xs, qn); words(&P->d_lag_first, qn); words(&P->d_lag_last, qn);   // per quotient point
  words(&P->d_apow, (size_t)SBN_NCH * P->apow_n);
  words(&P->d_zpow, 4 * n); words(&P->d_open, (C + Z + 4) * 4);
  words(&P->d_part, 2 * 32 * n); words(&P->d_w, 4096); words(&P->d_sponge, 12 * m);
  words(&P->d_fa, 4 * n); words(&P->d_fcoef, 2 * m); words(&P->d_fcoef2, 2 * m);
  words(&P->d_pow, 1);
  bytes(&P->d_pic, sizeof(ExpPiConsts<F>));
  bytes((void**)&P->d_idx, cfg->num_query_rounds * sizeof(u32));
  // FRI layer buffers
  {
    const size_t layers = P->fri.arity_bits.size();
    P->fri_vals.assign(layers, nullptr); P->fri_trees.assign(layers, DevTree());
    u32 bits = P->lde_log;
    for (size_t li = 0; li < layers; li++) {
      const u32 ab = P->fri.arity_bits[li];
      words(&P->fri_vals[li], 2 * ((size_t)1 << bits));
      tree(P->fri_trees[li], (size_t)1 << (bits - ab), cfg->cap_height);
      bits -= ab;
    }
  }
  words(&P->d_qbuf, P->qstride * cfg->num_query_rounds);
  bytes((void**)&P->d_pairs, std::max<size_t>(Z, 1) * sizeof(PairCols));
  if (P->sp && P->sp->zr) bytes((void**)&P->sp->d_pairs_own, P->sp->zr * sizeof(PairCols));
}
extern "C" int sbn_prover_memory_plan(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, const sbn_prover_options* opt, uint64_t* bytes_out) {
  if (!bytes_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  *bytes_out = 0;
  AirShape as; u32 storage = 0;
  if (int rc = ctx_check_args(air, cfg, degree_bits, nullptr, opt, as, storage)) return rc;
  const std::unique_ptr<sbn_prover> P(new sbn_prover());   // shape fields only: nothing of it touches a device
  if (int rc = ctx_shape(P.get(), as, cfg, degree_bits, storage)) return rc;
  std::vector<BufReq> L;
  ctx_buffers(P.get(), L);
  for (const BufReq& b : L) *bytes_out += b.bytes;
  return SBN_OK;
}

static int create_ctx(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, const sbn_comm* comm, const sbn_prover_options* opt, sbn_prover** out);
extern "C" int sbn_prover_create_with(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, const sbn_prover_options* opt, sbn_prover** out) {
  return create_ctx(air, cfg, degree_bits, nullptr, opt, out);
}
extern "C" int sbn_prover_create(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, sbn_prover** out) {
  return sbn_prover_create_with(air, cfg, degree_bits, nullptr, out);
}
static int create_ctx(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, const sbn_comm* comm, const sbn_prover_options* opt, sbn_prover** out) {
  if (!air || !cfg || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  *out = nullptr;
  AirShape as; u32 storage = 0;
  if (int rc = ctx_check_args(air, cfg, degree_bits, comm, opt, as, storage)) return rc;
  if (int rc = use_current_device("the prover path has no CPU fallback")) return rc;
  sbn_prover* P = new sbn_prover();
  P->device = g_device;
  // every failure below releases what was created so far (sbn_prover_destroy accepts a partly built context) and
  // returns the FIRST error code
  int rc = 0;
  auto acc = [&](int r) { if (!rc) rc = r; };
  auto hipc = [&](hipError_t e, const char* what) { if (e != hipSuccess && !rc) rc = fail(SBN_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e)); };
  if ((rc = ctx_shape(P, as, cfg, degree_bits, storage))) { sbn_prover_destroy(P); return rc; }
  const Settings& set = P->set;
  acc(ntt_fast_setup());
  hipc(hipStreamCreate(&P->stream), "hipStreamCreate");
  hipc(hipStreamCreate(&P->hstream), "hipStreamCreate");
  if (P->ntt_two_streams) {   // (ctx_shape)
    hipc(hipStreamCreate(&P->nstream), "hipStreamCreate");
    for (auto& e : P->intt_done) hipc(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
  }
  for (auto& e : P->ev) hipc(hipEventCreate(&e), "hipEventCreate");
  for (auto& e : P->abs_ev) hipc(hipEventCreate(&e), "hipEventCreate");
  for (auto& e : P->chunk_ready) hipc(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
  hipc(hipEventCreateWithFlags(&P->hash_done, hipEventDisableTiming), "hipEventCreate");
  if (P->compact) for (auto& e : P->ring_free) hipc(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
  for (auto& v : P->stage_ms) v = 0;
  if (rc) { sbn_prover_destroy(P); return rc; }
  const size_t n = P->n, m = P->m, qn = 2 * n, C = as.ncols, Z = as.nzs;
  if (comm && (C <= 4 || Z == 0)) { sbn_prover_destroy(P); return fail(SBN_ERR_UNSUPPORTED, "the split prover covers the wide tables (this one has %zu columns and %zu permutation Zs)", C, Z); }
  if (comm) {
    // one trace over comm->world GPUs: this rank keeps the coefficients of its own columns and the LDE ROWS of its Merkle
    // subtrees (views of the caller's receive buffer); the trace values stay whole
    const u32 R = comm->world;
    u32 lr = 0; while ((1u << lr) < R) lr++;
    uint64_t sb = 0, rb = 0; size_t sw = 0, slotw = 0;
    if (comm->struct_size != sizeof(sbn_comm)) { sbn_prover_destroy(P); return fail(SBN_ERR_BAD_ARG, "sbn_comm.struct_size does not match this library (ABI %d)", SBN_ABI_VERSION); }
    if (!set.ntt_chunk) P->ntt_chunk = SPLIT_BLOCK;   // (the size-dependent default above is the single-GPU pipeline's: a rank's rows are M / world)
    if (P->ntt_chunk != SPLIT_BLOCK) { sbn_prover_destroy(P); return fail(SBN_ERR_UNSUPPORTED, "the split prover deals columns in blocks of %zu: unset SBN_NTT_CHUNK", SPLIT_BLOCK); }
    split_sizes(as, degree_bits, cfg->rate_bits, R, SPLIT_BLOCK, &sb, &rb, &sw, &slotw);
    if ((1u << lr) != R || lr > cfg->cap_height || comm->rank >= R || !comm->all_to_all || !comm->all_gather_host || !comm->send_buf || !comm->recv_buf ||
        comm->send_bytes < sb || comm->recv_bytes < rb) {
      sbn_prover_destroy(P);
      return fail(SBN_ERR_BAD_ARG, "bad sbn_comm (world must be a power of two <= 2^cap_height; staging buffers of sbn_split_exchange_bytes)");
    }
    for (const void* buf : {(const void*)comm->send_buf, (const void*)comm->recv_buf}) {   // (a transport created on another GPU: ADVICE r3)
      hipPointerAttribute_t pa{};
      if (hipPointerGetAttributes(&pa, buf) != hipSuccess || pa.device != P->device) {
        (void)hipGetLastError();
        sbn_prover_destroy(P);
        return fail(SBN_ERR_BAD_ARG, "sbn_comm staging buffers do not live on this prover's device %d (call sbn_set_device before creating the transport)", g_device);
      }
    }
    SplitCtx* S = P->sp = new SplitCtx();
    P->fixed_f0 = P->fixed_f1 = 0;   // a rank keeps the LDE rows of its subtrees, not columns: every proof transforms every column
    for (auto& e : S->xchg_done) e = nullptr;
    S->comm = *comm; S->log_r = lr; S->rho = bitrev32(comm->rank, lr); S->ml = m >> lr; S->planes = R >= 4 ? 2 : 1;
    S->slot_words = slotw;
    S->cs.total = C; S->cs.ob = SPLIT_BLOCK; S->cs.R = R; S->cs.rank = comm->rank;
    S->zs = S->cs; S->zs.total = Z;
    S->cr = S->cs.own(); S->zr = S->zs.own();
    hipc(hipStreamCreate(&S->cstream), "hipStreamCreate");
    for (auto& e : S->xchg_done) hipc(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    S->tev.assign(2 * (2 * (S->cs.steps() + S->zs.steps()) + 8), nullptr);
    for (auto& e : S->tev) hipc(hipEventCreate(&e), "hipEventCreate");
    u64* rbuf = (u64*)comm->recv_buf;
    S->lde_l = rbuf; rbuf += C * S->ml;
    if (S->planes == 2) { S->lde_n = rbuf; rbuf += C * S->ml; }
    S->zlde_l = rbuf; rbuf += Z * S->ml;
    if (S->planes == 2) { S->zlde_n = rbuf; rbuf += Z * S->ml; }
    S->scratch = rbuf; S->scratch_words = sw;
    P->lde_scratch_words = (size_t)(rb / sizeof(u64));   // witness generation runs before the first exchange
  }
  {
    std::vector<BufReq> L;
    ctx_buffers(P, L);
    if ((rc = alloc_buffers(P, L))) { sbn_prover_destroy(P); return rc; }
  }
  P->d_fb = P->d_fa + 2 * n;
  hipc(hipHostMalloc((void**)&P->h_open, (C + Z + 4) * 4 * sizeof(u64), hipHostMallocDefault), "hipHostMalloc");
  hipc(hipHostMalloc((void**)&P->h_open2, (C + Z) * 4 * sizeof(u64), hipHostMallocDefault), "hipHostMalloc");
  hipc(hipHostMalloc((void**)&P->h_w, 4096 * sizeof(u64), hipHostMallocDefault), "hipHostMalloc");
  if (rc) { sbn_prover_destroy(P); return rc; }
  // tables
  fill_transform_tables(P);
  hipLaunchKernelGGL(domain_tables_kernel, blocks(qn), dim3(256), 0, P->stream, P->d_xs, P->d_lag_first, P->d_lag_last, qn, degree_bits + 1, degree_bits);
  // permutation pairs
  {
    std::vector<PairCols> pairs(Z);
    for (size_t z = 0; z < Z; z++) {
      int l, r;
      air_pair(as, z, l, r);
      pairs[z].lhs = l; pairs[z].rhs = r;
    }
    if (!rc && Z) hipc(hipMemcpy(P->d_pairs, pairs.data(), Z * sizeof(PairCols), hipMemcpyHostToDevice), "hipMemcpy");
    if (P->sp && P->sp->zr) {   // the split: the pairs of this rank's Z columns in local order
      SplitCtx* S = P->sp;
      std::vector<PairCols> own(S->zr);
      for (size_t l = 0; l < S->zr; l++) own[l] = pairs[S->zs.global_col(S->zs.rank, l)];
      if (!rc) hipc(hipMemcpy(S->d_pairs_own, own.data(), S->zr * sizeof(PairCols), hipMemcpyHostToDevice), "hipMemcpy");
    }
  }
  hipc(hipStreamSynchronize(P->stream), "hipStreamSynchronize");
  hipc(hipGetLastError(), "table kernels");
  if (rc) { sbn_prover_destroy(P); return rc; }
  *out = P;
  return SBN_OK;
}

namespace sbn { size_t prover_device_bytes(const sbn_prover* P) { return P ? P->dev_bytes + guard_device_bytes(P) : 0; } }   // capi.hip: the one-shot cache (the guard's verifier counts)
extern "C" void sbn_prover_destroy(sbn_prover* P) {
  if (!P) return;
  (void)hipSetDevice(P->device);
  guard_destroy(P);   // guard.hip: the device verifier of a guarded context, if one was created
  if (P->ustream) (void)hipStreamSynchronize(P->ustream);   // in front of the frees: the copy stream writes d_trace and its scan word (a refused call drained it already)
  for (void* b : P->owned) (void)hipFree(b);                 // every device buffer of the context (alloc_buffers)
  if (P->sp) {
    for (auto& e : P->sp->xchg_done) if (e) (void)hipEventDestroy(e);
    for (auto& e : P->sp->tev) if (e) (void)hipEventDestroy(e);
    if (P->sp->cstream) (void)hipStreamDestroy(P->sp->cstream);
    delete P->sp;
  }
  for (auto& e : P->ev) if (e) (void)hipEventDestroy(e);   // a partly built context (failed create) holds null handles
  for (auto& e : P->abs_ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : P->chunk_ready) if (e) (void)hipEventDestroy(e);
  if (P->hash_done) (void)hipEventDestroy(P->hash_done);
  for (auto& e : P->ring_free) if (e) (void)hipEventDestroy(e);
  for (void* h : {(void*)P->h_chain, (void*)P->h_io, (void*)P->h_open, (void*)P->h_open2, (void*)P->h_w}) if (h) (void)hipHostFree(h);   // pinned
  upload_destroy(P);   // trace_load.hip: the pinned ring, the upload events, the copy stream
  if (P->hstream) (void)hipStreamDestroy(P->hstream);
  if (P->nstream) { (void)hipStreamDestroy(P->nstream); for (auto& e : P->intt_done) if (e) (void)hipEventDestroy(e); }
  if (P->stream) (void)hipStreamDestroy(P->stream);
  delete P;
}

extern "C" int sbn_prover_stage_times(const sbn_prover* P, float* ms, int cap) {
  return P ? copy_times(P->stage_ms, ST_COUNT + EX_COUNT, ms, cap) : 0;
}
extern "C" const char* sbn_prover_stage_name(int i) { return (i >= 0 && i < ST_COUNT + EX_COUNT) ? STAGE_NAMES[i] : ""; }

// ---- prove ----------------------------------------------------------------------------------------
// quotient_kernel<KIND, PART>: PART 0 then 1 on the main stream, PART 2 (both permutation-check segments) on the second
template <int KIND>
static void launch_quotient_kind(sbn_prover* P, const QuotientParams& qp, size_t qblocks) {
  const dim3 g1((unsigned)qblocks, 1), g2((unsigned)qblocks, 2);
  if (qp.seg_mask & 12u) hipLaunchKernelGGL((quotient_kernel<KIND, 2>), g2, dim3(256), 0, P->hstream, qp, qp.apow[0], qp.apow[1], qp.pic);
  if (qp.seg_mask & 1u) hipLaunchKernelGGL((quotient_kernel<KIND, 0>), g1, dim3(256), 0, P->stream, qp, qp.apow[0], qp.apow[1], qp.pic);
  if (qp.seg_mask & 2u) hipLaunchKernelGGL((quotient_kernel<KIND, 1>), g1, dim3(256), 0, P->stream, qp, qp.apow[0], qp.apow[1], qp.pic);
}
int launch_quotient_parts(sbn_prover* P, const QuotientParams& qp, size_t qblocks) {
  for_air_kind(P->air.kind, [&](auto K) { launch_quotient_kind<decltype(K)::value>(P, qp, qblocks); });
  HIPC(hipGetLastError());
  return 0;
}

// The Z columns of `pairs` (starky permutation.rs compute_permutation_z_poly) from the trace values; also the trace check's (trace_check.hip).
void launch_perm_z(sbn_prover* P, const PairCols* pp, size_t cnt, u64 gamma0, u64 gamma1, u64* out, hipStream_t s) {
  if (cnt == 0) return;
  const size_t n = P->n;
  // from 2^13 rows up: chunk products, one wave per column for their prefix / suffix, then Z written once -- 5 words per row
  // instead of 7 (kernels.cuh permz_chunk_*; the chunk products wait in the idle quotient scratch).  Other shapes: the
  // one-workgroup-per-column kernel of rounds 1-3.
  const size_t chunks = n / 2048;
  if (n >= 8192 && n % 2048 == 0 && cnt <= 65535 && cnt * chunks * 4 <= 2 * 32 * n) {
    u64* tot = P->d_part; u64* pq = P->d_part + cnt * chunks * 2;
    hipLaunchKernelGGL(permz_chunk_products_kernel<8>, dim3((unsigned)chunks, (unsigned)cnt), dim3(256), 0, s, P->d_trace, n, pp, gamma0, gamma1, tot);
    hipLaunchKernelGGL(permz_chunk_scan_kernel, dim3((unsigned)cnt), dim3(64), 0, s, tot, (u32)chunks, pq);
    hipLaunchKernelGGL(permz_chunk_write_kernel<8>, dim3((unsigned)chunks, (unsigned)cnt), dim3(256), 0, s, P->d_trace, n, pp, gamma0, gamma1, pq, out);
    return;
  }
  if (n % 2048 == 0) hipLaunchKernelGGL(permutation_z_kernel<8>, dim3((unsigned)cnt), dim3(256), 0, s, P->d_trace, n, pp, gamma0, gamma1, out);
  else if (n % 1024 == 0) hipLaunchKernelGGL(permutation_z_kernel<4>, dim3((unsigned)cnt), dim3(256), 0, s, P->d_trace, n, pp, gamma0, gamma1, out);
  else hipLaunchKernelGGL(permutation_z_kernel<2>, dim3((unsigned)cnt), dim3(256), 0, s, P->d_trace, n, pp, gamma0, gamma1, out);   // n = 512
}

// The alpha-power table and the public-input constants of the constraint kernels, for the quotient stage and the trace check alike.
int upload_alpha_tables(sbn_prover* P, const F alphas[SBN_NCH]) {
  hipStream_t st = P->stream;
  const size_t APN = P->apow_n;
  std::vector<u64> apow((size_t)SBN_NCH * APN);
  std::vector<F> ap[SBN_NCH];
  for (int j = 0; j < SBN_NCH; j++) {
    ap[j].resize(APN);
    F a(1);
    for (size_t k = 0; k < APN; k++) { ap[j][k] = a; apow[(size_t)j * APN + k] = a.v; a = a * alphas[j]; }
  }
  HIPC(hipMemcpyAsync(P->d_apow, apow.data(), apow.size() * sizeof(u64), hipMemcpyHostToDevice, st));
  if (is_exp_air(P->air.kind)) {
    static thread_local ExpPiConsts<F> pic;  // 3 x 2 x G1EXP_MAX_IO field elements
    const F* app[SBN_NCH] = {ap[0].data(), ap[1].data()};
    std::vector<F> pif(P->pi.size());
    for (size_t i = 0; i < pif.size(); i++) pif[i] = F(P->pi[i]);
    exp_pi_consts<F>(exp_shape(P->air), app, pif.data(), pic);
    HIPC(hipMemcpyAsync(P->d_pic, &pic, sizeof(pic), hipMemcpyHostToDevice, st));
  }
  HIPC(stream_wait(st));
  return 0;
}
void quotient_segments(const sbn_prover* P, const F alphas[SBN_NCH], QuotientParams& qp) {
  const size_t Z = P->air.nzs;
  for (int j = 0; j < SBN_NCH; j++) { qp.alpha[j] = alphas[j].v; qp.apow[j] = P->d_apow + (size_t)j * P->apow_n; }
  qp.num_zs = (int)Z; qp.num_io = (int)P->air.num_io; qp.pic = P->d_pic;
  // constraints that follow each segment: [AIR head][AIR tail], then the permutation block, whose two segments take the Z
  // columns below / from zsplit with exponents counted from the end of the stream (nothing follows either of them).
  // (Measured and dropped: the AIR tail on a third stream beside the other two -- 1.22 -> 1.32 ms for the stage, G2 2.0 -> 2.3.)
  qp.zsplit = (int)(Z / 2);
  qp.lookups_in_perm = P->set.quotient_lookups == 1;   // measured slower (quotient stage 1.18 -> 1.25 ms for G1): an experiment switch only
  const u64 n_tail = is_exp_air(P->air.kind) ? (u64)exp_shape(P->air).num_tail_constraints() : 0;
  const u64 after[4] = {n_tail + 2 * (u64)Z, 2 * (u64)Z, 0, 0};
  qp.seg_count[0] = (int)(P->air.nconstraints - n_tail); qp.seg_count[1] = (int)n_tail;
  qp.seg_count[2] = qp.seg_count[3] = 2 * (int)Z;
  for (int sgm = 0; sgm < 4; sgm++) for (int j = 0; j < SBN_NCH; j++) qp.seg_shift[sgm][j] = f_pow(alphas[j], after[sgm]).v;
  qp.seg_mask = 0xfu;
}

// ---- prove: one ProofRun, one function per Stage -----------------------------------------------------
// The state of one prove() call that crosses a stage boundary, and nothing else: per member, the stage that writes it; the stages
// that read it.  The stage functions stand in the order of enum Stage (prover_ctx.hpp), the order of the transcript.  Stage X spans
// [ev[X], ev[X + 1]) on the main stream and records ev[X + 1] itself (next_stage): behind what it enqueued and IN FRONT of its host
// wait (cap download, opening slices, stream_wait), so that round trip is not in the time it reports.  (fri_layers and pow wait
// inside their loops: their event follows the last wait.)
struct ProofRun {
  sbn_prover* P = nullptr;                    // prove_streamed; read by every stage
  SplitCtx* S = nullptr;                      // prove_streamed: P->sp, non-null: this rank's share of one trace split over S->comm.world GPUs; every stage
  const HostUpload* up = nullptr;             // prove_streamed: null for sbn_prover_prove (the trace is resident), else the host trace streamed in; trace_commit
  Challenger ch;                              // the transcript: every stage observes into it and draws from it, in stage order
  bool fills_fixed = false;                   // trace_commit: it transforms the generators' words of the shape-constant columns; prove_streamed, behind the proof
  std::vector<u64> trace_cap, z_cap, q_cap;   // trace_commit, z_commit (Z > 0 only), quotient_commit; assemble_proof
  F gamma0, gamma1;                           // perm_z; quotient_eval
  F alphas[SBN_NCH];                          // quotient_eval draws them, for its own tables and kernels
  E2 zeta, zeta_next;                         // openings; fri_combine
  E2 fri_alpha;                               // fri_combine draws it, for its weights and its divisions
  const u64 *open = nullptr, *open2 = nullptr;   // openings: the values at zeta / at g * zeta (pinned, [(C + Z + 4)][4]); assemble_proof
  std::vector<std::vector<u64>> fri_caps; std::vector<u64> final_poly;   // fri_layers; assemble_proof
  u64 pow_witness = ~0ULL;                    // pow; assemble_proof
  std::vector<u32> idx, idx_local;            // queries: the leaf indices, pageable sources of async uploads that live until its wait
  std::vector<u64> qwords;                    // queries; assemble_proof
  size_t split_section = 0;                   // queries (the split): words per query that come from the row-sharded trees

  size_t capw() const { return ((size_t)1 << P->cfg.cap_height) * 4; }   // words of a Merkle cap
  // the cap of a commitment to the host -- a host wait -- and into the transcript (sharded: a row-sharded tree of the split)
  int observe_cap(const DevTree& t, std::vector<u64>& cap, bool sharded, bool upload_result = false) {
    if (int rc = sharded ? split_cap_to_host(P, t, cap) : tree_cap_to_host(P, t, cap, upload_result)) return rc;
    ch.observe_words(cap.data(), capw());
    return 0;
  }
  // closes the interval of the stage in front of `next` (and opens that of `next`) on the main stream
  int next_stage(int next) { HIPC(hipEventRecord(P->ev[next], P->stream)); return 0; }
};

// P1 trace commitment ---------------------------------------------------------------------------
static int stage_trace_commit(ProofRun& run) {
  sbn_prover* P = run.P; SplitCtx* S = run.S; const HostUpload* up = run.up;
  if (up) if (int rc = upload_begin(P, *up)) return rc;   // in front of the first scan
  // The shape-constant columns (prover_ctx.hpp fixed_match / fixed_valid; the range is empty for the split, compact storage and the
  // tables without one).  The resident trace holds the generators' words there and an earlier proof of them succeeded: their
  // coefficients and LDE are in place, nothing transforms them.  It holds them and no such proof yet: everything is transformed, and
  // prove_streamed sets fixed_valid behind the proof.  Anything else -- other words, a trace that is still on the host -- is transformed
  // whole, and d_coef / d_lde then hold the transforms of other words.
  const bool canonical = !up && P->fixed_match && P->fixed_f1 > P->fixed_f0;
  if (!canonical) P->fixed_valid = false;
  run.fills_fixed = canonical && !P->fixed_valid;
  const size_t keep0 = canonical && P->fixed_valid ? P->fixed_f0 : 0, keep1 = canonical && P->fixed_valid ? P->fixed_f1 : 0;
  P->fixed_skipped = 0;
  if (S) {
    S->tev_used = 0;
    if (int rc = commit_split(P, S->cs, P->d_trace, true, P->d_coef, S->lde_l, S->lde_n, P->tree_t)) return rc;
  } else if (int rc = commit_pipeline(P, P->d_trace, P->d_coef, P->d_lde, P->air.ncols, P->tree_t, EX_TRACE_ABSORB_MS, EX_TRACE_ABSORB_LAUNCHES, up, P->compact ? P->d_lde : nullptr,
                                      keep0, keep1, &P->fixed_skipped)) return rc;
  if (int rc = run.next_stage(ST_PERM_Z)) return rc;
  if (int rc = run.observe_cap(P->tree_t, run.trace_cap, S != nullptr, up != nullptr)) return rc;   // (the scans' word rides back behind the cap)
  return up ? upload_verdict(P, *up) : 0;
}

// P2 permutation argument -------------------------------------------------------------------------
// get_n_permutation_challenge_sets(num_challenges, batch_size=2): sets[s].challenges[c] = (beta, gamma)
// (a table without permutation pairs -- FlagStark -- draws no permutation challenges and commits no Z: starky prover.rs
//  `stark.uses_permutation_args()`)
static int stage_perm_z(ProofRun& run) {
  sbn_prover* P = run.P; SplitCtx* S = run.S;
  const size_t Z = P->air.nzs;
  F gam[2][2] = {};
  if (Z) for (int s = 0; s < 2; s++) for (int c = 0; c < (int)P->cfg.num_challenges; c++) { (void)run.ch.challenge(); gam[s][c] = run.ch.challenge(); }
  run.gamma0 = gam[0][0]; run.gamma1 = gam[1][1];  // instance i of a batch uses sets[i].challenges[chal]
  const size_t zn = S ? S->zr : Z;                       // Z columns computed here (the split: this rank's range)
  const PairCols* pairs = S ? S->d_pairs_own : P->d_pairs;
  // MEASURED and dropped (profiles/r3_ab_z_overlap.txt): only the first column chunk in front of the commit pipeline and the
  // other Z columns on a third stream beside that chunk's transforms and sponge -- the stage in front shrinks by 0.2 ms (a
  // single workgroup's scan chain is 0.36 ms long), the Z commitment grows by 0.44 ms (26.25 -> 26.5 ms per proof, five pairs).
  launch_perm_z(P, pairs, zn, run.gamma0.v, run.gamma1.v, P->d_zval, P->stream);
  HIPC(hipGetLastError());
  return run.next_stage(ST_Z_COMMIT);
}
static int stage_z_commit(ProofRun& run) {
  sbn_prover* P = run.P; SplitCtx* S = run.S;
  const size_t C = P->air.ncols, Z = P->air.nzs;
  if (S) {
    if (int rc = commit_split(P, S->zs, P->d_zval, false, P->d_zcoef, S->zlde_l, S->zlde_n, P->tree_z)) return rc;
  } else {
    if (C > 4) if (int rc = absorb_times(P, C, EX_TRACE_ABSORB_MS)) return rc;   // (27 event queries: behind the Z kernel, not in front of it)
    if (Z) if (int rc = commit_pipeline(P, P->d_zval, P->d_zcoef, P->d_zlde, Z, P->tree_z, EX_Z_ABSORB_MS, EX_Z_ABSORB_LAUNCHES, nullptr, P->compact ? P->d_zlde : nullptr)) return rc;
  }
  if (int rc = run.next_stage(ST_QUOTIENT_EVAL)) return rc;
  return Z ? run.observe_cap(P->tree_z, run.z_cap, S != nullptr) : 0;
}

// P3 quotient -------------------------------------------------------------------------------------
static int stage_quotient_eval(ProofRun& run) {
  sbn_prover* P = run.P; SplitCtx* S = run.S; hipStream_t st = P->stream;
  const size_t n = P->n, m = P->m, qn = 2 * n, Z = P->air.nzs;   // qn: points of the quotient's domain
  for (int j = 0; j < SBN_NCH; j++) run.alphas[j] = run.ch.challenge();
  if (int rc = upload_alpha_tables(P, run.alphas)) return rc;
  QuotientParams qp{};
  // starky evaluates the quotient on the coset of qn = 2n points (quotient_degree_bits = 1): quotient point k is LDE row
  // k << (rate_bits - 1), its next row quotient point k + 2.  The LDE stays in natural row order, so this is a strided view
  // (the section on rate_bits, has the byte counts against a dense copy); at rate_bits 1 the stride is one row.
  qp.lde = P->d_lde; qp.zlde = P->d_zlde; qp.m = qn; qp.next_step = 2;  // 2^quotient_degree_bits
  qp.lde_stride = m; qp.row_log = P->cfg.rate_bits - 1;
  if (P->compact) { qp.lde_stride = qn; qp.row_log = 0; }   // d_lde / d_zlde hold the quotient's rows only, densely
  qp.lde_next = qp.lde; qp.zlde_next = qp.zlde; qp.row_shift = 0; qp.row_rho = 0;
  if (S) {
    // this rank's LDE points j * R + rho; the row two LDE points on is local row j + 1 (two ranks) or sits at local row j
    // of the second plane (four ranks and more)
    qp.lde = S->lde_l; qp.zlde = S->zlde_l; qp.m = S->ml; qp.lde_stride = S->ml; qp.row_shift = S->log_r; qp.row_rho = S->rho;   // (rate_bits 1: create_ctx)
    qp.lde_next = S->planes == 2 ? S->lde_n : S->lde_l; qp.zlde_next = S->planes == 2 ? S->zlde_n : S->zlde_l;
    qp.next_step = S->comm.world == 1 ? 2 : (S->comm.world == 2 ? 1 : 0);
  }
  qp.xs = P->d_xs; qp.lag_first = P->d_lag_first; qp.lag_last = P->d_lag_last;
  F gn = f_exp_pow2(F(GL_GEN), P->degree_bits);
  qp.zh_inv[0] = f_inv(gn - F(1)).v; qp.zh_inv[1] = f_inv(-gn - F(1)).v;  // Z_H(7 w^i) = 7^N (-1)^i - 1
  qp.last = f_inv(f_root_of_unity(P->degree_bits)).v;
  quotient_segments(P, run.alphas, qp);
  qp.gamma0 = run.gamma0.v; qp.gamma1 = run.gamma1.v; qp.qout = P->d_q;
  if (S) qp.qout = (u64*)S->comm.send_buf;   // [2][ml]: all-gathered below
  qp.part = P->d_part;   // QSEG x SBN_NCH planes of qn words = 16 n of its 64 n (the FRI combine's scratch, idle here)
  const size_t qblocks = (qp.m + 255) / 256;
#ifdef SBN_DIAG   // diagnostic builds only (make CXXFLAGS+=-DSBN_DIAG): time single segments; the proof is invalid unless the mask is 15
  { const char* e = std::getenv("SBN_DIAG_QUOTIENT_SEGMASK"); if (e) qp.seg_mask = (u32)atoi(e) & 0xfu; }
  if (qp.seg_mask != 0xfu) HIPC(hipMemsetAsync(qp.part, 0, (size_t)QSEG * SBN_NCH * qp.m * sizeof(u64), st));
#endif
  // AIR head and tail on the main stream, the permutation checks beside them on the second stream (idle here)
  HIPC(hipEventRecord(P->chunk_ready[3], st));
  HIPC(hipStreamWaitEvent(P->hstream, P->chunk_ready[3], 0));
  if (int rc = launch_quotient_parts(P, qp, qblocks)) return rc;
  HIPC(hipEventRecord(P->hash_done, P->hstream));
  HIPC(hipStreamWaitEvent(st, P->hash_done, 0));
  hipLaunchKernelGGL(quotient_combine_kernel, blocks(qp.m), dim3(256), 0, st, qp);
  HIPC(hipGetLastError());
  if (S) {
    // quotient values of every rank's points -> all ranks, natural order; the 4 quotient columns are then committed on
    // every rank alike (no exchange: 4 columns)
    if (int rc = split_all_gather_device(P, 2 * S->ml)) return rc;
    hipLaunchKernelGGL(split_unpack_rows_kernel, blocks(m), dim3(256), 0, st, S->scratch, m, 2u, S->log_r, P->d_q);
    HIPC(hipGetLastError());
  } else if (Z > 4) { if (int rc = absorb_times(P, Z, EX_Z_ABSORB_MS)) return rc; }   // behind the quotient kernel
  return run.next_stage(ST_QUOTIENT_COMMIT);
}
static int stage_quotient_commit(ProofRun& run) {
  sbn_prover* P = run.P;
  const size_t qn = 2 * P->n;
  // coset_ifft(7) of the 2 quotient value vectors (size qn = 2n), in place via tmp; the result viewed as
  // [4][n] is exactly quotient_poly.chunks(degree) in the order q0_lo, q0_hi, q1_lo, q1_hi.
  if (int rc = ntt_columns(P, P->d_q, qn, P->d_q, qn, P->d_tmp, P->m, 2, P->degree_bits + 1, true, qn, nullptr, P->d_shift_inv, host_inv_pow2(P->degree_bits + 1))) return rc;
  if (int rc = lde_coeffs(P, P->d_q, P->d_qlde, 4)) return rc;
  if (int rc = tree_from_matrix(P, P->tree_q, P->d_qlde, 4)) return rc;
  if (int rc = run.next_stage(ST_OPENINGS)) return rc;
  return run.observe_cap(P->tree_q, run.q_cap, false);
}

// P4 openings -------------------------------------------------------------------------------------
// The split (world > 1): this rank evaluates its own trace / Z columns at both points (the quotient columns everywhere; own columns
// sit compactly in local order at the start of the trace / Z sections of d_open), the values are all-gathered on the host,
// scattered to their global positions and observed in transcript order
static int openings_split(ProofRun& run) {
  sbn_prover* P = run.P; SplitCtx* S = run.S; Challenger& ch = run.ch; hipStream_t st = P->stream;
  const size_t n = P->n, C = P->air.ncols, Z = P->air.nzs;
  const u64 *zp0 = P->d_zpow, *zp1 = P->d_zpow + n, *zp2 = P->d_zpow + 2 * n, *zp3 = P->d_zpow + 3 * n;
  auto open_k = n % 1024 == 0 ? openings_kernel<4> : openings_kernel<1>;
  if (S->cr) hipLaunchKernelGGL(open_k, dim3((unsigned)S->cr), dim3(256), 0, st, P->d_coef, n, zp0, zp1, zp2, zp3, P->d_open);
  if (S->zr) hipLaunchKernelGGL(open_k, dim3((unsigned)S->zr), dim3(256), 0, st, P->d_zcoef, n, zp0, zp1, zp2, zp3, P->d_open + C * 4);
  hipLaunchKernelGGL(open_k, dim3(4), dim3(256), 0, st, P->d_q, n, zp0, zp1, zp2, zp3, P->d_open + (C + Z) * 4);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(P->h_open, P->d_open, (C + Z + 4) * 4 * sizeof(u64), hipMemcpyDeviceToHost, st));
  if (int rc = run.next_stage(ST_FRI_COMBINE)) return rc;
  HIPC(stream_wait(st));
  const u32 R = S->comm.world;
  const size_t cmax = S->cs.max_own(), zmax = S->zs.max_own(), per = (cmax + zmax) * 4;
  std::vector<u64> mine(per, 0), all((size_t)R * per);
  memcpy(mine.data(), P->h_open, S->cr * 4 * sizeof(u64));
  memcpy(mine.data() + cmax * 4, P->h_open + C * 4, S->zr * 4 * sizeof(u64));
  if (int rc = split_all_gather_host(P, mine.data(), all.data(), per * sizeof(u64))) return rc;
  for (u32 r = 0; r < R; r++) {
    const u64* src = all.data() + (size_t)r * per;
    for (size_t l = 0, cnt = S->cs.own_cols(r); l < cnt; l++) memcpy(P->h_open + S->cs.global_col(r, l) * 4, src + l * 4, 4 * sizeof(u64));
    for (size_t l = 0, cnt = S->zs.own_cols(r); l < cnt; l++) memcpy(P->h_open + (C + S->zs.global_col(r, l)) * 4, src + (cmax + l) * 4, 4 * sizeof(u64));
  }
  const u64* open = run.open2 = run.open;   // one pass: both points of a column sit in one row of h_open
  for (size_t p = 0; p < C + Z + 4; p++) { ch.observe(F(open[4 * p])); ch.observe(F(open[4 * p + 1])); }
  for (size_t p = 0; p < C + Z; p++) { ch.observe(F(open[4 * p + 2])); ch.observe(F(open[4 * p + 3])); }
  return 0;
}
static int openings_single(ProofRun& run) {
  sbn_prover* P = run.P; Challenger& ch = run.ch; hipStream_t st = P->stream;
  const size_t n = P->n, C = P->air.ncols, Z = P->air.nzs;
  const u64 *open = run.open, *open2 = run.open2;
  auto open1_k = n % 1024 == 0 ? openings1_kernel<4> : openings1_kernel<1>;
  const u64 *zp0 = P->d_zpow, *zp1 = P->d_zpow + n, *zp2 = P->d_zpow + 2 * n, *zp3 = P->d_zpow + 3 * n;
  // The host hashes ~3 columns per microsecond, the device evaluates ~5: the trace columns at zeta go out in slices that
  // double in size (C/16, C/8, C/4, rest), so the host starts after a sixteenth of an opening pass and is never starved.
  size_t sl[5] = {0, C / 16, C / 16 + C / 8, C / 16 + C / 8 + C / 4, C};
  for (int k = 0; k < 4; k++) {
    const size_t a = sl[k], cnt = sl[k + 1] - sl[k];
    if (cnt) {
      hipLaunchKernelGGL(open1_k, dim3((unsigned)cnt), dim3(256), 0, st, P->d_coef + a * n, n, zp0, zp1, P->d_open + a * 4, 0u);
      HIPC(hipMemcpyAsync(P->h_open + a * 4, P->d_open + a * 4, cnt * 4 * sizeof(u64), hipMemcpyDeviceToHost, st));
    }
    HIPC(hipEventRecord(P->chunk_ready[8 + k], st));  // (the commit pipeline's chunk events are idle here)
  }
  // Z and quotient at zeta, then everything at g*zeta, again in slices: the host (0.86 us per permutation, 4 columns each)
  // is the slower side, and it must never find the next values missing -- with the trace at g*zeta evaluated last in one
  // kernel it idled 0.3 ms before it.
  if (Z) hipLaunchKernelGGL(open1_k, dim3((unsigned)Z), dim3(256), 0, st, P->d_zcoef, n, zp0, zp1, P->d_open + C * 4, 0u);
  hipLaunchKernelGGL(open1_k, dim3(4), dim3(256), 0, st, P->d_q, n, zp0, zp1, P->d_open + (C + Z) * 4, 0u);
  HIPC(hipMemcpyAsync(P->h_open + C * 4, P->d_open + C * 4, (Z + 4) * 4 * sizeof(u64), hipMemcpyDeviceToHost, st));
  HIPC(hipEventRecord(P->chunk_ready[1], st));
  size_t sn[5] = {0, C / 4, C / 2, C / 2 + C / 4, C};
  for (int k = 0; k < 4; k++) {
    const size_t a = sn[k], cnt = sn[k + 1] - sn[k];
    if (cnt) {
      hipLaunchKernelGGL(open1_k, dim3((unsigned)cnt), dim3(256), 0, st, P->d_coef + a * n, n, zp2, zp3, P->d_open + a * 4, 2u);
      HIPC(hipMemcpyAsync(P->h_open2 + a * 4, P->d_open + a * 4, cnt * 4 * sizeof(u64), hipMemcpyDeviceToHost, st));
    }
    HIPC(hipEventRecord(P->chunk_ready[12 + k], st));
  }
  if (Z) hipLaunchKernelGGL(open1_k, dim3((unsigned)Z), dim3(256), 0, st, P->d_zcoef, n, zp2, zp3, P->d_open + C * 4, 2u);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(P->h_open2 + C * 4, P->d_open + C * 4, Z * 4 * sizeof(u64), hipMemcpyDeviceToHost, st));
  if (int rc = run.next_stage(ST_FRI_COMBINE)) return rc;   // in front of the host hashing
  // observe_openings: batch zeta = local ++ perm_zs ++ quotient ; batch g*zeta = next ++ perm_zs_next
  for (int k = 0; k < 4; k++) {
    HIPC(event_wait(P->chunk_ready[8 + k]));
    for (size_t p = sl[k]; p < sl[k + 1]; p++) { ch.observe(F(open[4 * p])); ch.observe(F(open[4 * p + 1])); }
  }
  HIPC(event_wait(P->chunk_ready[1]));
  for (size_t p = C; p < C + Z + 4; p++) { ch.observe(F(open[4 * p])); ch.observe(F(open[4 * p + 1])); }
  for (int k = 0; k < 4; k++) {
    HIPC(event_wait(P->chunk_ready[12 + k]));
    for (size_t p = sn[k]; p < sn[k + 1]; p++) { ch.observe(F(open2[4 * p + 2])); ch.observe(F(open2[4 * p + 3])); }
  }
  HIPC(stream_wait(st));
  for (size_t p = C; p < C + Z; p++) { ch.observe(F(open2[4 * p + 2])); ch.observe(F(open2[4 * p + 3])); }
  return 0;
}
static int stage_openings(ProofRun& run) {
  sbn_prover* P = run.P; hipStream_t st = P->stream;
  const size_t n = P->n;
  run.zeta = run.ch.ext_challenge();
  F g = f_root_of_unity(P->degree_bits);
  if (e2_exp_pow2(run.zeta, P->degree_bits) == E2(F(1), F(0))) return fail(SBN_ERR_HIP, "opening point is in the subgroup");
  run.zeta_next = run.zeta * g;
  hipLaunchKernelGGL(ext_pow_table_kernel, blocks(n), dim3(256), 0, st, P->d_zpow, P->d_zpow + n, n, run.zeta.a.v, run.zeta.b.v);
  hipLaunchKernelGGL(ext_pow_table_kernel, blocks(n), dim3(256), 0, st, P->d_zpow + 2 * n, P->d_zpow + 3 * n, n, run.zeta_next.a.v, run.zeta_next.b.v);
  // Transcript order: local (trace at zeta), Z at zeta, quotient at zeta, then next (trace at g*zeta), Z at g*zeta.  The
  // 1,220 sequential permutations that hash them are the longest host stretch of a proof, so the device produces the
  // values in that order behind three events: trace at zeta alone first (the host starts hashing after half an opening
  // pass), then Z and quotient at both points, then trace at g*zeta -- the coefficients are read twice, in time the
  // device would otherwise spend waiting for the host.
  run.open = P->h_open; run.open2 = P->h_open2;
  return (run.S && run.S->comm.world > 1) ? openings_split(run) : openings_single(run);
}

// P5 FRI ------------------------------------------------------------------------------------------
// The weights alpha^(offset + g * stride) of the ceil(npoly / GS) groups of one matrix, appended to `wall`; returns where they start.
static size_t fri_plan_weights(std::vector<u64>& wall, E2 fri_alpha, u32 GS, u32 npoly, E2 weight0, u64 stride) {
  const size_t off = wall.size();
  E2 ag = e2_pow(fri_alpha, stride), cur = weight0;
  for (u32 k = 0, ng = (npoly + GS - 1) / GS; k < ng; k++) { wall.push_back(cur.a.v); wall.push_back(cur.b.v); cur = cur * ag; }
  return off;
}
// (oa, ob) = [accumulate: (oa, ob) +] sum over the groups of `coeffs` [npoly][n], GS polynomials each, of weight * sum_k alpha^k f_k:
// groups run on grid.y, <= 32 per launch; the weights from P->d_w + woff, alpha^k from the two planes at P->d_apow
static int fri_combine(sbn_prover* P, u32 GS, const u64* coeffs, u32 npoly, size_t woff, u64* oa, u64* ob, int accumulate) {
  const size_t n = P->n;
  const u32 ng = (npoly + GS - 1) / GS;
  for (u32 g0 = 0; g0 < ng; g0 += 32) {
    u32 gc = std::min<u32>(32, ng - g0);
    hipLaunchKernelGGL(fri_combine_partial_kernel, dim3((unsigned)((n + 255) / 256), gc), dim3(256), 0, P->stream, coeffs + (size_t)g0 * GS * n, n,
                       npoly - g0 * GS, GS, P->d_apow, P->d_apow + GS, P->d_part, P->d_part + 32 * n);
    hipLaunchKernelGGL(fri_combine_reduce_kernel, blocks(n), dim3(256), 0, P->stream, P->d_part, P->d_part + 32 * n, n, gc, P->d_w + woff + 2 * g0, oa, ob,
                       (accumulate || g0 > 0) ? 1 : 0);
  }
  HIPC(hipGetLastError());
  return 0;
}
// (ca, cb) / (X - z), n - 1 coefficients, into d_fcoef: chunk remainders, their scan, then the quotient (mul, accumulate: pass 3)
static void fri_divide(sbn_prover* P, const u64* ca, const u64* cb, E2 z, E2 mul, int accumulate) {
  const size_t nch = P->n / DBL_CHUNK;  // a power of two >= 32
  hipStream_t st = P->stream;
  u64 *ha = P->d_part, *hb = P->d_part + nch;
  hipLaunchKernelGGL(divide_by_linear_pass1, blocks(nch), dim3(256), 0, st, ca, cb, nch, z.a.v, z.b.v, ha, hb);
  hipLaunchKernelGGL(divide_by_linear_pass2, dim3(1), dim3(256), 0, st, ha, hb, nch, z.a.v, z.b.v);
  hipLaunchKernelGGL(divide_by_linear_pass3, blocks(nch), dim3(256), 0, st, ca, cb, nch, z.a.v, z.b.v, ha, hb, mul.a.v, mul.b.v, P->d_fcoef, P->d_fcoef + P->m, accumulate,
                     fri_times_x(P->cfg));
}
static int stage_fri_combine(ProofRun& run) {
  sbn_prover* P = run.P; SplitCtx* S = run.S; hipStream_t st = P->stream;
  const size_t n = P->n, m = P->m, C = P->air.ncols, Z = P->air.nzs;
  const E2 fri_alpha = run.fri_alpha = run.ch.ext_challenge();
  // F1 = sum_{j < C+Z} alpha^j f_j ; F0 = F1 + alpha^(C+Z) * sum_{j<4} alpha^j q_j
  // polys per group; groups run on grid.y, <= 32 per launch.  The split: a group = one own column block (ColShare), whose
  // weight is alpha^(global position of the block); consecutive own blocks are `world` blocks apart.
  const u32 RW = S ? S->comm.world : 1;
  const u32 GS = RW > 1 ? (u32)SPLIT_BLOCK : 128;
  // all group weights alpha^(offset + g*stride) are known up front: one upload, no host sync in the loop
  std::vector<u64> wall;   // (staged here, uploaded from the context's pinned h_w)
  // the split: this rank's columns only, with the weights of their global positions
  const size_t tc0 = S ? (size_t)S->comm.rank * GS : 0, tcn = S ? S->cr : C, tzn = S ? S->zr : Z;
  const u64 gstride = (u64)GS * RW;
  const size_t w_t = tcn ? fri_plan_weights(wall, fri_alpha, GS, (u32)tcn, e2_pow(fri_alpha, RW > 1 ? tc0 : 0), gstride) : 0;
  const size_t w_z = tzn ? fri_plan_weights(wall, fri_alpha, GS, (u32)tzn, e2_pow(fri_alpha, C + (RW > 1 ? tc0 : 0)), gstride) : 0;
  const size_t w_q = fri_plan_weights(wall, fri_alpha, GS, 4, e2_pow(fri_alpha, C + Z), GS);
  if (wall.size() > 4096) return fail(SBN_ERR_UNSUPPORTED, "too many FRI combine groups");
  memcpy(P->h_w, wall.data(), wall.size() * sizeof(u64));   // pinned: the upload needs no host wait behind it
  HIPC(hipMemcpyAsync(P->d_w, P->h_w, wall.size() * sizeof(u64), hipMemcpyHostToDevice, st));
  // alpha^k, k < GS, as two planes in the quotient's alpha-power buffer (idle now; it holds at least 1,025 words per plane)
  hipLaunchKernelGGL(ext_pow_table_kernel, dim3(1), dim3(GS), 0, st, P->d_apow, P->d_apow + GS, (size_t)GS, fri_alpha.a.v, fri_alpha.b.v);
  u64 *f1a = P->d_fb, *f1b = P->d_fb + n, *f0a = P->d_fa, *f0b = P->d_fa + n;
  if (!tcn) HIPC(hipMemsetAsync(f1a, 0, 2 * n * sizeof(u64), st));
  if (tcn) if (int rc = fri_combine(P, GS, P->d_coef, (u32)tcn, w_t, f1a, f1b, 0)) return rc;
  if (tzn) if (int rc = fri_combine(P, GS, P->d_zcoef, (u32)tzn, w_z, f1a, f1b, 1)) return rc;
  if (S) {
    // F1 = sum over ranks of the partial sums: all-gather + a mod-p add kernel (RCCL has no mod-p reduction); 16 N bytes per rank
    HIPC(hipMemcpyAsync(S->comm.send_buf, f1a, 2 * n * sizeof(u64), hipMemcpyDeviceToDevice, st));
    if (int rc = split_all_gather_device(P, 2 * n)) return rc;   // stream-ordered behind the copy
    hipLaunchKernelGGL(split_modadd_kernel, blocks(2 * n), dim3(256), 0, st, S->scratch, 2 * n, S->comm.world, f1a);
    HIPC(hipGetLastError());
  }
  HIPC(hipMemcpyAsync(f0a, f1a, 2 * n * sizeof(u64), hipMemcpyDeviceToDevice, st));
  if (int rc = fri_combine(P, GS, P->d_q, 4, w_q, f0a, f0b, 1)) return rc;
  // final_poly = alpha^(C+Z) * (F0 / (X - zeta)) + F1 / (X - g zeta), n-1 coefficients each; times X (a zero in front, plonky2
  // 0.1.x, sbn_config.fri_variant) or zero-padded at the end; then lde -> m
  HIPC(hipMemsetAsync(P->d_fcoef, 0, 2 * m * sizeof(u64), st));
  fri_divide(P, f0a, f0b, run.zeta, E2{F(0), F(0)}, 0);
  fri_divide(P, f1a, f1b, run.zeta_next, e2_pow(fri_alpha, C + Z), 1);
  HIPC(hipGetLastError());
  return run.next_stage(ST_FRI_LAYERS);
}
// fri_committed_trees
static int stage_fri_layers(ProofRun& run) {
  sbn_prover* P = run.P; Challenger& ch = run.ch; hipStream_t st = P->stream;
  const size_t n = P->n, m = P->m;
  u32 bits = P->lde_log;
  u64* coef = P->d_fcoef; u64* coef_alt = P->d_fcoef2;
  size_t clen = m;  // coefficient vector length (planes at coef, coef + clen)
  F shift(GL_GEN);
  for (size_t li = 0; li < P->fri.arity_bits.size(); li++) {
    u32 ab = P->fri.arity_bits[li];
    u64* va = P->fri_vals[li]; u64* vb = va + clen;
    // values = coeffs.coset_fft(shift): scale by shift^i then NTT (2 base planes).  Layer 0 is n coefficients zero-padded to m on
    // the coset of 7: the coset LDE of lde_coeffs, out of place, whose first pass skips the zero half
    if (li == 0) {
      if (int rc = ntt_columns(P, coef, clen, va, clen, P->d_tmp, m, 2, bits, false, n, P->d_shift, nullptr, 1)) return rc;
    } else {
      HIPC(hipMemcpyAsync(va, coef, 2 * clen * sizeof(u64), hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(scale_pow_kernel, blocks(clen), dim3(256), 0, st, va, clen, shift.v);
      hipLaunchKernelGGL(scale_pow_kernel, blocks(clen), dim3(256), 0, st, vb, clen, shift.v);
      if (int rc = ntt_columns(P, va, clen, va, clen, P->d_tmp, m, 2, bits, false, clen, nullptr, nullptr, 1)) return rc;
    }
    DevTree& t = P->fri_trees[li];
    if (t.nleaf <= 16384) hipLaunchKernelGGL(fri_leaf_hash_coop_kernel, blocks(t.nleaf * 16), dim3(256), 0, st, va, vb, bits, ab, t.d);
    else hipLaunchKernelGGL(fri_leaf_hash_kernel, blocks(t.nleaf), dim3(256), 0, st, va, vb, bits, ab, t.d);
    if (int rc = tree_build_inner(P, t, st)) return rc;
    run.fri_caps.emplace_back();
    if (int rc = run.observe_cap(t, run.fri_caps.back(), false)) return rc;
    E2 beta = ch.ext_challenge();
    size_t nout = clen >> ab;
    hipLaunchKernelGGL(fri_fold_kernel, blocks(nout), dim3(256), 0, st, coef, coef + clen, nout, 1u << ab, beta.a.v, beta.b.v, coef_alt, coef_alt + nout);
    HIPC(hipGetLastError());
    std::swap(coef, coef_alt);
    clen = nout; bits -= ab;
    shift = f_pow(shift, (u64)1 << ab);
  }
  size_t fl = clen >> P->cfg.rate_bits;  // coefficients beyond are zero
  run.final_poly.resize(2 * fl);
  std::vector<u64> fa(fl), fb(fl);
  HIPC(hipMemcpyAsync(fa.data(), coef, fl * sizeof(u64), hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(fb.data(), coef + clen, fl * sizeof(u64), hipMemcpyDeviceToHost, st));
  HIPC(stream_wait(st));
  for (size_t i = 0; i < fl; i++) { run.final_poly[2 * i] = fa[i]; run.final_poly[2 * i + 1] = fb[i]; ch.observe(F(fa[i])); ch.observe(F(fb[i])); }
  return run.next_stage(ST_POW);
}
// fri_proof_of_work: smallest witness
static int stage_pow(ProofRun& run) {
  sbn_prover* P = run.P; Challenger& ch = run.ch; hipStream_t st = P->stream;
  PowParams pp{};
  for (int i = 0; i < 12; i++) pp.state[i] = ch.st[i].v;
  for (size_t i = 0; i < ch.in.size(); i++) pp.state[i] = ch.in[i].v;
  pp.wpos = (u32)ch.in.size(); pp.min_lz = P->cfg.proof_of_work_bits; pp.result = P->d_pow;
  // candidates are scanned in increasing windows (2^17, then 2^20 each): a 16-bit PoW is found in the
  // first window with probability 1 - e^-2; the smallest witness over the scanned prefix is kept.
  u64 base = 0;
  for (int round = 0; run.pow_witness == ~0ULL; round++) {
    const u64 BATCH = round == 0 ? (1ULL << 17) : (1ULL << 20);
    if (base >= GLP - BATCH) return fail(SBN_ERR_HIP, "proof of work failed");
    u64 init = ~0ULL;
    HIPC(hipMemcpyAsync(P->d_pow, &init, sizeof(u64), hipMemcpyHostToDevice, st));
    pp.base = base; pp.count = BATCH;
    hipLaunchKernelGGL(pow_kernel, blocks(BATCH), dim3(256), 0, st, pp);
    HIPC(hipMemcpyAsync(&run.pow_witness, P->d_pow, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPC(stream_wait(st));
    base += BATCH;
  }
  ch.observe(F(run.pow_witness));
  F resp = ch.challenge();
  u32 lz = resp.v ? (u32)__builtin_clzll(resp.v) : 64;
  if (lz < P->cfg.proof_of_work_bits) return fail(SBN_ERR_HIP, "proof-of-work witness check failed");
  return run.next_stage(ST_QUERIES);
}
// The initial-tree section of every query into d_qbuf at `off` (advanced): the opened row of a matrix and its Merkle path.
// A row-sharded matrix (the split): `rows` local rows, leaf index inside this rank's subtrees; the rank that owns a
// query's leaf holds its whole row and its Merkle path up to the cap (other ranks gather a row that is dropped below)
// coef (compact storage of a wide matrix; else null): the rows are not resident and are evaluated from the coefficients
// (lde_compact.hip; its point tables sit in d_part, idle since the FRI combine)
static int query_initial(sbn_prover* P, size_t& off, const u64* mat, size_t ncols, const DevTree& t, size_t rows, u32 log_rows, const u32* d_index, const u64* coef = nullptr) {
  hipStream_t st = P->stream;
  const u32 nq = P->cfg.num_query_rounds, nsib = P->lde_log - P->cfg.cap_height;
  if (coef) { if (int rc = launch_query_rows(coef, ncols, P->n, P->lde_log, P->d_shift, P->d_tw_f, d_index, nq, P->d_part, P->d_qbuf, P->qstride, off, st)) return rc; }
  else hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((ncols + 255) / 256), nq), dim3(256), 0, st, mat, rows, log_rows, (u32)ncols, d_index, P->d_qbuf, P->qstride, off);
  off += ncols;
  hipLaunchKernelGGL(gather_siblings_kernel, dim3(nq), dim3(128), 0, st, t.d, t.nleaf, nsib, d_index, 0u, P->d_qbuf, P->qstride, off);
  off += (size_t)nsib * 4;
  return 0;
}
// fri_prover_query_rounds
static int stage_queries(ProofRun& run) {
  sbn_prover* P = run.P; SplitCtx* S = run.S; hipStream_t st = P->stream;
  const size_t m = P->m, C = P->air.ncols, Z = P->air.nzs;
  const u32 nq = P->cfg.num_query_rounds;
  run.qwords.resize(P->qstride * nq);
  run.idx.resize(nq); run.idx_local.resize(nq);
  for (u32 q = 0; q < nq; q++) run.idx[q] = (u32)(run.ch.challenge().v % m);
  HIPC(hipMemcpyAsync(P->d_idx, run.idx.data(), nq * sizeof(u32), hipMemcpyHostToDevice, st));
  size_t off = 0;
  if (S) {
    for (u32 q = 0; q < nq; q++) run.idx_local[q] = run.idx[q] & (u32)(S->ml - 1);
    HIPC(hipMemcpyAsync(S->d_idx_local, run.idx_local.data(), nq * sizeof(u32), hipMemcpyHostToDevice, st));
    if (int rc = query_initial(P, off, S->lde_l, C, P->tree_t, S->ml, P->lde_log - S->log_r, S->d_idx_local)) return rc;
    if (Z) if (int rc = query_initial(P, off, S->zlde_l, Z, P->tree_z, S->ml, P->lde_log - S->log_r, S->d_idx_local)) return rc;
    run.split_section = off;
  } else {
    if (int rc = query_initial(P, off, P->d_lde, C, P->tree_t, m, P->lde_log, P->d_idx, P->compact ? P->d_coef : nullptr)) return rc;
    if (Z) if (int rc = query_initial(P, off, P->d_zlde, Z, P->tree_z, m, P->lde_log, P->d_idx, P->compact ? P->d_zcoef : nullptr)) return rc;
  }
  if (int rc = query_initial(P, off, P->d_qlde, 4, P->tree_q, m, P->lde_log, P->d_idx)) return rc;
  u32 bits = P->lde_log, shift = 0;
  for (size_t li = 0; li < P->fri.arity_bits.size(); li++) {
    u32 ab = P->fri.arity_bits[li];
    shift += ab;
    size_t len = (size_t)1 << bits;
    hipLaunchKernelGGL(gather_fri_leaf_kernel, dim3(nq), dim3(64), 0, st, P->fri_vals[li], P->fri_vals[li] + len, bits, ab, P->d_idx, shift, P->d_qbuf, P->qstride, off);
    off += 2 * ((size_t)1 << ab);
    const DevTree& t = P->fri_trees[li];
    hipLaunchKernelGGL(gather_siblings_kernel, dim3(nq), dim3(128), 0, st, t.d, t.nleaf, t.nlevels, P->d_idx, shift, P->d_qbuf, P->qstride, off);
    off += (size_t)t.nlevels * 4;
    bits -= ab;
  }
  HIPC(hipGetLastError());
  if (off != P->qstride) return fail(SBN_ERR_HIP, "internal: query layout mismatch (%zu vs %zu)", off, P->qstride);
  HIPC(hipMemcpyAsync(run.qwords.data(), P->d_qbuf, run.qwords.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
  if (int rc = run.next_stage(ST_COUNT)) return rc;
  HIPC(stream_wait(st));
  if (S) {
    // the trace / Z sections of every query come from the rank that owns the leaf: all-gather on the host and pick
    const u32 R = S->comm.world;
    const size_t sec = run.split_section;
    std::vector<u64> mine((size_t)nq * sec), all((size_t)R * nq * sec);
    for (u32 q = 0; q < nq; q++) memcpy(mine.data() + (size_t)q * sec, run.qwords.data() + (size_t)q * P->qstride, sec * sizeof(u64));
    if (int rc = split_all_gather_host(P, mine.data(), all.data(), mine.size() * sizeof(u64))) return rc;
    for (u32 q = 0; q < nq; q++) {
      const u32 owner = run.idx[q] >> (P->lde_log - S->log_r);
      memcpy(run.qwords.data() + (size_t)q * P->qstride, all.data() + ((size_t)owner * nq + q) * sec, sec * sizeof(u64));
    }
    float xms = 0;   // device time inside the exchanges (waiting for the peers' blocks included)
    for (size_t i = 0; i + 1 < S->tev_used; i += 2) { float t = 0; HIPC(hipEventElapsedTime(&t, S->tev[i], S->tev[i + 1])); xms += t; }
    P->stage_ms[ST_COUNT + EX_COMM_MS] = xms;
  }
  return 0;
}
// the canonical proof words (layout: include/sbn.h)
static int assemble_proof(const ProofRun& run, sbn_proof** out) {
  const sbn_prover* P = run.P;
  const sbn_config& cfg = P->cfg;
  const size_t C = P->air.ncols, Z = P->air.nzs;
  const u64 *open = run.open, *open2 = run.open2;
  sbn_proof* pr = new sbn_proof();
  pr->degree_bits = P->degree_bits;
  std::vector<u64>& w = pr->words;
  w.reserve(12 + 3 * run.capw() + (C + Z + 4) * 4 + run.fri_caps.size() * run.capw() + run.qwords.size() + run.final_poly.size() + 1 + P->pi.size());
  u64 hdr[12] = {PROOF_MAGIC, P->degree_bits, C, Z, 4, P->pi.size(), cfg.cap_height, cfg.rate_bits, run.fri_caps.size(), cfg.fri_arity_bits,
                 run.final_poly.size() / 2, cfg.num_query_rounds};
  w.insert(w.end(), hdr, hdr + 12);
  w.insert(w.end(), run.trace_cap.begin(), run.trace_cap.end());
  if (Z) w.insert(w.end(), run.z_cap.begin(), run.z_cap.end());
  w.insert(w.end(), run.q_cap.begin(), run.q_cap.end());
  for (size_t p = 0; p < C; p++) { w.push_back(open[4 * p]); w.push_back(open[4 * p + 1]); }          // local_values
  for (size_t p = 0; p < C; p++) { w.push_back(open2[4 * p + 2]); w.push_back(open2[4 * p + 3]); }    // next_values
  for (size_t p = C; p < C + Z; p++) { w.push_back(open[4 * p]); w.push_back(open[4 * p + 1]); }      // permutation_zs
  for (size_t p = C; p < C + Z; p++) { w.push_back(open2[4 * p + 2]); w.push_back(open2[4 * p + 3]); }  // permutation_zs_next
  for (size_t p = C + Z; p < C + Z + 4; p++) { w.push_back(open[4 * p]); w.push_back(open[4 * p + 1]); }  // quotient_polys
  for (auto& cap : run.fri_caps) w.insert(w.end(), cap.begin(), cap.end());
  w.insert(w.end(), run.qwords.begin(), run.qwords.end());
  w.insert(w.end(), run.final_poly.begin(), run.final_poly.end());
  w.push_back(run.pow_witness);
  w.insert(w.end(), P->pi.begin(), P->pi.end());
  *out = pr;
  return SBN_OK;
}
// up: null for sbn_prover_prove (the trace is resident); else the host trace sbn_prover_prove_host_trace streams in (trace_load.hip)
int prove_streamed(sbn_prover* P, const HostUpload* up, sbn_proof** out) {
  if (!P || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  *out = nullptr;
  if (!up && !P->loaded && !(P->sp && P->sp->comm.world > 1)) return fail(SBN_ERR_BAD_ARG, "no trace loaded");   // (split: agreed with the other ranks below)
  HIPC(hipSetDevice(P->device));
  ProofRun run;
  run.P = P; run.S = P->sp; run.up = up;
  if (int rc = run.next_stage(ST_TRACE_COMMIT)) return rc;   // (the first interval opens in front of the ranks' agreement)
  struct DeadlineScope { ~DeadlineScope() { t_wait_deadline_s = 0; } } deadline_scope;
  if (SplitCtx* S = run.S; S && S->comm.world > 1) {
    // every rank must have a witness before anyone walks into the first exchange (a rank whose generate_trace failed would
    // leave the others waiting for its blocks): agree on a status word first
    t_wait_deadline_s = P->set.comm_timeout_s;
    std::vector<uint32_t> st_all(S->comm.world, 0);
    const uint32_t mine = P->loaded ? 1u : 0u;
    if (int rc = split_all_gather_host(P, &mine, st_all.data(), sizeof(uint32_t))) return rc;
    for (u32 r = 0; r < S->comm.world; r++) if (!st_all[r]) return fail(SBN_ERR_BAD_ARG, "split proof abandoned: rank %u has no trace loaded", r);
  }
  if (!up && !P->loaded) return fail(SBN_ERR_BAD_ARG, "no trace loaded");
  int rc;
  if ((rc = stage_trace_commit(run)) || (rc = stage_perm_z(run)) || (rc = stage_z_commit(run)) || (rc = stage_quotient_eval(run)) ||
      (rc = stage_quotient_commit(run)) || (rc = stage_openings(run)) || (rc = stage_fri_combine(run)) || (rc = stage_fri_layers(run)) ||
      (rc = stage_pow(run)) || (rc = stage_queries(run)))
    return rc;
  for (int i = 0; i < ST_COUNT; i++) HIPC(hipEventElapsedTime(&P->stage_ms[i], P->ev[i], P->ev[i + 1]));
  if ((rc = assemble_proof(run, out))) return rc;
  if (run.fills_fixed) P->fixed_valid = true;   // every stage has run and been waited for: d_coef and d_lde hold those transforms
  if (P->guard_mode) return guard_check(P, out);   // include/sbn.h sbn_prover_set_guard (guard.hip): the streams are idle, the words final
  return SBN_OK;
}
extern "C" int sbn_prover_prove(sbn_prover* P, sbn_proof** out) { return prove_streamed(P, nullptr, out); }


// ---- building blocks for parity tests ---------------------------------------------------------------
// A stub context for the transforms of one (degree_bits, rate_bits, cap_height): the shape fields, the switches, the transform plan
// of a real context of this size (ntt_plan), one stream, and the buffers of `L` -- the caller's own, to which open() adds the
// transforms' scratch and tables (lde: those of the coset LDE too, as ntt_plan picks them) -- allocated through alloc_buffers and
// released through `owned` on every return path.
struct ScratchCtx {
  sbn_prover P{};
  ~ScratchCtx() { for (void* b : P.owned) (void)hipFree(b); if (P.stream) (void)hipStreamDestroy(P.stream); }
  int open(u32 degree_bits, u32 rate_bits, u32 cap_height, bool lde, std::vector<BufReq> L) {
    sbn_standard_fast_config(&P.cfg); P.cfg.cap_height = cap_height; P.cfg.rate_bits = rate_bits;
    P.degree_bits = degree_bits; P.lde_log = degree_bits + rate_bits; P.n = (size_t)1 << degree_bits; P.m = P.n << rate_bits; P.ntt_chunk = 64;
    if (int rc = use_current_device("no CPU fallback")) return rc;
    P.device = g_device;
    if (int rc = ntt_fast_setup()) return rc;
    { std::string serr; if (!P.set.load(serr)) return fail(SBN_ERR_BAD_ARG, "%s", serr.c_str()); }
    ntt_plan(&P);   // the transform kernels the prover picks at this size
    HIPC(hipStreamCreate(&P.stream));
    L.insert(L.end(), {words_req(&P.d_tmp, 64 * P.m), words_req(&P.d_tw_f, P.m), words_req(&P.d_tw_i, P.m), words_req(&P.d_shift, P.m)});
    if (lde && (P.ntt_fused || P.ntt_fused512)) L.push_back(words_req(&P.d_tmp2, 64 * P.m));
    if (lde && P.ntt_fused512) L.push_back(words_req(&P.d_shift_odd, P.n));
    if (lde && P.lde_za_log) L.push_back(words_req(&P.d_shift_za, P.n << P.lde_za_log));
    if (int rc = alloc_buffers(&P, L)) return rc;
    fill_transform_tables(&P);
    return 0;
  }
};

extern "C" int sbn_commit_values(const uint64_t* cols, size_t ncols, size_t n, uint32_t rate_bits, uint32_t cap_height, uint64_t* cap_out,
                                 uint64_t* coeffs_out, uint64_t* lde_out) {
  if (!cols || !cap_out || ncols == 0) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (rate_bits < 1 || rate_bits > 3 || n < 512 || (n & (n - 1))) return fail(SBN_ERR_UNSUPPORTED, "need rate_bits 1..3 and n a power of two >= 512");
  u32 lg = 0; while (((size_t)1 << lg) < n) lg++;
  if (lg + rate_bits > SBN_MAX_LDE_BITS) return fail(SBN_ERR_UNSUPPORTED, "n << rate_bits exceeds 2^%u points", SBN_MAX_LDE_BITS);
  // the range of config_supported: tree_shape computes the level count lg + rate_bits - cap_height unsigned, and lg + rate_bits >= 10
  if (cap_height < 1 || cap_height > 8) return fail(SBN_ERR_UNSUPPORTED, "cap_height must be 1..8");
  // a throw-away prover-like context built on the G1_OP shape would waste memory; build a minimal one
  ScratchCtx sc;
  sbn_prover& P = sc.P;
  const size_t m = n << rate_bits;
  u64 *d_vals = nullptr, *d_coef = nullptr, *d_lde = nullptr;
  std::vector<BufReq> L{words_req(&d_vals, ncols * n), words_req(&d_coef, ncols * n), words_req(&d_lde, ncols * m)};
  tree_shape(P.tree_t, m, cap_height);
  L.push_back(words_req(&P.tree_t.d, 2 * m * 4));
  if (ncols > 4) L.push_back(words_req(&P.d_sponge, 12 * m));
  if (int rc = sc.open(lg, rate_bits, cap_height, true, L)) return rc;
  if (hipMemcpy(d_vals, cols, ncols * n * sizeof(u64), hipMemcpyHostToDevice) != hipSuccess) return fail(SBN_ERR_HIP, "H2D failed");
  for (size_t c0 = 0; c0 < ncols; c0 += P.ntt_chunk)
    if (int rc = intt_lde_cols(&P, d_vals + c0 * n, d_coef + c0 * n, d_lde + c0 * m, std::min(P.ntt_chunk, ncols - c0))) return rc;
  if (ncols <= 4) {
    if (int rc = tree_from_matrix(&P, P.tree_t, d_lde, ncols)) return rc;
  } else {  // same chunked sponge as the prover (chunks of 64 columns), on one stream
    for (size_t c0 = 0; c0 < ncols; c0 += 64) {
      size_t nc = std::min<size_t>(64, ncols - c0);
      hipLaunchKernelGGL(leaf_absorb_kernel, blocks(m), dim3(256), 0, P.stream, d_lde + c0 * m, m, P.lde_log, (u32)nc, P.d_sponge,
                         c0 == 0 ? 1 : 0, c0 + 64 >= ncols ? 1 : 0, P.tree_t.d, (c0 + 64 < ncols && ncols - (c0 + 64) >= 8) ? 1 : 0);
    }
    if (int rc = tree_build_inner(&P, P.tree_t, P.stream)) return rc;
  }
  std::vector<u64> cap;
  if (int rc = tree_cap_to_host(&P, P.tree_t, cap)) return rc;
  memcpy(cap_out, cap.data(), cap.size() * sizeof(u64));
  if (coeffs_out && hipMemcpy(coeffs_out, d_coef, ncols * n * sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess) return fail(SBN_ERR_HIP, "D2H failed");
  if (lde_out && hipMemcpy(lde_out, d_lde, ncols * m * sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess) return fail(SBN_ERR_HIP, "D2H failed");
  return SBN_OK;
}

// The twin of sbn_commit_values for the compact storage: values -> coefficients through the transform plan of a prover of this
// height and rate, then the opened rows of the coset LDE from the coefficients by the kernels of lde_compact.hip.
extern "C" int sbn_lde_rows(const uint64_t* cols, size_t ncols, uint32_t degree_bits, uint32_t rate_bits, const uint32_t* leaf_indices, size_t count, uint64_t* rows_out) {
  if (!cols || !leaf_indices || !rows_out || ncols == 0 || count == 0) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (count > 65536) return fail(SBN_ERR_BAD_ARG, "at most 65536 leaf indices per call");
  if (rate_bits < 1 || rate_bits > 3 || degree_bits < 9 || degree_bits + rate_bits > SBN_MAX_LDE_BITS)
    return fail(SBN_ERR_UNSUPPORTED, "need rate_bits 1..3 and 9 <= degree_bits with degree_bits + rate_bits <= %u", SBN_MAX_LDE_BITS);
  const size_t n = (size_t)1 << degree_bits, m = n << rate_bits;
  for (size_t i = 0; i < count; i++) if (leaf_indices[i] >= m) return fail(SBN_ERR_BAD_ARG, "leaf index %zu is %u, beyond the %zu leaves", i, leaf_indices[i], m);
  ScratchCtx sc;
  sbn_prover& P = sc.P;
  u64 *d_vals = nullptr, *d_coef = nullptr, *d_table = nullptr, *d_out = nullptr; u32* d_index = nullptr;
  if (int rc = sc.open(degree_bits, rate_bits, 1, false,   // (no tree is built: the cap height is not read)
                       {words_req(&d_vals, ncols * n), words_req(&d_coef, ncols * n), words_req(&d_table, 64 * n), words_req(&d_out, count * ncols),
                        BufReq{(void**)&d_index, count * sizeof(u32)}}))
    return rc;
  if (hipMemcpy(d_vals, cols, ncols * n * sizeof(u64), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_index, leaf_indices, count * sizeof(u32), hipMemcpyHostToDevice) != hipSuccess) return fail(SBN_ERR_HIP, "H2D failed");
  if (int rc = intt_values(&P, d_vals, d_coef, ncols)) return rc;
  if (int rc = launch_query_rows(d_coef, ncols, n, P.lde_log, P.d_shift, P.d_tw_f, d_index, (u32)count, d_table, d_out, ncols, 0, P.stream)) return rc;
  if (hipStreamSynchronize(P.stream) != hipSuccess) return fail(SBN_ERR_HIP, "sbn_lde_rows: the kernels failed");
  if (hipMemcpy(rows_out, d_out, count * ncols * sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess) return fail(SBN_ERR_HIP, "D2H failed");
  return SBN_OK;
}

extern "C" int sbn_poseidon_permute_batch(uint64_t* states, size_t count) {
  if (!states) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (int rc = use_current_device("no CPU fallback")) return rc;
  for (size_t i = 0; i < count * 12; i++) if (states[i] >= GLP) return fail(SBN_ERR_NON_CANONICAL, "state word %zu is not canonical", i);
  DevWords w;
  if (int rc = w.alloc(count * 12)) return rc;
  HIPC(hipMemcpy(w.d, states, count * 12 * sizeof(u64), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(poseidon_batch_kernel, blocks(count), dim3(256), 0, 0, w.d, count);
  HIPC(hipMemcpy(states, w.d, count * 12 * sizeof(u64), hipMemcpyDeviceToHost));
  return SBN_OK;
}

extern "C" int sbn_poseidon_permute_coop_batch(uint64_t* states, size_t count) {
  if (!states) return fail(SBN_ERR_BAD_ARG, "null argument");
  for (size_t i = 0; i < count * 12; i++) if (states[i] >= GLP) return fail(SBN_ERR_NON_CANONICAL, "state word %zu is not canonical", i);
  if (int rc = use_current_device("no CPU fallback")) return rc;
  if (count == 0) return SBN_OK;
  DevWords w;
  if (int rc = w.alloc(count * 12)) return rc;
  HIPC(hipMemcpy(w.d, states, count * 12 * sizeof(u64), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(poseidon_coop_batch_kernel, blocks(count * 16), dim3(256), 0, 0, w.d, count);
  HIPC(hipMemcpy(states, w.d, count * 12 * sizeof(u64), hipMemcpyDeviceToHost));
  return SBN_OK;
}

extern "C" int sbn_field_mul_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, int mode) {
  if (!a || !b || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (int rc = use_current_device("no CPU fallback")) return rc;
  if (count == 0) return SBN_OK;
  DevWords w;
  if (int rc = w.alloc(3 * count)) return rc;
  u64* const d = w.d;
  HIPC(hipMemcpy(d, a, count * sizeof(u64), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d + count, b, count * sizeof(u64), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(field_mul_batch_kernel, blocks(count), dim3(256), 0, 0, d, d + count, d + 2 * count, count, mode);
  HIPC(hipMemcpy(out, d + 2 * count, count * sizeof(u64), hipMemcpyDeviceToHost));
  return SBN_OK;
}

// The shape-constant columns [*first_out, *end_out) of a table (host_common.hpp fixed_columns_range; 0, 0: none).  No device involved.
extern "C" int sbn_fixed_columns_range(const sbn_air_desc* air, uint32_t* first_out, uint32_t* end_out) {
  if (!air || !first_out || !end_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  AirShape as;
  if (!air_shape(air, nullptr, as)) return fail(SBN_ERR_BAD_ARG, "unknown air kind / num_io");
  size_t f0, f1;
  fixed_columns_range(as, f0, f1);
  *first_out = (uint32_t)f0; *end_out = (uint32_t)f1;
  return SBN_OK;
}
// The comparison behind sbn_prover_load_trace as a building block (host in, host out): `block` = those columns of a trace of
// 2^degree_bits rows; *match_out = 1 when every word is the one the generators write, else 0.
extern "C" int sbn_fixed_columns_check(const sbn_air_desc* air, uint32_t degree_bits, const uint64_t* block, int* match_out) {
  if (!air || !block || !match_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  *match_out = 0;
  AirShape as;
  if (!air_shape(air, nullptr, as)) return fail(SBN_ERR_BAD_ARG, "unknown air kind / num_io");
  size_t f0, f1;
  fixed_columns_range(as, f0, f1);
  if (f1 <= f0) return fail(SBN_ERR_UNSUPPORTED, "this table has no shape-constant columns");
  if (degree_bits > SBN_MAX_LDE_BITS || (exp_rows_per_instance(as.kind) * as.num_io) != ((size_t)1 << degree_bits))
    return fail(SBN_ERR_BAD_ARG, "the Exp tables need 512*num_io rows (FQ12_EXP_U64: 128*num_io)");
  if (int rc = use_current_device("no CPU fallback")) return rc;
  const size_t n = (size_t)1 << degree_bits, words = (f1 - f0) * n;
  DevWords w;   // d[0]: the mismatch word; the block from d + 2
  if (int rc = w.alloc(2 + words)) return rc;
  HIPC(hipMemcpy(w.d + 2, block, words * sizeof(u64), hipMemcpyHostToDevice));
  if (int rc = launch_fixed_columns_check(w.d + 2, f1 - f0, n, exp_shape(as), (unsigned long long*)w.d, 0)) return rc;
  unsigned long long mismatch = 1;
  HIPC(hipMemcpy(&mismatch, w.d, sizeof mismatch, hipMemcpyDeviceToHost));
  *match_out = mismatch == 0;
  return SBN_OK;
}

// The transcript's host permutation (sparse partial rounds) or, with use_definition != 0, the plain round-by-round
// form it must agree with.  No device involved: this is the Fiat-Shamir hasher of prove() / verify().
extern "C" int sbn_poseidon_permute_host(uint64_t* states, size_t count, int use_definition) {
  if (!states) return fail(SBN_ERR_BAD_ARG, "null argument");
  for (size_t i = 0; i < count * 12; i++) if (states[i] >= GLP) return fail(SBN_ERR_NON_CANONICAL, "state word %zu is not canonical", i);
  for (size_t k = 0; k < count; k++) {
    F st[12];
    for (int i = 0; i < 12; i++) st[i] = F(states[12 * k + i]);
    if (use_definition) poseidon_permute_generic(st); else poseidon_permute(st);
    for (int i = 0; i < 12; i++) states[12 * k + i] = st[i].v;
  }
  return SBN_OK;
}

extern "C" int sbn_set_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(SBN_ERR_NO_DEVICE, "device %d not available", device);
  HIPC(hipSetDevice(device));
  t_device = device; g_default_device.store(device);
  return SBN_OK;
}
extern "C" int sbn_set_thread_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(SBN_ERR_NO_DEVICE, "device %d not available", device);
  HIPC(hipSetDevice(device));
  t_device = device;
  return SBN_OK;
}
// The resolved switches of a prover as one line of key=value pairs (settings.hpp): what bench.py prints into `config`.
extern "C" int sbn_prover_describe(const sbn_prover* P, char* out, size_t cap) {
  if (!P || !out || cap == 0) return fail(SBN_ERR_BAD_ARG, "null argument");
  const Settings& s = P->set;
  static const char* const CH[] = {"host_pool", "device_lane", "device_wave"};
  const char* chain = P->chain_mode == 0 && tracegen_host_chains_vectorized() ? "host_pool_ifma_x8" : CH[P->chain_mode < 0 || P->chain_mode > 2 ? 0 : P->chain_mode];
  char buf[1024];
  snprintf(buf, sizeof buf,
           "abi=%d device=%d dev_bytes=%zu ntt_chunk=%zu ntt_fused=%d ntt_streams=%d ntt_split1024=%d ntt_lde_zero_aware=%d "
           "curve_chains=%s host_threads=%u fq12_host_chain=%d fq12_row_kernel=%d range_check=%d quotient_lookups=%d comm_timeout_s=%g experimental=%d lde=%s lde_ring=%u lde_ring_bytes=%zu "
           "fixed_columns=%d fixed_columns_range=%zu:%zu fixed_columns_skipped=%zu perm_diff_routes=%zu:%zu:%zu guard=%s guard_bytes=%zu ignored=[%s]",
           SBN_ABI_VERSION, P->device, P->dev_bytes, P->ntt_chunk, (int)(P->ntt_fused || P->ntt_fused512), P->ntt_two_streams ? 2 : 1, P->d_shift_odd ? 1 : 0, P->d_shift_za ? 1 : 0,
           chain, tracegen_host_threads(), (int)s.fq12_host_chain,
           (int)s.fq12_row_kernel, s.range_check, s.quotient_lookups, s.comm_timeout_s, (int)s.experimental, P->lde_storage == SBN_LDE_COMPACT ? "compact" : "full", P->ring_depth,
           P->d_ring ? (size_t)P->ring_depth * P->ntt_chunk * P->m * sizeof(u64) : (size_t)0,
           // the switch; the columns whose transforms this context keeps between proofs (0:0 none); how many the last prove() left untransformed
           (int)s.fixed_columns, P->fixed_f0, P->fixed_f1, P->fixed_skipped,
           // pairs of the last sbn_prover_explain_permutations by route: bins alone, overflow list, downloaded columns (perm_diff.hip)
           P->permdiff_routes[0], P->permdiff_routes[1], P->permdiff_routes[2],
           // verified proving (sbn_prover_set_guard): the mode, and the device bytes of the guard's verifier (outside dev_bytes)
           P->guard_mode == SBN_GUARD_DEVICE ? "device" : P->guard_mode == SBN_GUARD_HOST ? "host" : "off", guard_device_bytes(P), s.ignored.c_str());
  snprintf(out, cap, "%s", buf);
  return SBN_OK;
}
extern "C" int sbn_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }

// ---- oversized-trace split: C ABI (include/sbn.h) -----------------------------------------------------------------------
struct sbn_split_prover { sbn_prover* P; };
extern "C" int sbn_split_exchange_bytes(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, uint32_t world, uint64_t* send_bytes,
                                        uint64_t* recv_bytes) {
  if (!air || !cfg || !send_bytes || !recv_bytes || world == 0) return fail(SBN_ERR_BAD_ARG, "null argument");
  AirShape as;
  if (!air_shape(air, cfg, as)) return fail(SBN_ERR_BAD_ARG, "unknown air kind / num_io");
  if (cfg->rate_bits != 1) return fail(SBN_ERR_UNSUPPORTED, "the split prover covers rate_bits = 1 only");
  size_t sw;
  return split_sizes(as, degree_bits, cfg->rate_bits, world, SPLIT_BLOCK, send_bytes, recv_bytes, &sw, nullptr);
}
extern "C" int sbn_split_prover_create(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, const sbn_comm* comm, sbn_split_prover** out) {
  if (!out || !comm) return fail(SBN_ERR_BAD_ARG, "null argument");
  *out = nullptr;
  sbn_prover* P = nullptr;
  int rc = create_ctx(air, cfg, degree_bits, comm, nullptr, &P);
  if (rc) return rc;
  *out = new sbn_split_prover{P};
  return SBN_OK;
}
extern "C" void sbn_split_prover_destroy(sbn_split_prover* sp) {
  if (!sp) return;
  sbn_prover_destroy(sp->P);
  delete sp;
}
extern "C" int sbn_split_prover_generate_trace(sbn_split_prover* sp, const uint32_t* ios, size_t num_io, uint64_t* pi_out) {
  if (!sp) return fail(SBN_ERR_BAD_ARG, "null argument");
  return sbn_prover_generate_trace(sp->P, ios, num_io, pi_out);
}
extern "C" int sbn_split_prover_load_trace(sbn_split_prover* sp, const uint64_t* trace, const uint64_t* pi, size_t n_pi) {
  if (!sp) return fail(SBN_ERR_BAD_ARG, "null argument");
  return sbn_prover_load_trace(sp->P, trace, pi, n_pi);
}
extern "C" int sbn_split_prover_prove(sbn_split_prover* sp, sbn_proof** out) {
  if (!sp) return fail(SBN_ERR_BAD_ARG, "null argument");
  return sbn_prover_prove(sp->P, out);
}
extern "C" int sbn_split_prover_set_guard(sbn_split_prover* sp, uint32_t mode) {
  if (!sp) return fail(SBN_ERR_BAD_ARG, "null argument");
  return sbn_prover_set_guard(sp->P, mode);   // (guard.hip refuses the context of a split prover behind the mode check)
}
extern "C" int sbn_split_prover_check_trace(sbn_split_prover* sp, uint64_t seed, sbn_trace_report* rep, uint8_t* row_flags_out) {
  if (!sp) return fail(SBN_ERR_BAD_ARG, "null argument");
  return sbn_prover_check_trace(sp->P, seed, rep, row_flags_out);   // (trace_check.hip refuses world > 1)
}
extern "C" int sbn_split_prover_explain_rows(sbn_split_prover* sp, uint64_t seed, const uint64_t* rows, size_t n_rows, uint8_t* block_flags_out, uint8_t* z_flags_out) {
  if (!sp) return fail(SBN_ERR_BAD_ARG, "null argument");
  return sbn_prover_explain_rows(sp->P, seed, rows, n_rows, block_flags_out, z_flags_out);   // (trace_explain.hip refuses world > 1)
}
extern "C" int sbn_split_prover_explain_trace(sbn_split_prover* sp, uint64_t seed, sbn_block_stat* block_stats_out, sbn_block_stat* z_stats_out) {
  if (!sp) return fail(SBN_ERR_BAD_ARG, "null argument");
  return sbn_prover_explain_trace(sp->P, seed, block_stats_out, z_stats_out);
}
extern "C" int sbn_split_prover_stage_times(const sbn_split_prover* sp, float* ms_out, int cap) {
  if (!sp) return 0;
  return sbn_prover_stage_times(sp->P, ms_out, cap);
}
