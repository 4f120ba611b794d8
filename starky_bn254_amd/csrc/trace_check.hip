// Trace check (include/sbn.h, sbn_prover_check_trace / sbn_check_trace_host): every constraint of the table evaluated on the
// TRACE domain H, row i against row i + 1 mod N, and the rows on which a segment's accumulators are non-zero reported -- what
// starky's `check_constraints` does inside a debug-build prove() ([DEP-RECALL]).
//
// Device form: nothing of the constraint code is new.  quotient_kernel<KIND, PART> (quotient.hip) reads its rows through
// QuotientParams, so pointed at d_trace / d_zval with m = n, next_step = 1 and the selector tables of H instead of the coset's
// it evaluates the four segments per trace row and leaves their accumulators in d_part; one reduction kernel turns the eight
// planes into a flag byte per row and a count and a first row per segment.  Scratch: the tables of H and the flag bytes sit in
// d_zpow (the opening stage's power tables, rebuilt by every prove()), the report block in d_open: a context that never checks
// allocates nothing for it.
// Host form: the same templates of air.cuh over F on host threads, segment by segment; Z as the running product with one
// batched inversion per column.  Both forms draw their challenges from the same transcript, so they give the same report.
// Also here, because the check was their first user: the way into a device diagnostic and the TraceDomain setup that explain shares
// (prover_ctx.hpp), and the setup of the host forms (trace_host.hpp) that explain and the permutation explain share.
#include "prover_ctx.hpp"
#include "trace_host.hpp"
#include "kernels_quotient.cuh"
#include <atomic>

static const char* SEGMENT_NAMES[QSEG] = {"air_head", "air_tail", "perm_lo", "perm_hi"};
extern "C" const char* sbn_trace_segment_name(int s) { return (s >= 0 && s < (int)QSEG) ? SEGMENT_NAMES[s] : ""; }

// The challenges of a check: the transcript observes a tag, the seed, the table and the public inputs, then hands out the
// permutation sets (tables with Z columns only) as stage_perm_z draws them and the alphas as stage_quotient_eval does (prover.hip).
static void check_challenges(const AirShape& as, u32 degree_bits, const u64* pi, size_t n_pi, u64 seed, F& gamma0, F& gamma1, F alphas[SBN_NCH]) {
  Challenger ch;
  ch.observe(F(0x4b4843544e4253ULL));   // "SBNTCHK"
  ch.observe(F(seed & 0xffffffffULL)); ch.observe(F(seed >> 32));   // (a seed may be any 64-bit value, a field element may not)
  ch.observe(F((u64)as.kind)); ch.observe(F((u64)as.num_io)); ch.observe(F((u64)degree_bits));
  for (size_t i = 0; i < n_pi; i++) ch.observe(F(pi[i]));
  F gam[2][2] = {};
  if (as.nzs) for (int s = 0; s < 2; s++) for (int c = 0; c < SBN_NCH; c++) { (void)ch.challenge(); gam[s][c] = ch.challenge(); }
  gamma0 = gam[0][0]; gamma1 = gam[1][1];
  for (int j = 0; j < SBN_NCH; j++) alphas[j] = ch.challenge();
}

static void report_init(sbn_trace_report* rep, size_t n, const AirShape& as) {
  rep->num_segments = QSEG; rep->rows = n; rep->failing_rows = 0; rep->first_failing_row = UINT64_MAX;
  for (u32 s = 0; s < QSEG; s++) { rep->seg_failing_rows[s] = 0; rep->seg_first_row[s] = UINT64_MAX; }
  rep->num_zs = (uint32_t)as.nzs; rep->z_split = (uint32_t)(as.nzs / 2);
}

// ---- the way into a device diagnostic (prover_ctx.hpp) ------------------------------------------------------------------------
int diag_refuse_split(const sbn_prover* P, const char* what, bool any_split) {
  if (P->sp && (any_split || P->sp->comm.world > 1)) return fail(SBN_ERR_UNSUPPORTED, "%s runs on single-GPU provers (this one is rank %u of %u)", what, P->sp->comm.rank, P->sp->comm.world);
  return SBN_OK;
}
int diag_enter(sbn_prover* P, const char* what, bool any_split) {
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (int rc = diag_refuse_split(P, what, any_split)) return rc;
  if (!P->loaded) return fail(SBN_ERR_BAD_ARG, "no trace loaded");
  HIPC(hipSetDevice(P->device));
  return SBN_OK;
}

// ---- device form ------------------------------------------------------------------------------------------------------------
// Points and Lagrange selectors of the trace domain: x_i = g^i, L_first = [i == 0], L_last = [i == n - 1].
__global__ void trace_domain_tables_kernel(u64* xs, u64* lag_first, u64* lag_last, size_t n, u32 degree_bits) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  xs[i] = f_pow(f_root_of_unity(degree_bits), (u64)i).v;
  lag_first[i] = i == 0 ? 1 : 0;
  lag_last[i] = i == n - 1 ? 1 : 0;
}

int trace_domain_setup(sbn_prover* P, uint64_t seed, TraceDomain& td) {
  hipStream_t st = P->stream;
  const size_t n = P->n, Z = P->air.nzs;
  check_challenges(P->air, P->degree_bits, P->pi.data(), P->pi.size(), seed, td.gamma0, td.gamma1, td.alphas);
  // Z on H: the permutation stage's own kernels into d_zval (a one-rank split context keeps its pairs in local order)
  HIPC(hipEventRecord(P->ev[0], st));
  if (Z) launch_perm_z(P, P->sp ? P->sp->d_pairs_own : P->d_pairs, Z, td.gamma0.v, td.gamma1.v, P->d_zval, st);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(P->ev[1], st));
  // the tables of H in the first three planes of d_zpow (scratch that only a running prove() owns), then the alpha powers
  u64 *xs = P->d_zpow, *lag_first = P->d_zpow + n, *lag_last = P->d_zpow + 2 * n;
  hipLaunchKernelGGL(trace_domain_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, xs, lag_first, lag_last, n, P->degree_bits);
  HIPC(hipGetLastError());
  if (int rc = upload_alpha_tables(P, td.alphas)) return rc;
  td.xs = xs; td.lag_first = lag_first; td.lag_last = lag_last;
  td.last = f_inv(f_root_of_unity(P->degree_bits)).v;
  return SBN_OK;
}

// part: [QSEG][SBN_NCH][n] accumulators.  flags[i] bit s = segment s is non-zero on row i; blk[0 .. QSEG) = failing rows per segment,
// blk[QSEG] = rows with any flag, blk[QSEG + 1 ..] = the smallest such row of each (all ones: none; the caller initialises the block).
// The accumulator words are the kernels' weak representatives (air.cuh Acc<F>::value ends in canonical operators today, but
// nothing promises it): zero is 0 or p.  Two-level: wave ballots, the four waves of a workgroup through LDS, then one atomic per
// value and workgroup.
static constexpr u32 CHK_VALS = QSEG + 1;
__global__ __launch_bounds__(256) void trace_check_reduce_kernel(const u64* __restrict__ part, size_t n, unsigned char* __restrict__ flags,
                                                                 unsigned long long* __restrict__ blk) {
  __shared__ u32 wcnt[4][CHK_VALS];
  __shared__ unsigned long long wmin[4][CHK_VALS];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  u32 f = 0;
  if (i < n) {
#pragma unroll
    for (u32 s = 0; s < QSEG; s++) {
      bool nz = false;
#pragma unroll
      for (int j = 0; j < SBN_NCH; j++) { const u64 v = part[((size_t)s * SBN_NCH + j) * n + i]; nz = nz || !(v == 0 || v == GLP); }
      f |= nz ? 1u << s : 0u;
    }
    flags[i] = (unsigned char)f;
  }
  const size_t wave_row0 = (size_t)blockIdx.x * blockDim.x + (size_t)wv * 64;
#pragma unroll
  for (u32 k = 0; k < CHK_VALS; k++) {
    const bool on = k < QSEG ? ((f >> k) & 1u) != 0 : f != 0;
    const unsigned long long b = __ballot(on);
    if (lane == 0) { wcnt[wv][k] = (u32)__popcll(b); wmin[wv][k] = b ? wave_row0 + (size_t)(__ffsll((long long)b) - 1) : ~0ull; }
  }
  __syncthreads();
  if (threadIdx.x < CHK_VALS) {
    const u32 k = threadIdx.x;
    u32 c = 0; unsigned long long mn = ~0ull;
    for (int w = 0; w < 4; w++) { c += wcnt[w][k]; mn = wmin[w][k] < mn ? wmin[w][k] : mn; }
    if (c) { atomicAdd(&blk[k], (unsigned long long)c); atomicMin(&blk[CHK_VALS + k], mn); }
  }
}

extern "C" int sbn_prover_check_trace(sbn_prover* P, uint64_t seed, sbn_trace_report* rep, uint8_t* row_flags_out) {
  if (!P || !rep) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (rep->struct_size != sizeof(sbn_trace_report)) return fail(SBN_ERR_BAD_ARG, "sbn_trace_report.struct_size does not match this library (ABI %d)", SBN_ABI_VERSION);
  int rc;
  if ((rc = diag_enter(P, "the trace check", false))) return rc;
  hipStream_t st = P->stream;
  hipEvent_t* ev = P->ev;
  const size_t n = P->n;
  TraceDomain td;
  if ((rc = trace_domain_setup(P, seed, td))) return rc;
  // more scratch that only a running prove() owns: the flag bytes in the fourth plane of d_zpow, the report block in d_open
  unsigned char* d_flags = (unsigned char*)(P->d_zpow + 3 * n);
  unsigned long long* d_blk = (unsigned long long*)P->d_open;   // (C + Z + 4) * 4 >= 24 words

  // the constraint kernels on the trace rows
  QuotientParams qp{};
  qp.lde = qp.lde_next = P->d_trace; qp.zlde = qp.zlde_next = P->d_zval; qp.m = n; qp.lde_stride = n; qp.row_log = 0; qp.next_step = 1;
  qp.row_shift = 0; qp.row_rho = 0;
  qp.xs = td.xs; qp.lag_first = td.lag_first; qp.lag_last = td.lag_last;
  qp.last = td.last;
  quotient_segments(P, td.alphas, qp);
  qp.lookups_in_perm = 0;   // the segments of the report are the default ones whatever SBN_QUOTIENT_LOOKUPS says
  qp.gamma0 = td.gamma0.v; qp.gamma1 = td.gamma1.v; qp.qout = nullptr;
  qp.part = P->d_part;      // QSEG x SBN_NCH planes of n words (the chunked Z above is done with it: same stream)
  HIPC(hipEventRecord(P->chunk_ready[3], st));
  HIPC(hipStreamWaitEvent(P->hstream, P->chunk_ready[3], 0));
  if ((rc = launch_quotient_parts(P, qp, (n + 255) / 256))) return rc;
  HIPC(hipEventRecord(P->hash_done, P->hstream));
  HIPC(hipStreamWaitEvent(st, P->hash_done, 0));
  HIPC(hipEventRecord(ev[2], st));

  // verdict
  HIPC(hipMemsetAsync(d_blk, 0, CHK_VALS * sizeof(unsigned long long), st));
  HIPC(hipMemsetAsync(d_blk + CHK_VALS, 0xff, CHK_VALS * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(trace_check_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P->d_part, n, d_flags, d_blk);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(ev[3], st));
  HIPC(hipMemcpyAsync(P->h_open, d_blk, 2 * CHK_VALS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPC(hipEventRecord(ev[4], st));
  HIPC(hipStreamSynchronize(st));
  if (row_flags_out) HIPC(hipMemcpy(row_flags_out, d_flags, n, hipMemcpyDeviceToHost));   // the caller's memory is pageable: a plain copy, as read_trace
  for (int k = 0; k < 4; k++) HIPC(hipEventElapsedTime(&P->diag_ms[DIAG_CHECK][k], ev[k], ev[k + 1]));

  report_init(rep, n, P->air);
  const u64* blk = P->h_open;
  for (u32 s = 0; s < QSEG; s++) { rep->seg_failing_rows[s] = blk[s]; rep->seg_first_row[s] = blk[CHK_VALS + s]; }
  rep->failing_rows = blk[QSEG]; rep->first_failing_row = blk[CHK_VALS + QSEG];
  return SBN_OK;
}

extern "C" int sbn_prover_check_times(const sbn_prover* P, float* ms, int cap) { return P ? copy_times(P->diag_ms[DIAG_CHECK], 4, ms, cap) : 0; }

// ---- host form --------------------------------------------------------------------------------------------------------------
namespace {
// rows of one tile, row-major: the trace is column-major, and a row of it is one word out of every column
struct TileRow {
  const u64* lv; const u64* nv;
  F l(int c) const { return F(lv[c]); }
  F n(int c) const { return F(nv[c]); }
};
struct TileZRow {
  const u64* lv; const u64* nv;
  F zl(int z) const { return F(lv[z]); }
  F zn(int z) const { return F(nv[z]); }
};
// One segment on one row, as quotient_kernel<KIND, PART> (quotient.hip) evaluates it, lookups with the tail segment.
template <int KIND>
static bool segment_nonzero(const HostCheck& hc, u32 seg, const TileRow& row, const TileZRow& zrow, F x, F last, F l_first, F l_last) {
  Cons<F> cs;
  for (int j = 0; j < SBN_NCH; j++) { cs.alpha[j] = hc.alpha[j]; cs.apow[j] = hc.apow[j]; }
  cs.start(hc.seg_count[seg]);
  cs.z_last = x - last; cs.l_first = l_first; cs.l_last = l_last;
  const int num_zs = (int)hc.as.nzs, num_io = (int)hc.as.num_io;
  const int z0 = seg == 2 ? 0 : hc.zsplit, z1 = seg == 2 ? hc.zsplit : num_zs;
  if (KIND == 1) {
    if (seg == 0) g1op_eval(cs, row);
    else if (seg >= 2) permutation_checks(cs, row, zrow, G1OpShape(), num_zs, hc.gamma0, hc.gamma1, z0, z1);
  } else if (KIND == 9) {
    if (seg == 0) lookup_eval(cs, row);
    else if (seg >= 2) permutation_checks(cs, row, zrow, LookupShape(), num_zs, hc.gamma0, hc.gamma1, z0, z1);
  } else if (KIND == 10) {
    if (seg == 0) flag_eval(cs, row, FlagShape(num_io));
  } else if (KIND == 11) {
    if (seg == 0) flag_u64_eval(cs, row, FlagU64Shape(num_io));
  } else if (KIND == 7 || KIND == 8) {
    const OpShape sh(KIND);
    if (seg == 0) op_eval<KIND>(cs, row, sh);
    else if (seg >= 2) permutation_checks(cs, row, zrow, sh, num_zs, hc.gamma0, hc.gamma1, z0, z1);
  } else {
    constexpr int E = air_exp_e(KIND);
    const ExpShape sh(E, num_io);
    if (seg < 2) exp_eval<E>(cs, row, sh, hc.pic, 1 + (int)seg);
    else permutation_checks(cs, row, zrow, sh, num_zs, hc.gamma0, hc.gamma1, z0, z1);
  }
  return cs.result(0).v != 0 || cs.result(1).v != 0;   // host arithmetic is canonical
}

template <int KIND>
static void check_tile(const HostCheck& hc, size_t t) {
  const size_t n = hc.n, C = hc.as.ncols, Z = hc.as.nzs, r0 = t * HOST_TILE;
  std::vector<u64> rows((HOST_TILE + 1) * C), zrows((HOST_TILE + 1) * std::max<size_t>(Z, 1));
  const size_t wrap = (r0 + HOST_TILE) & (n - 1);   // the row after the tile's last
  for (size_t c = 0; c < C; c++) {
    const u64* col = hc.trace + c * n;
    for (size_t r = 0; r < HOST_TILE; r++) rows[r * C + c] = col[r0 + r];
    rows[HOST_TILE * C + c] = col[wrap];
  }
  for (size_t z = 0; z < Z; z++) {
    const u64* col = hc.zval + z * n;
    for (size_t r = 0; r < HOST_TILE; r++) zrows[r * Z + z] = col[r0 + r];
    zrows[HOST_TILE * Z + z] = col[wrap];
  }
  const F g = f_root_of_unity(hc.degree_bits), last = f_inv(g);
  F x = f_pow(g, (u64)r0);
  for (size_t r = 0; r < HOST_TILE; r++, x = x * g) {
    const size_t i = r0 + r;
    const TileRow row{rows.data() + r * C, rows.data() + (r + 1) * C};
    const TileZRow zrow{zrows.data() + r * Z, zrows.data() + (r + 1) * Z};
    const F l_first(i == 0 ? 1 : 0), l_last(i == n - 1 ? 1 : 0);
    uint8_t f = 0;
    for (u32 seg = 0; seg < QSEG; seg++) {
      if (hc.seg_count[seg] == 0) continue;
      if (segment_nonzero<KIND>(hc, seg, row, zrow, x, last, l_first, l_last)) f |= (uint8_t)(1u << seg);
    }
    hc.flags[i] = f;
  }
}

// Z[0] = 1, Z[i + 1] = Z[i] * num_i / den_i (kernels.cuh permutation_z_kernel: prefix of num times suffix of den over the product of
// every den -- a column with a zero denominator is zero throughout there, so it is here)
static void host_perm_z(const HostCheck& hc, size_t z, int lc, int rc, u64* out) {
  const size_t n = hc.n;
  const u64 *lhs = hc.trace + (size_t)lc * n, *rhs = hc.trace + (size_t)rc * n;
  std::vector<F> pre(n);   // pre[i] = den_0 .. den_i
  F acc(1);
  for (size_t i = 0; i < n; i++) { const F r(rhs[i]); acc = acc * ((r + hc.gamma0) * (r + hc.gamma1)); pre[i] = acc; }
  if (acc.v == 0) { for (size_t i = 0; i < n; i++) out[i] = 0; return; }
  // inverses of the denominators from the top: inv = 1 / (den_0 .. den_i), so 1 / den_i = inv * pre[i - 1]
  std::vector<F> dinv(n);
  F inv = f_inv(acc);
  for (size_t i = n; i-- > 0;) {
    const F r(rhs[i]);
    dinv[i] = i ? inv * pre[i - 1] : inv;
    inv = inv * ((r + hc.gamma0) * (r + hc.gamma1));
  }
  F zc(1);
  for (size_t i = 0; i < n; i++) {
    out[i] = zc.v;
    const F l(lhs[i]);
    zc = zc * ((l + hc.gamma0) * (l + hc.gamma1)) * dinv[i];
  }
}
}  // namespace

// ---- the setup of the host forms (trace_host.hpp) ---------------------------------------------------------------------------
// Tables and heights as sbn_prover_create accepts them:
int host_table_check(const sbn_air_desc* air, uint32_t degree_bits, AirShape& as) {
  if (!air_shape(air, nullptr, as)) return fail(SBN_ERR_BAD_ARG, "unknown air kind / num_io");
  if (degree_bits < 9 || degree_bits > 22) return fail(SBN_ERR_UNSUPPORTED, "degree_bits out of range");
  const size_t n = (size_t)1 << degree_bits;
  if (as.kind == SBN_AIR_FLAGS && 512 * (size_t)as.num_io != n) return fail(SBN_ERR_BAD_ARG, "FlagStark needs 512*num_io rows");
  if (as.kind == SBN_AIR_FLAGS_U64 && 128 * (size_t)as.num_io != n) return fail(SBN_ERR_BAD_ARG, "the u64 FlagStark needs 128*num_io rows");
  if (is_exp_air(as.kind)) {
    if (exp_rows_per_instance(as.kind) * as.num_io != n) return fail(SBN_ERR_BAD_ARG, "the Exp tables need 512*num_io rows (FQ12_EXP_U64: 128*num_io)");
    if (as.kind != SBN_AIR_FQ12_EXP && as.kind != SBN_AIR_FQ12_EXP_U64 && degree_bits < 16)
      return fail(SBN_ERR_UNSUPPORTED, "G1_EXP / G2_EXP / FQ_EXP need >= 2^16 rows (u16 range check, range_check.rs:26)");
  }
  return SBN_OK;
}
// canonical form, on the pool; the smallest bad index wins
int host_canonical_check(const uint64_t* trace, size_t words) {
  const size_t pieces = std::max<size_t>(1, std::min<size_t>(words >> 16, 256)), per = (words + pieces - 1) / pieces;
  std::atomic<size_t> bad(words);
  host_parallel_for(pieces, [&](size_t t) {
    const size_t a = t * per, b = std::min(words, a + per);
    for (size_t i = a; i < b; i++) if (trace[i] >= GLP) { size_t cur = bad.load(); while (i < cur && !bad.compare_exchange_weak(cur, i)) {} break; }
  });
  if (bad.load() < words) return fail(SBN_ERR_NON_CANONICAL, "trace word %zu is not canonical", bad.load());
  return SBN_OK;
}
// The argument checks of the host forms after their own null checks (tables and heights as sbn_prover_create accepts them, canonical
// form), then the challenges, the tables and Z.
int host_setup(const sbn_air_desc* air, const uint64_t* trace, uint32_t degree_bits, const uint64_t* pi, size_t n_pi, uint64_t seed,
               HostCheck& hc, HostStore& hs) {
  AirShape& as = hc.as;
  if (int rc = host_table_check(air, degree_bits, as)) return rc;
  const size_t n = (size_t)1 << degree_bits;
  if (n_pi != as.npi) return fail(SBN_ERR_BAD_ARG, "expected %zu public inputs, got %zu", as.npi, n_pi);
  if (n_pi && !pi) return fail(SBN_ERR_BAD_ARG, "null public inputs");
  for (size_t i = 0; i < n_pi; i++) if (pi[i] >= GLP) return fail(SBN_ERR_NON_CANONICAL, "public input %zu is not canonical", i);
  const size_t C = as.ncols, Z = as.nzs, words = C * n;
  if (int rc = host_canonical_check(trace, words)) return rc;
  hc.n = n; hc.degree_bits = degree_bits; hc.trace = trace;
  check_challenges(as, degree_bits, pi, n_pi, seed, hc.gamma0, hc.gamma1, hc.alpha);
  std::vector<F>* apow = hs.apow;
  for (int j = 0; j < SBN_NCH; j++) {
    apow[j].resize(apow_len(as.nconstraints, as.nzs));
    F a(1);
    for (size_t k = 0; k < apow[j].size(); k++) { apow[j][k] = a; a = a * hc.alpha[j]; }
    hc.apow[j] = apow[j].data();
  }
  std::vector<ExpPiConsts<F>>& pic = hs.pic;
  pic.resize(is_exp_air(as.kind) ? 1 : 0);
  if (is_exp_air(as.kind)) {
    std::vector<F> pif(n_pi);
    for (size_t i = 0; i < n_pi; i++) pif[i] = F(pi[i]);
    const F* app[SBN_NCH] = {apow[0].data(), apow[1].data()};
    exp_pi_consts<F>(exp_shape(as), app, pif.data(), pic[0]);
    hc.pic = pic.data();
  }
  {  // the segments of the quotient stage (prover.hip quotient_segments)
    const size_t n_tail = is_exp_air(as.kind) ? (size_t)exp_shape(as).num_tail_constraints() : 0;
    hc.seg_count[0] = (int)(as.nconstraints - n_tail); hc.seg_count[1] = (int)n_tail;
    hc.seg_count[2] = hc.seg_count[3] = 2 * (int)Z;
    hc.zsplit = (int)(Z / 2);
  }
  std::vector<u64>& zval = hs.zval;
  zval.resize(Z * n);
  hc.zval = zval.data();
  host_parallel_for(Z, [&](size_t z) {
    int l, r;
    air_pair(as, z, l, r);
    host_perm_z(hc, z, l, r, zval.data() + z * n);
  });
  return SBN_OK;
}

extern "C" int sbn_check_trace_host(const sbn_air_desc* air, const uint64_t* trace, uint32_t degree_bits, const uint64_t* pi, size_t n_pi,
                                    uint64_t seed, sbn_trace_report* rep, uint8_t* row_flags_out) {
  if (!air || !trace || !rep) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (rep->struct_size != sizeof(sbn_trace_report)) return fail(SBN_ERR_BAD_ARG, "sbn_trace_report.struct_size does not match this library (ABI %d)", SBN_ABI_VERSION);
  HostCheck hc{};
  HostStore hs;
  if (int rc = host_setup(air, trace, degree_bits, pi, n_pi, seed, hc, hs)) return rc;
  const AirShape& as = hc.as;
  const size_t n = hc.n;
  std::vector<uint8_t> own_flags(row_flags_out ? 0 : n);
  hc.flags = row_flags_out ? row_flags_out : own_flags.data();
  void (*tile)(const HostCheck&, size_t) = nullptr;
  for_air_kind(as.kind, [&](auto K) { tile = check_tile<decltype(K)::value>; });
  host_parallel_for(n / HOST_TILE, [&](size_t t) { tile(hc, t); });
  report_init(rep, n, as);
  for (size_t i = 0; i < n; i++) {
    const uint8_t f = hc.flags[i];
    if (!f) continue;
    if (!rep->failing_rows++) rep->first_failing_row = i;
    for (u32 s = 0; s < QSEG; s++) if ((f >> s) & 1) { if (!rep->seg_failing_rows[s]++) rep->seg_first_row[s] = i; }
  }
  return SBN_OK;
}
