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
// The host forms of explain (sbn_air_constraint_blocks, sbn_explain_rows_host, sbn_explain_trace_host) follow at the end: the same
// argument checks, challenges and Z, the evaluators through the recording consumer of air_record.cuh (device form: trace_explain.hip).
#include "prover_ctx.hpp"
#include "kernels_quotient.cuh"
#include "air_record.cuh"
#include <atomic>

static const char* SEGMENT_NAMES[QSEG] = {"air_head", "air_tail", "perm_lo", "perm_hi"};
extern "C" const char* sbn_trace_segment_name(int s) { return (s >= 0 && s < (int)QSEG) ? SEGMENT_NAMES[s] : ""; }

// The challenges of a check: the transcript observes a tag, the seed, the table and the public inputs, then hands out the
// permutation sets (tables with Z columns only) as stage_perm_z draws them and the alphas as stage_quotient_eval does (prover.hip).
void check_challenges(const AirShape& as, u32 degree_bits, const u64* pi, size_t n_pi, u64 seed, F& gamma0, F& gamma1, F alphas[SBN_NCH]) {
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

// ---- device form ------------------------------------------------------------------------------------------------------------
// Points and Lagrange selectors of the trace domain: x_i = g^i, L_first = [i == 0], L_last = [i == n - 1].
__global__ void trace_domain_tables_kernel(u64* xs, u64* lag_first, u64* lag_last, size_t n, u32 degree_bits) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  xs[i] = f_pow(f_root_of_unity(degree_bits), (u64)i).v;
  lag_first[i] = i == 0 ? 1 : 0;
  lag_last[i] = i == n - 1 ? 1 : 0;
}

void launch_trace_domain_tables(u64* xs, u64* lag_first, u64* lag_last, size_t n, u32 degree_bits, hipStream_t s) {
  hipLaunchKernelGGL(trace_domain_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, xs, lag_first, lag_last, n, degree_bits);
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
  if (P->sp && P->sp->comm.world > 1) return fail(SBN_ERR_UNSUPPORTED, "the trace check runs on single-GPU provers (this one is rank %u of %u)", P->sp->comm.rank, P->sp->comm.world);
  if (!P->loaded) return fail(SBN_ERR_BAD_ARG, "no trace loaded");
  HIPC(hipSetDevice(P->device));
  hipStream_t st = P->stream;
  const size_t n = P->n, Z = P->air.nzs;
  auto blocks = [](size_t k) { return dim3((unsigned)((k + 255) / 256)); };
  int rc;
  F gamma0, gamma1, alphas[SBN_NCH];
  check_challenges(P->air, P->degree_bits, P->pi.data(), P->pi.size(), seed, gamma0, gamma1, alphas);
  // scratch that only a running prove() owns: [xs | L_first | L_last | flag bytes] in the four planes of d_zpow, the report block in d_open
  u64 *xs = P->d_zpow, *lag_first = P->d_zpow + n, *lag_last = P->d_zpow + 2 * n;
  unsigned char* d_flags = (unsigned char*)(P->d_zpow + 3 * n);
  unsigned long long* d_blk = (unsigned long long*)P->d_open;   // (C + Z + 4) * 4 >= 24 words
  hipEvent_t* ev = P->ev;                                        // the stage events are idle outside prove()

  // Z on H: the permutation stage's own kernels into d_zval (a one-rank split context keeps its pairs in local order)
  HIPC(hipEventRecord(ev[0], st));
  if (Z) launch_perm_z(P, P->sp ? P->sp->d_pairs_own : P->d_pairs, Z, gamma0.v, gamma1.v, P->d_zval, st);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(ev[1], st));

  // tables of H, the alpha powers, then the constraint kernels on the trace rows
  hipLaunchKernelGGL(trace_domain_tables_kernel, blocks(n), dim3(256), 0, st, xs, lag_first, lag_last, n, P->degree_bits);
  HIPC(hipGetLastError());
  if ((rc = upload_alpha_tables(P, alphas))) return rc;
  QuotientParams qp{};
  qp.lde = qp.lde_next = P->d_trace; qp.zlde = qp.zlde_next = P->d_zval; qp.m = n; qp.lde_stride = n; qp.row_log = 0; qp.next_step = 1;
  qp.row_shift = 0; qp.row_rho = 0;
  qp.xs = xs; qp.lag_first = lag_first; qp.lag_last = lag_last;
  qp.last = f_inv(f_root_of_unity(P->degree_bits)).v;
  quotient_segments(P, alphas, qp);
  qp.lookups_in_perm = 0;   // the segments of the report are the default ones whatever SBN_QUOTIENT_LOOKUPS says
  qp.gamma0 = gamma0.v; qp.gamma1 = gamma1.v; qp.qout = nullptr;
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
  hipLaunchKernelGGL(trace_check_reduce_kernel, blocks(n), dim3(256), 0, st, P->d_part, n, d_flags, d_blk);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(ev[3], st));
  HIPC(hipMemcpyAsync(P->h_open, d_blk, 2 * CHK_VALS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPC(hipEventRecord(ev[4], st));
  HIPC(hipStreamSynchronize(st));
  if (row_flags_out) HIPC(hipMemcpy(row_flags_out, d_flags, n, hipMemcpyDeviceToHost));   // the caller's memory is pageable: a plain copy, as read_trace
  for (int k = 0; k < 4; k++) HIPC(hipEventElapsedTime(&P->check_ms[k], ev[k], ev[k + 1]));

  report_init(rep, n, P->air);
  const u64* blk = P->h_open;
  for (u32 s = 0; s < QSEG; s++) { rep->seg_failing_rows[s] = blk[s]; rep->seg_first_row[s] = blk[CHK_VALS + s]; }
  rep->failing_rows = blk[QSEG]; rep->first_failing_row = blk[CHK_VALS + QSEG];
  return SBN_OK;
}

extern "C" int sbn_prover_check_times(const sbn_prover* P, float* ms, int cap) {
  if (!P || !ms) return 0;
  const int k = std::min(cap, 4);
  for (int i = 0; i < k; i++) ms[i] = P->check_ms[i];
  return k;
}

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
struct HostCheck {
  AirShape as; size_t n; u32 degree_bits;
  const u64* trace; const u64* zval;   // [ncols][n], [nzs][n]
  F gamma0, gamma1, alpha[SBN_NCH];
  const F* apow[SBN_NCH];
  const ExpPiConsts<F>* pic;
  int seg_count[QSEG]; int zsplit;
  uint8_t* flags;
};
static constexpr size_t TILE = 64;

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
    constexpr int E = KIND == 4 ? 12 : (KIND == 6 ? 13 : (KIND == 3 ? 2 : (KIND == 5 ? 0 : 1)));
    const ExpShape sh(E, num_io);
    if (seg < 2) exp_eval<E>(cs, row, sh, hc.pic, 1 + (int)seg);
    else permutation_checks(cs, row, zrow, sh, num_zs, hc.gamma0, hc.gamma1, z0, z1);
  }
  return cs.result(0).v != 0 || cs.result(1).v != 0;   // host arithmetic is canonical
}

template <int KIND>
static void check_tile(const HostCheck& hc, size_t t) {
  const size_t n = hc.n, C = hc.as.ncols, Z = hc.as.nzs, r0 = t * TILE;
  std::vector<u64> rows((TILE + 1) * C), zrows((TILE + 1) * std::max<size_t>(Z, 1));
  const size_t wrap = (r0 + TILE) & (n - 1);   // the row after the tile's last
  for (size_t c = 0; c < C; c++) {
    const u64* col = hc.trace + c * n;
    for (size_t r = 0; r < TILE; r++) rows[r * C + c] = col[r0 + r];
    rows[TILE * C + c] = col[wrap];
  }
  for (size_t z = 0; z < Z; z++) {
    const u64* col = hc.zval + z * n;
    for (size_t r = 0; r < TILE; r++) zrows[r * Z + z] = col[r0 + r];
    zrows[TILE * Z + z] = col[wrap];
  }
  const F g = f_root_of_unity(hc.degree_bits), last = f_inv(g);
  F x = f_pow(g, (u64)r0);
  for (size_t r = 0; r < TILE; r++, x = x * g) {
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

// What a host form owns while it runs: the alpha powers, the public-input constants of the Exp tables, the Z columns.
struct HostStore { std::vector<F> apow[SBN_NCH]; std::vector<ExpPiConsts<F>> pic; std::vector<u64> zval; };
// Shared with perm_diff.hip (prover_ctx.hpp).  Tables and heights as sbn_prover_create accepts them:
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
static int host_setup(const sbn_air_desc* air, const uint64_t* trace, uint32_t degree_bits, const uint64_t* pi, size_t n_pi, uint64_t seed,
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
    if (as.kind == SBN_AIR_G1_OP) G1OpShape::pair((int)z, l, r);
    else if (as.kind == SBN_AIR_LOOKUP) LookupShape().pair((int)z, l, r);
    else if (is_op_air(as.kind)) OpShape(as.kind).pair((int)z, l, r);
    else exp_shape(as).pair((int)z, l, r);
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
  switch (as.kind) {
    case SBN_AIR_G1_OP: tile = check_tile<1>; break;
    case SBN_AIR_G1_EXP: tile = check_tile<2>; break;
    case SBN_AIR_G2_EXP: tile = check_tile<3>; break;
    case SBN_AIR_FQ12_EXP: tile = check_tile<4>; break;
    case SBN_AIR_FQ_EXP: tile = check_tile<5>; break;
    case SBN_AIR_FQ12_EXP_U64: tile = check_tile<6>; break;
    case SBN_AIR_MODULAR: tile = check_tile<7>; break;
    case SBN_AIR_FQ12_MUL: tile = check_tile<8>; break;
    case SBN_AIR_LOOKUP: tile = check_tile<9>; break;
    case SBN_AIR_FLAGS: tile = check_tile<10>; break;
    default: tile = check_tile<11>; break;
  }
  host_parallel_for(n / TILE, [&](size_t t) { tile(hc, t); });
  report_init(rep, n, as);
  for (size_t i = 0; i < n; i++) {
    const uint8_t f = hc.flags[i];
    if (!f) continue;
    if (!rep->failing_rows++) rep->first_failing_row = i;
    for (u32 s = 0; s < QSEG; s++) if ((f >> s) & 1) { if (!rep->seg_failing_rows[s]++) rep->seg_first_row[s] = i; }
  }
  return SBN_OK;
}

// ---- explain: which constraint BLOCKS a row breaks (include/sbn.h, sbn_explain_*) -------------------------------------------
// The recording consumer of air_record.cuh over host rows.  The block table is RECORDED, not counted by hand: the evaluator of
// the table runs once over a zero row and leaves the constraint count of every emission; what each emission is (section,
// instance, columns) is attached from the table's Shape by walking the evaluator's sections in their order, and a walk whose
// length differs from the recorded one is an error, not a table.
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

void air_pair(const AirShape& as, size_t z, int& l, int& r) {
  if (as.kind == SBN_AIR_G1_OP) G1OpShape::pair((int)z, l, r);
  else if (as.kind == SBN_AIR_LOOKUP) LookupShape().pair((int)z, l, r);
  else if (is_op_air(as.kind)) OpShape(as.kind).pair((int)z, l, r);
  else exp_shape(as).pair((int)z, l, r);
}
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
  switch (kind) {
    case SBN_AIR_G1_OP: record_row<1>(cs, row, num_io, ncons, pic); break;
    case SBN_AIR_G1_EXP: record_row<2>(cs, row, num_io, ncons, pic); break;
    case SBN_AIR_G2_EXP: record_row<3>(cs, row, num_io, ncons, pic); break;
    case SBN_AIR_FQ12_EXP: record_row<4>(cs, row, num_io, ncons, pic); break;
    case SBN_AIR_FQ_EXP: record_row<5>(cs, row, num_io, ncons, pic); break;
    case SBN_AIR_FQ12_EXP_U64: record_row<6>(cs, row, num_io, ncons, pic); break;
    case SBN_AIR_MODULAR: record_row<7>(cs, row, num_io, ncons, pic); break;
    case SBN_AIR_FQ12_MUL: record_row<8>(cs, row, num_io, ncons, pic); break;
    case SBN_AIR_LOOKUP: record_row<9>(cs, row, num_io, ncons, pic); break;
    case SBN_AIR_FLAGS: record_row<10>(cs, row, num_io, ncons, pic); break;
    default: record_row<11>(cs, row, num_io, ncons, pic); break;
  }
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
      air_pair(hc.as, z, lc, rc);
      const F lv(row.lv[lc]), rv(row.lv[rc]);
      const F t = F(zn[z]) * ((rv + hc.gamma0) * (rv + hc.gamma1)) - F(zl[z]) * ((lv + hc.gamma0) * (lv + hc.gamma1));
      const F f = (F(zl[z]) - one) * l_first;
      if (t.v != 0 || f.v != 0) zb[z >> 3] |= (uint8_t)(1u << (z & 7));
    }
    sink(i, bb.data(), zb.data());
  }
}
static int explain_args(const sbn_air_desc* air, const uint64_t* trace) {
  if (!air || !trace) return fail(SBN_ERR_BAD_ARG, "null argument");
  return SBN_OK;
}
}  // namespace

extern "C" int sbn_explain_rows_host(const sbn_air_desc* air, const uint64_t* trace, uint32_t degree_bits, const uint64_t* pi, size_t n_pi,
                                     uint64_t seed, const uint64_t* rows, size_t n_rows, uint8_t* block_flags_out, uint8_t* z_flags_out) {
  if (int rc = explain_args(air, trace)) return rc;
  if (n_rows && (!rows || !block_flags_out)) return fail(SBN_ERR_BAD_ARG, "null argument");
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
  if (int rc = explain_args(air, trace)) return rc;
  if (!block_stats_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  HostCheck hc{};
  HostStore hs;
  if (int rc = host_setup(air, trace, degree_bits, pi, n_pi, seed, hc, hs)) return rc;
  std::vector<sbn_constraint_block> blocks;
  if (int rc = block_table(hc.as, blocks)) return rc;
  const size_t B = blocks.size(), Z = hc.as.nzs, tiles = hc.n / TILE;
  // failing rows per tile and block, summed in tile order afterwards: the first row of a block is its first tile's
  std::vector<std::vector<std::pair<u32, u64>>> hits(tiles);   // (index: block b, or B + z; row), rows ascending inside a tile
  host_parallel_for(tiles, [&](size_t t) {
    explain_span(hc, B, t * TILE, TILE, [&](size_t i, const uint8_t* bb, const uint8_t* zb) {
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
