// On-device witness generation of the Exp tables (sbn_prover_generate_trace) and the parity hook of the BN254 field helpers
// (sbn_bn254_fq_batch): the one unit that includes kernels_tracegen.cuh, whose kernels are ordinary external definitions.
#include "prover_ctx.hpp"
#include "kernels_tracegen.cuh"
#include <atomic>
#include <cstring>

// Scratch lives in the (not yet used) LDE buffer; the only host traffic is the instance list in (20 KB) and the
// instance outputs + error word back (8 KB).
// the u16 range-check kernel keeps 156 KB in LDS (> the 64 KiB default); idempotent, see ntt_fast_setup (prover.hip)
static int range_check_setup(int device) {
  static std::atomic<bool> done[SBN_MAX_DEVICES];
  const int d = device >= 0 && device < SBN_MAX_DEVICES ? device : 0;
  if (!done[d].load()) {
    HIPC(hipFuncSetAttribute((const void*)tg::range_check_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tg::RC_LDS_BYTES));
    HIPC(hipFuncSetAttribute((const void*)tg::range_check_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tg::RC_LDS_BYTES));
    done[d].store(true);
  }
  return 0;
}
// One step of the curve chains as levels of independent micro-operations for tg::chain_coop_kernel: the formulas of
// bnw::jac_double / bnw::jac_add (bn254w.cuh) written once over builder values, Fq2 products expanded into four Fq products,
// every value in a fresh slot (no hazards), level = 1 + the deepest operand.  Program 0: a <- 2a (exponent bit clear);
// program 1: b <- b + a, a <- 2a.  Persistent slots: a.X a.Y a.Z b.X b.Y b.Z, E each, in that order from slot 0.
struct ChainProgram {
  std::vector<uint32_t> ops[2];
  int levels[2] = {0, 0};
  int slots = 0;
};
static ChainProgram build_chain_program(int E) {
  struct Op { int kind, d, a, b, level; };
  struct Val { int s[2]; };
  ChainProgram out;
  for (int bit = 0; bit < 2; bit++) {
    std::vector<int> lvl;
    std::vector<Op> ops;
    auto fresh = [&](int level) { lvl.push_back(level); return (int)lvl.size() - 1; };
    auto emit = [&](int kind, int a, int b) { const int L = 1 + std::max(lvl[a], lvl[b]); const int d = fresh(L); ops.push_back({kind, d, a, b, L}); return d; };
    auto add = [&](Val x, Val y) { Val r{}; for (int q = 0; q < E; q++) r.s[q] = emit(tg::CP_ADD, x.s[q], y.s[q]); return r; };
    auto sub = [&](Val x, Val y) { Val r{}; for (int q = 0; q < E; q++) r.s[q] = emit(tg::CP_SUB, x.s[q], y.s[q]); return r; };
    auto mul = [&](Val x, Val y) {
      Val r{};
      if (E == 1) { r.s[0] = emit(tg::CP_MUL, x.s[0], y.s[0]); return r; }
      const int t0 = emit(tg::CP_MUL, x.s[0], y.s[0]), t1 = emit(tg::CP_MUL, x.s[1], y.s[1]);
      const int t2 = emit(tg::CP_MUL, x.s[0], y.s[1]), t3 = emit(tg::CP_MUL, x.s[1], y.s[0]);
      r.s[0] = emit(tg::CP_SUB, t0, t1); r.s[1] = emit(tg::CP_ADD, t2, t3);   // Fq2 = Fq[i] / (i^2 + 1), cmul of bn254w.cuh
      return r;
    };
    auto chk_zero = [&](Val x) {   // czero: every component zero -> TG_ERR_DEGENERATE
      const int a = x.s[0], b = E == 2 ? x.s[1] : x.s[0];
      ops.push_back({E == 2 ? tg::CP_CHK2 : tg::CP_CHK1, 0, a, b, 1 + std::max(lvl[a], lvl[b])});
    };
    Val pa[3], pb[3];                                           // persistent a, b: slots 0 .. 6E-1, level 0
    for (int c = 0; c < 3; c++) for (int q = 0; q < E; q++) pa[c].s[q] = fresh(0);
    for (int c = 0; c < 3; c++) for (int q = 0; q < E; q++) pb[c].s[q] = fresh(0);
    Val nb[3] = {pb[0], pb[1], pb[2]};
    if (bit) {   // b + a: add-2007-bl, p = b, q = a (exp_chains: b = jac_add(b, a))
      const Val Z1Z1 = mul(pb[2], pb[2]), Z2Z2 = mul(pa[2], pa[2]);
      const Val U1 = mul(pb[0], Z2Z2), U2 = mul(pa[0], Z1Z1);
      const Val S1 = mul(mul(pb[1], pa[2]), Z2Z2), S2 = mul(mul(pa[1], pb[2]), Z1Z1);
      const Val H = sub(U2, U1);
      chk_zero(H);
      const Val H2 = add(H, H), I = mul(H2, H2), J = mul(H, I);
      const Val rr0 = sub(S2, S1), r = add(rr0, rr0);
      const Val V = mul(U1, I);
      nb[0] = sub(sub(mul(r, r), J), add(V, V));
      const Val sj = mul(S1, J);
      nb[1] = sub(mul(r, sub(V, nb[0])), add(sj, sj));
      const Val zs = add(pb[2], pa[2]);
      nb[2] = mul(sub(sub(mul(zs, zs), Z1Z1), Z2Z2), H);
    }
    chk_zero(pa[1]);   // exp_chains: czero(a.Y) before every doubling
    Val na[3];
    {   // 2a: dbl-2009-l
      const Val A = mul(pa[0], pa[0]), B = mul(pa[1], pa[1]), C = mul(B, B);
      const Val t0 = add(pa[0], B), t1 = mul(t0, t0), t2 = sub(sub(t1, A), C);
      const Val D = add(t2, t2), Ee = add(add(A, A), A), F = mul(Ee, Ee);
      na[0] = sub(F, add(D, D));
      const Val C2 = add(C, C), C4 = add(C2, C2), C8 = add(C4, C4);
      na[1] = sub(mul(Ee, sub(D, na[0])), C8);
      const Val yz = mul(pa[1], pa[2]);
      na[2] = add(yz, yz);
    }
    int top = 0;
    for (const Op& o : ops) top = std::max(top, o.level);
    for (int c = 0; c < 3; c++) for (int q = 0; q < E; q++) {   // the new points replace the old ones after every read
      ops.push_back({tg::CP_COPY, pa[c].s[q], na[c].s[q], na[c].s[q], top + 1});
      if (bit) ops.push_back({tg::CP_COPY, pb[c].s[q], nb[c].s[q], nb[c].s[q], top + 1});
    }
    const int nl = top + 1;
    out.levels[bit] = nl;
    out.slots = std::max(out.slots, (int)lvl.size());
    out.ops[bit].assign((size_t)nl * tg::CP_LANES, 0u);
    std::vector<int> fill(nl, 0);
    for (const Op& o : ops) {
      const int L = o.level - 1;
      if (fill[L] >= tg::CP_LANES || (int)lvl.size() > tg::CP_MAX_SLOTS) { out.levels[0] = out.levels[1] = -1; return out; }   // (cannot happen for E <= 2: checked by the caller)
      out.ops[bit][(size_t)L * tg::CP_LANES + fill[L]++] = (uint32_t)o.kind | ((uint32_t)o.d << 8) | ((uint32_t)o.a << 16) | ((uint32_t)o.b << 24);
    }
  }
  return out;
}

// ---- what the three generators share --------------------------------------------------------------------------------
static dim3 blocks(size_t k, unsigned b) { return dim3((unsigned)((k + b - 1) / b)); }

// the first `values` Fq elements of every instance (eight u32 words each) are below p
static int check_below_p(const uint32_t* ios, size_t IOW, int values, size_t K, const char* what) {
  for (size_t k = 0; k < K; k++)
    for (int v = 0; v < values; v++) {
      u64 t[4]; for (int i = 0; i < 4; i++) t[i] = (u64)ios[IOW * k + 8 * v + 2 * i] | ((u64)ios[IOW * k + 8 * v + 2 * i + 1] << 32);
      if (bnw::geq_p(t)) return fail(SBN_ERR_BAD_ARG, "%s >= p (instance %zu)", what, k);
    }
  return 0;
}

// grow-on-demand pinned staging (a copy from / to pageable memory blocks the calling thread inside the runtime, once per copy)
static int pinned_reserve(u64** buf, size_t* words, size_t need) {
  if (*words >= need) return 0;
  if (*buf) (void)hipHostFree(*buf);
  *buf = nullptr; *words = 0;
  HIPC(hipHostMalloc((void**)buf, need * sizeof(u64), hipHostMallocDefault));
  *words = need;
  return 0;
}

// sbn_prover_generate_trace_chained: the offsets are derived on the device from `terms` (instance rows without their offset words)
// and `start`; the explicit-list call passes none of this and launches what it always launched.
struct ChainedIn { const uint32_t* terms; const uint32_t* start; uint32_t* ios_out; };
// the preliminary list: every instance with the same `offset` words (xw words of x, ew of the exponent)
static std::vector<uint32_t> preliminary_list(const ChainedIn& ch, size_t K, size_t xw, size_t ew, const uint32_t* offset) {
  std::vector<uint32_t> ios((2 * xw + ew) * K);
  for (size_t k = 0; k < K; k++) {
    uint32_t* io = ios.data() + (2 * xw + ew) * k;
    memcpy(io, ch.terms + (xw + ew) * k, xw * sizeof(uint32_t));
    memcpy(io + xw, offset, xw * sizeof(uint32_t));
    memcpy(io + 2 * xw, ch.terms + (xw + ew) * k + xw, ew * sizeof(uint32_t));
  }
  return ios;
}

// sbn_prover_generate_trace_scalar_muls: every instance carries `offset`; the list is expanded on the device from the points, the
// one-or-K scalars and the offset, and the products output + (-offset) are computed there (kernels_tracegen.cuh, "independent
// scalar multiplications").  G1 / G2 only.
struct ScalarMulIn { const uint32_t* points; const uint32_t* scalars; size_t scalar_count; const uint32_t* offset; uint32_t* products_out; uint8_t* infinity_out; uint32_t* ios_out; };

// sbn_prover_generate_trace_powers: `count` towers of `depth` levels on an Fq12 table whose chains run on the device; level 0 takes
// its x from `bases`, level l from the output of level l - 1, derived on the device (kernels_tracegen.cuh, "power towers").
struct PowerIn { const uint32_t* bases; const uint32_t* exps; size_t exp_count, count, depth; uint32_t* powers_out; uint32_t* ios_out; };

// sbn_prover_generate_trace_msm_batch: one unit of `segments` chained lists, M real instances and num_io - M pads; the offsets are
// derived on the device from the terms, the heads and the starts (kernels_tracegen.cuh, "segmented chained lists"), the finals
// are the instance outputs at the segment tails and, on the curves, the sums final + (-start) are computed there too.
struct BatchIn {
  const uint32_t* terms; const uint64_t* lengths; size_t segments; const uint32_t* starts; size_t start_count, M;
  uint32_t* finals_out; uint32_t* sums_out; uint8_t* infinity_out; uint32_t* ios_out;
};
// the preliminary list of a segmented one: row g carries x and exponent of instance min(g, M - 1) and `offset_of(segment)` as its
// offset; head_of[g] = the head of the segment of that instance (optional); seg_head / seg_len: per segment
static std::vector<uint32_t> batch_preliminary_list(const BatchIn& mb, size_t K, size_t xw, size_t ew, const std::function<const uint32_t*(size_t)>& offset_of,
                                                    std::vector<uint32_t>& seg_head, std::vector<uint32_t>& seg_len, std::vector<uint32_t>* head_of) {
  std::vector<uint32_t> ios((2 * xw + ew) * K);
  seg_head.resize(mb.segments); seg_len.resize(mb.segments);
  if (head_of) head_of->resize(K);
  size_t g = 0;
  for (size_t s = 0; s < mb.segments; s++) {
    seg_head[s] = (uint32_t)g; seg_len[s] = (uint32_t)mb.lengths[s];
    for (size_t j = 0; j < mb.lengths[s]; j++, g++) {
      uint32_t* io = ios.data() + (2 * xw + ew) * g;
      memcpy(io, mb.terms + (xw + ew) * g, xw * sizeof(uint32_t));
      memcpy(io + xw, offset_of(s), xw * sizeof(uint32_t));
      memcpy(io + 2 * xw, mb.terms + (xw + ew) * g + xw, ew * sizeof(uint32_t));
      if (head_of) (*head_of)[g] = seg_head[s];
    }
  }
  for (; g < K; g++) {   // the reference's resize rule: a pad row is the last row again
    memcpy(ios.data() + (2 * xw + ew) * g, ios.data() + (2 * xw + ew) * (mb.M - 1), (2 * xw + ew) * sizeof(uint32_t));
    if (head_of) (*head_of)[g] = (uint32_t)g;   // (never read: the scan's lanes stop at M)
  }
  return ios;
}

// One sbn_prover_generate_trace call: the scratch carver, the launches every table has, the SBN_TRACE_TIMING marks and the tail.
struct TraceJob {
  sbn_prover* const P;
  const size_t K, IOW, n;   // K instances of IOW u32 words each
  const hipStream_t st;
  const ExpShape sh;
  u64* const wbase;   // scratch: the LDE buffer, not yet in use
  u64* w;
  std::vector<hipEvent_t> kev;
  TraceJob(sbn_prover* P, size_t K, size_t IOW)
      : P(P), K(K), IOW(IOW), n(P->n), st(P->stream), sh(exp_shape(P->air)), wbase(P->sp ? (u64*)P->sp->comm.recv_buf : P->d_lde), w(wbase) {}

  u64* take(size_t words) { u64* r = w; w += (words + 7) & ~(size_t)7; return r; }
  unsigned int* take_histograms() { return n > 65536 ? (unsigned int*)take((size_t)sh.num_rc * 32768) : nullptr; }   // u32 histograms of the range-checked columns
  int fits() const { return (size_t)(w - wbase) > P->lde_scratch_words ? fail(SBN_ERR_UNSUPPORTED, "scratch does not fit") : 0; }

  void mark() {
    hipEvent_t e;
    if (P->set.trace_timing && hipEventCreate(&e) == hipSuccess && hipEventRecord(e, st) == hipSuccess) kev.push_back(e);
  }
  // the timed span opens (EX_TRACEGEN_MS); the instance list goes in from `h_ios`, the caller's memory or a pinned copy of it
  // (`words`: u32 words that go up when it is not the whole list: the compact form of the scalar multiplications)
  int begin(const void* h_ios, uint32_t* d_ios, int* d_err, size_t words = 0) {
    HIPC(hipEventRecord(P->abs_ev[0], st));
    HIPC(hipMemcpyAsync(d_ios, h_ios, (words ? words : IOW * K) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPC(hipMemsetAsync(d_err, 0, sizeof(int), st));
    mark();
    return 0;
  }
  // the input-independent columns; table_max: the last entry of the lookup table (u16 tables 65535, the split check's 255)
  template <typename FlagsKernel>
  void launch_common_columns(FlagsKernel flags, const uint32_t* d_ios, u64* inv, u64 table_max) {
    hipLaunchKernelGGL(flags, blocks(n, 256), dim3(256), 0, st, d_ios, IOW, n, sh.start_flags, P->d_trace);
    hipLaunchKernelGGL(tg::small_inverse_kernel, blocks(n, 256), dim3(256), 0, st, inv, n);
    hipLaunchKernelGGL(tg::periodic_kernel, blocks(n, 256), dim3(256), 0, st, inv, n, sh.start_periodic, sh.start_io_pulses, sh.start_lookups, table_max, P->d_trace);
    hipLaunchKernelGGL(tg::io_pulse_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)(2 * K)), dim3(256), 0, st, inv, n, (size_t)sh.rpb, sh.witness_col(0), P->d_trace);
    mark();
  }
  int launch_u16_range_check(unsigned int* d_cnt, int* d_err) {
    if (n > 65536) {   // multiplicities beyond u16: histogram of every target column in HBM first (kernels_tracegen.cuh)
      HIPC(hipMemsetAsync(d_cnt, 0, (size_t)sh.num_rc * 65536 * sizeof(unsigned int), st));
      hipLaunchKernelGGL(tg::range_count_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)sh.num_rc), dim3(256), 0, st, P->d_trace, n, sh.rc_start, d_cnt, d_err);
      hipLaunchKernelGGL(tg::range_check_kernel<true>, dim3((unsigned)sh.num_rc), dim3(tg::RC_THREADS), tg::RC_LDS_BYTES, st, P->d_trace, n, sh.rc_start, sh.start_lookups, d_err, d_cnt, P->set.range_check);
    } else {
      hipLaunchKernelGGL(tg::range_check_kernel<false>, dim3((unsigned)sh.num_rc), dim3(tg::RC_THREADS), tg::RC_LDS_BYTES, st, P->d_trace, n, sh.rc_start, sh.start_lookups, d_err, (const unsigned int*)nullptr, P->set.range_check);
    }
    return 0;
  }
  // the timed span closes and the stream drains: the generator's copies back to the host, queued before this, have landed
  int end(const char* const* names) {
    HIPC(hipEventRecord(P->abs_ev[1], st));
    HIPC(hipStreamSynchronize(st));
    float ms = 0; HIPC(hipEventElapsedTime(&ms, P->abs_ev[0], P->abs_ev[1]));
    P->stage_ms[ST_COUNT + EX_TRACEGEN_MS] = ms;
    if (P->set.trace_timing) {
      for (size_t i = 0; i + 1 < kev.size(); i++) { float t = 0; (void)hipEventElapsedTime(&t, kev[i], kev[i + 1]); fprintf(stderr, "[device tracegen] %-14s %8.3f ms\n", names[i], t); }
      for (auto e : kev) (void)hipEventDestroy(e);
      fprintf(stderr, "[device tracegen] %-14s %8.3f ms\n", "total", ms);
    }
    return 0;
  }
  // the kernels' error word, a degenerate instance first; then the public inputs `pi(k, p)` writes for instance k
  template <typename PublicInputs>
  int finish(int err, uint64_t* pi_out, PublicInputs pi) {
    if (err & tg::TG_ERR_INFINITY) return fail(SBN_ERR_WITNESS, "an offset of the chained list is the point at infinity");
    if (err & tg::TG_ERR_DEGENERATE) return fail(SBN_ERR_WITNESS, "degenerate affine operation (x1 == x2 or y == 0)");
    if (err & tg::TG_ERR_WITNESS) return fail(SBN_ERR_WITNESS, "modular witness generation failed");
    if (err & tg::TG_ERR_RANGE) return fail(SBN_ERR_WITNESS, "range-checked column holds a value >= 2^16");
    P->pi.resize(P->air.npi);
    for (size_t k = 0; k < K; k++) pi(k, P->pi.data() + (size_t)sh.pi_per_io * k);
    if (pi_out) memcpy(pi_out, P->pi.data(), P->pi.size() * sizeof(u64));
    P->loaded = true;
    return SBN_OK;
  }
};

// G1ExpStark / G2ExpStark (E = 1 / 2)
template <int E>
static int generate_trace_device(sbn_prover* P, const uint32_t* ios, size_t K, uint64_t* pi_out, const ChainedIn* ch = nullptr, const ScalarMulIn* sm = nullptr,
                                 const BatchIn* mb = nullptr) {
  const size_t IOW = 8 * (4 * E + 1);  // u32 words per instance: x and offset (2E Fq each) + exp_val
  std::vector<uint32_t> prelim;        // chained: x, start, exp_val of every instance; the device rewrites the offsets
  const size_t cin_words = sm ? 16 * E * K + 8 * sm->scalar_count + 16 * E : 0;   // scalar multiplications: u32 words of the compact upload
  std::vector<uint32_t> aux;           // segmented: head[K], then tail[segments] and head-of-segment[segments]
  const size_t NP = sm ? K : (mb ? mb->segments : 0);   // products (scalar multiplications) / sums (segmented) that come back
  if (sm) {   // the host keeps its own explicit list for the public inputs; only the compact form goes up
    if (int rc = scalar_mul_check_points(E, sm->points, K, sm->offset)) return rc;
    prelim.resize(IOW * K);
    scalar_mul_explicit_list(E, sm->points, sm->scalars, sm->scalar_count, K, K, sm->offset, prelim.data());
    ios = prelim.data();
  } else if (ch) {
    if (K > (size_t)tg::CS_LANES) return fail(SBN_ERR_UNSUPPORTED, "a chained list has at most %d instances", tg::CS_LANES);
    if (int rc = chain_terms_check_curve(E, ch->terms, K, ch->start)) return rc;
    prelim = preliminary_list(*ch, K, 16 * E, 8, ch->start);
    ios = prelim.data();
  } else if (mb) {   // segmented: x, the start of its segment, exp_val of every instance; heads of the lanes, then tail and head per segment
    if (K > (size_t)tg::CS_LANES) return fail(SBN_ERR_UNSUPPORTED, "a segmented list has at most %d instances", tg::CS_LANES);
    if (int rc = msm_batch_check_inputs(P->air.kind, mb->terms, mb->lengths, mb->segments, mb->starts, mb->start_count, mb->M)) return rc;
    std::vector<uint32_t> seg_head, seg_len;
    prelim = batch_preliminary_list(*mb, K, 16 * E, 8, [&](size_t s) { return mb->starts + (mb->start_count == 1 ? 0 : 16 * E * s); }, seg_head, seg_len, &aux);
    for (size_t s = 0; s < mb->segments; s++) aux.push_back(seg_head[s] + seg_len[s] - 1);
    aux.insert(aux.end(), seg_head.begin(), seg_head.end());
    ios = prelim.data();
  } else if (int rc = check_below_p(ios, IOW, 4 * E, K, "coordinate")) return rc;
  HIPC(hipSetDevice(P->device));
  TraceJob J(P, K, IOW);
  const size_t n = J.n;
  const hipStream_t st = J.st;
  const size_t cw = 257 * 12 * E * K;  // one Jacobian chain of every instance
  u64* ja = J.take(cw); u64* jb = J.take(cw);
  u64* sv = J.take(28 * E * n);       u64* inv = J.take(n);
  u64* d_out = J.take(16 * E * K);
  unsigned char* row_op = (unsigned char*)J.take(n / 8 + 1);
  uint32_t* d_ios = (uint32_t*)J.take(IOW * K / 2 + 1);
  uint32_t* d_prog[2] = {(uint32_t*)J.take(64 * tg::CP_LANES / 2), (uint32_t*)J.take(64 * tg::CP_LANES / 2)};   // chain programs: <= 64 levels of 64 micro-operations
  int* d_err = (int*)J.take(1);
  unsigned int* d_cnt = J.take_histograms();
  const bool scan = ch || mb;                                                 // chained and segmented lists derive their offsets here
  u64* d_pre = scan ? J.take(12 * E * tg::CT_LANES * K) : nullptr;            // chained: the partial sums of every instance,
  u64* d_terms = scan ? J.take(12 * E * K) : nullptr;                         // e_k x_k, then the two scan buffers
  u64* d_scan[2] = {scan ? J.take(12 * E * K) : nullptr, scan ? J.take(12 * E * K) : nullptr};
  int* d_err_pre = scan ? (int*)J.take(1) : nullptr;                          // flags of the preliminary chains (offsets = start): never read
  uint32_t* d_cin = sm ? (uint32_t*)J.take(cin_words / 2 + 1) : nullptr;      // scalar multiplications: the compact upload, the Jacobian
  u64* d_jp = NP ? J.take(12 * E * NP) : nullptr;                             // products between the two passes of a lane, the affine
  uint32_t* d_prod = NP ? (uint32_t*)J.take(8 * E * NP) : nullptr;            // products ([NP][16E] u32) and their infinity flags
  unsigned char* d_inf = NP ? (unsigned char*)J.take(NP / 8 + 1) : nullptr;
  uint32_t* d_aux = mb ? (uint32_t*)J.take(aux.size() / 2 + 1) : nullptr;     // segmented: the index arrays
  if (int rc = J.fits()) return rc;
  if (int rc = range_check_setup(P->device)) return rc;
  // both chains of every instance on the device, flags into `errw` (chain_mode 2 / 1, see below)
  auto launch_chains = [&](int* errw) -> int {
    if (P->chain_mode == 2) {
      static const ChainProgram prog = build_chain_program(E);
      if (prog.levels[0] <= 0 || prog.levels[0] > 24 || prog.levels[1] > 24) return fail(SBN_ERR_UNSUPPORTED, "internal: chain program does not fit");
      tg::ChainProgDev cp{};
      for (int b = 0; b < 2; b++) {
        HIPC(hipMemcpyAsync(d_prog[b], prog.ops[b].data(), prog.ops[b].size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        cp.ops[b] = d_prog[b]; cp.levels[b] = prog.levels[b];
      }
      for (int v = 0; v < 4; v++) for (int q = 0; q < E; q++) cp.in_slot[v * E + q] = (unsigned char)((v < 2 ? v : v + 1) * E + q);   // a.X a.Y | b.X b.Y
      cp.one_slot[0] = (unsigned char)(2 * E); cp.one_slot[1] = (unsigned char)(5 * E);
      cp.zero_slot[0] = (unsigned char)(2 * E + 1); cp.zero_slot[1] = (unsigned char)(5 * E + 1);
      for (int i = 0; i < 6 * E; i++) cp.coord[i] = (unsigned char)i;
      hipLaunchKernelGGL(tg::chain_coop_kernel<E>, dim3((unsigned)K), dim3(tg::CP_LANES), 0, st, d_ios, K, ja, jb, errw, cp);
    } else hipLaunchKernelGGL(tg::chain_kernel<E>, blocks(K, 64), dim3(64), 0, st, d_ios, K, ja, jb, errw);
    return 0;
  };
  // the instance list in and the outputs + error word back cross through pinned staging (chained: the derived list comes back too)
  // (scalar multiplications: the compact form in, the products and their flags back behind the outputs)
  const size_t io_words = sm ? (cin_words + 1) / 2 : (IOW * K + 1) / 2, out_words = 16 * E * K + 1;
  const size_t prod_words = 8 * E * NP, inf_words = (NP + 7) / 8;
  if (int rc = pinned_reserve(&P->h_io, &P->h_io_words, io_words + out_words + (scan ? io_words : 0) + prod_words + inf_words)) return rc;
  u64* const h_out = P->h_io + io_words;
  u64* const h_prod = h_out + out_words + (scan ? io_words : 0);   // (behind the derived list where one comes back)
  if (sm) {
    uint32_t* h = (uint32_t*)P->h_io;
    memcpy(h, sm->points, 16 * E * K * sizeof(uint32_t));
    memcpy(h + 16 * E * K, sm->scalars, 8 * sm->scalar_count * sizeof(uint32_t));
    memcpy(h + 16 * E * K + 8 * sm->scalar_count, sm->offset, 16 * E * sizeof(uint32_t));
    if (int rc = J.begin(P->h_io, d_cin, d_err, cin_words)) return rc;
    hipLaunchKernelGGL(tg::scalar_mul_list_kernel<E>, blocks(IOW * K, 256), dim3(256), 0, st, d_cin, K, sm->scalar_count, d_ios);
    J.mark();
  } else {
    memcpy(P->h_io, ios, IOW * K * sizeof(uint32_t));
    if (int rc = J.begin(P->h_io, d_ios, d_err)) return rc;
  }
  if (scan) {   // offsets on the device (kernels_tracegen.cuh, "chained instance lists"); only chain_mode 1 and 2 come here
    if (mb) HIPC(hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (int rc = launch_chains(d_err_pre)) return rc;
    hipLaunchKernelGGL(tg::chain_prefix_kernel<E>, dim3((unsigned)K), dim3(tg::CT_LANES), 0, st, d_ios, K, ja, d_pre, d_terms);
    if (mb) hipLaunchKernelGGL(tg::chain_seg_scan_kernel<E>, dim3(1), dim3(tg::CS_LANES), 0, st, d_ios, K, mb->M, d_aux, d_terms, d_scan[0], d_scan[1], d_err);
    else hipLaunchKernelGGL(tg::chain_scan_kernel<E>, dim3(1), dim3(tg::CS_LANES), 0, st, d_ios, K, d_terms, d_scan[0], d_scan[1], d_err);
    J.mark();
    ios = (const uint32_t*)(h_out + out_words);   // where the derived list lands, below
  }
  J.launch_common_columns(tg::flags_kernel, d_ios, inv, 65535);
  // the two 256-step curve chains per instance: host threads while the device writes the input-independent columns
  // chain_mode (SBN_TRACEGEN_DEVICE_CHAIN; create_ctx picks by the host pool's size): 2 = one wave per instance walking levels of
  // independent Fq operations (tg::chain_coop_kernel), 1 = one lane per instance (tg::chain_kernel, 13 ms), 0 = host threads +
  // pinned upload
  if (scan) hipLaunchKernelGGL(tg::chain_rebase_kernel<E>, blocks(K * 257, 64), dim3(64), 0, st, d_ios, K, d_pre, jb);   // A is in ja already
  else if (P->chain_mode) { if (int rc = launch_chains(d_err)) return rc; }
  else {
    if (int rc = pinned_reserve(&P->h_chain, &P->h_chain_words, 2 * cw)) return rc;
    if (tracegen_host_chains(E, ios, K, P->h_chain, P->h_chain + cw)) return fail(SBN_ERR_WITNESS, "degenerate affine operation (x1 == x2 or y == 0)");
    HIPC(hipMemcpyAsync(ja, P->h_chain, cw * sizeof(u64), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(jb, P->h_chain + cw, cw * sizeof(u64), hipMemcpyHostToDevice, st));
  }
  J.mark();
  hipLaunchKernelGGL(tg::affine_lambda_kernel<E>, blocks((n + tg::TG_ROWS - 1) / tg::TG_ROWS, 64), dim3(64), 0, st, d_ios, K, ja, jb, n, sv, row_op, d_out, d_err);
  J.mark();
  if (sm) {   // the products from the instance outputs affine_lambda_kernel left in d_out
    hipLaunchKernelGGL(tg::scalar_mul_unoffset_kernel<E>, blocks((K + tg::TG_INV_BATCH - 1) / tg::TG_INV_BATCH, 64), dim3(64), 0, st, d_ios, K, d_out, d_jp, d_prod, d_inf);
    J.mark();
  }
  if (mb) {   // final_s + (-start_s): the same kernel, indexed by the tail and the head of every segment
    hipLaunchKernelGGL(tg::scalar_mul_unoffset_kernel<E>, blocks((NP + tg::TG_INV_BATCH - 1) / tg::TG_INV_BATCH, 64), dim3(64), 0, st, d_ios, NP, d_out, d_jp, d_prod, d_inf,
                       d_aux + K, d_aux + K + NP);
    J.mark();
  }
  hipLaunchKernelGGL(tg::gadget_witness_kernel<E>, blocks(3 * E * n, 256), dim3(256), 0, st, sv, row_op, n, J.sh.gadget_col, P->d_trace, d_err);
  J.mark();
  if (int rc = J.launch_u16_range_check(d_cnt, d_err)) return rc;
  J.mark();
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(h_out, d_out, 16 * E * K * sizeof(u64), hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(h_out + 16 * E * K, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
  if (scan) HIPC(hipMemcpyAsync(h_out + out_words, d_ios, IOW * K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  static const char* const names[] = {"flags+pulses", "chains", "affine+lambda", "row_witness", "range_check"};
  if (NP) {
    HIPC(hipMemcpyAsync(h_prod, d_prod, 16 * E * NP * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(h_prod + prod_words, d_inf, NP, hipMemcpyDeviceToHost, st));
  }
  static const char* const names_chained[] = {"chain_offsets", "flags+pulses", "chains", "affine+lambda", "row_witness", "range_check"};
  static const char* const names_scalar[] = {"scalar_list", "flags+pulses", "chains", "affine+lambda", "un_offset", "row_witness", "range_check"};
  static const char* const names_batch[] = {"chain_offsets", "flags+pulses", "chains", "affine+lambda", "un_offset", "row_witness", "range_check"};
  if (int rc = J.end(sm ? names_scalar : mb ? names_batch : ch ? names_chained : names)) return rc;
  // public inputs: x, offset, exp_val, output as u32 limbs (g1/exp.rs:124-135, g2/exp.rs:139-156)
  const int rc = J.finish((int)(h_out[16 * E * K] & 0xffffffffu), pi_out, [&](size_t k, u64* p) {
    for (size_t i = 0; i < IOW; i++) p[i] = ios[IOW * k + i];
    for (int i = 0; i < 16 * E; i++) p[IOW + i] = h_out[16 * E * k + i];
  });
  if (rc == SBN_OK && ch && ch->ios_out) memcpy(ch->ios_out, ios, IOW * K * sizeof(uint32_t));
  if (sm && rc == SBN_ERR_WITNESS && ((int)(h_out[16 * E * K] & 0xffffffffu) & tg::TG_ERR_DEGENERATE)) {
    // the kernels report an error word only: the host walk names the first instance the table cannot walk (error path)
    if (int named = scalar_mul_name_degenerate(E, ios, K)) return named;
    return fail(SBN_ERR_WITNESS, "degenerate affine operation (x1 == x2 or y == 0)");
  }
  if (mb && rc == SBN_ERR_WITNESS && ((int)(h_out[16 * E * K] & 0xffffffffu) & (tg::TG_ERR_INFINITY | tg::TG_ERR_DEGENERATE))) {
    // the kernels report an error word only: the host derivation names the instance and its segment (error path)
    std::vector<uint32_t> named(IOW * K);
    if (int why = msm_batch_derive(P->air.kind, mb->terms, mb->lengths, mb->segments, mb->starts, mb->start_count, mb->M, K, named.data(), nullptr, nullptr, nullptr)) return why;
    return rc;
  }
  if (mb && rc == SBN_OK) {
    if (mb->ios_out) memcpy(mb->ios_out, ios, IOW * K * sizeof(uint32_t));
    if (mb->finals_out)   // the instance outputs at the segment tails: one u32 limb per u64 word
      for (size_t s = 0; s < NP; s++) for (int i = 0; i < 16 * E; i++) mb->finals_out[16 * E * s + i] = (uint32_t)h_out[16 * E * aux[K + s] + i];
    if (mb->sums_out) memcpy(mb->sums_out, h_prod, 16 * E * NP * sizeof(uint32_t));
    if (mb->infinity_out) memcpy(mb->infinity_out, h_prod + prod_words, NP);
  }
  if (sm && rc == SBN_OK) {
    if (sm->products_out) memcpy(sm->products_out, h_prod, 16 * E * K * sizeof(uint32_t));
    if (sm->infinity_out) memcpy(sm->infinity_out, h_prod + prod_words, K);
    if (sm->ios_out) memcpy(sm->ios_out, ios, IOW * K * sizeof(uint32_t));
  }
  return rc;
}

// Fq12ExpStark: the square-and-multiply chains (no inversion anywhere) on host threads in standard form, then one lane
// per row for the limb columns and the twelve modular-gadget witnesses, and the split range check per target column.
static int generate_trace_device_fq12(sbn_prover* P, const uint32_t* ios, size_t K, uint64_t* pi_out, const ChainedIn* ch = nullptr, const PowerIn* pw = nullptr,
                                      const BatchIn* mb = nullptr) {
  const bool u64e = P->air.kind == SBN_AIR_FQ12_EXP_U64;        // 128-row instances, one-element exponent
  const size_t IOW = u64e ? 194 : 200;
  const int steps = u64e ? 64 : 256, log_rpb = u64e ? 7 : 9;
  std::vector<uint32_t> prelim, derived;   // chained: x, one, exp_val of every instance; the device rewrites the offsets
  if (ch) {
    if (int rc = check_below_p(ch->start, 96, 12, 1, "coefficient of start")) return rc;
    uint32_t one[96] = {1};
    prelim = preliminary_list(*ch, K, 96, IOW - 192, one);
    derived.resize(IOW * K);
    ios = prelim.data();
  }
  std::vector<uint32_t> aux;   // segmented: head[segments], len[segments], then the starts ([start_count][96])
  if (mb) {   // x, one, exp_val of every instance (a pad row repeats row M - 1); the device rewrites the offsets
    if (int rc = msm_batch_check_inputs(P->air.kind, mb->terms, mb->lengths, mb->segments, mb->starts, mb->start_count, mb->M)) return rc;
    uint32_t one[96] = {1};
    std::vector<uint32_t> seg_head, seg_len;
    prelim = batch_preliminary_list(*mb, K, 96, IOW - 192, [&](size_t) { return (const uint32_t*)one; }, seg_head, seg_len, nullptr);
    aux = seg_head;
    aux.insert(aux.end(), seg_len.begin(), seg_len.end());
    aux.insert(aux.end(), mb->starts, mb->starts + 96 * mb->start_count);
    derived.resize(IOW * K);
    ios = prelim.data();
  }
  const size_t M = pw ? pw->count * pw->depth : K;   // towers: the real instances; rows [M, K) are pads
  if (pw) {   // x of level 0, zeros above it (the device writes them), one, the tower's exponent; a pad row repeats row M - 1
    if (int rc = power_check_inputs(P->air.kind, pw->bases, pw->exps, pw->exp_count, pw->count)) return rc;
    const size_t ew = IOW - 192;
    prelim.assign(IOW * K, 0u);
    for (size_t g = 0; g < K; g++) {
      const size_t r = g < M ? g : M - 1, k = r / pw->depth;
      uint32_t* io = prelim.data() + IOW * g;
      if (r % pw->depth == 0) memcpy(io, pw->bases + 96 * k, 96 * sizeof(uint32_t));
      io[96] = 1;
      memcpy(io + 192, pw->exps + (pw->exp_count == 1 ? 0 : ew * k), ew * sizeof(uint32_t));
    }
    ios = prelim.data();
  }
  if (int rc = check_below_p(ios, IOW, 24, K, "coefficient")) return rc;
  HIPC(hipSetDevice(P->device));
  if (u64e)
    for (size_t k = 0; k < K; k++)
      if (((u64)ios[IOW * k + 192] | ((u64)ios[IOW * k + 193] << 32)) >= GLP) return fail(SBN_ERR_NON_CANONICAL, "exponent of instance %zu is not a canonical field element", k);
  TraceJob J(P, K, IOW);
  const size_t n = J.n;
  const hipStream_t st = J.st;
  const size_t cw = (size_t)(steps + 1) * 48 * K;  // one chain of every instance, standard form
  u64* ca = J.take(cw); u64* cb = J.take(cw);
  u64* inv = J.take(n);
  u64* d_outs = J.take(K * 48);
  uint32_t* d_ios = (uint32_t*)J.take(IOW * K / 2 + 1);
  int* d_err = (int*)J.take(1);
  uint32_t* d_start = ch ? (uint32_t*)J.take(48) : nullptr;
  uint32_t* d_aux = mb ? (uint32_t*)J.take(aux.size() / 2 + 1) : nullptr;
  if (int rc = J.fits()) return rc;
  if (pw && (u64*)d_ios != d_outs + K * 48) return fail(SBN_ERR_UNSUPPORTED, "internal: the instance list does not follow the outputs");   // (one download, below)
  if (int rc = J.begin(ios, d_ios, d_err)) return rc;
  if (ch) {
    HIPC(hipMemcpyAsync(d_start, ch->start, 96 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    ios = derived.data();   // where the derived list lands, below
  }
  if (mb) {
    HIPC(hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    ios = derived.data();
  }
  if (u64e) J.launch_common_columns(tg::flags_u64_kernel, d_ios, inv, 255);
  else J.launch_common_columns(tg::flags_kernel, d_ios, inv, 255);
  // the square-and-multiply chains: one workgroup per instance on the device (kernels_tracegen.cuh fq12_chain_kernel);
  // SBN_FQ12_HOST_CHAIN=1: the library's host threads + a pinned upload, as in round 2 (A/B)
  const bool host_chain = P->set.fq12_host_chain && !pw;   // (towers under the host-chain switch never come here)
  if (pw) {   // d_ios holds the level-0 x, the offsets and the exponents: one workgroup per tower links and walks its levels
    hipLaunchKernelGGL(tg::fq12_tower_kernel, dim3((unsigned)pw->count), dim3(320), 0, st, d_ios, IOW, steps, pw->depth, ca, cb, d_outs);
    J.mark();
    if (M < K) hipLaunchKernelGGL(tg::fq12_tower_pad_kernel, dim3((unsigned)(K - M)), dim3(256), 0, st, d_ios, IOW, M, K, (size_t)(steps + 1) * 48, ca, cb, d_outs);
  } else if (host_chain) {
    if (int rc = pinned_reserve(&P->h_chain, &P->h_chain_words, 2 * cw)) return rc;
    tracegen_host_chains_fq12(ios, IOW, steps, K, P->h_chain, P->h_chain + cw);
    HIPC(hipMemcpyAsync(ca, P->h_chain, 2 * cw * sizeof(u64), hipMemcpyHostToDevice, st));  // ca and cb are adjacent
  } else hipLaunchKernelGGL(tg::fq12_chain_kernel, dim3((unsigned)K), dim3(320), 0, st, d_ios, IOW, steps, ca, cb, d_outs);
  J.mark();
  if (ch) {   // the chains above ran on offsets of one (device chains only): x^e of every instance is in d_outs; the running product
    // writes the offsets into d_ios and the chain is rebased onto them (kernels_tracegen.cuh, "chained instance lists")
    hipLaunchKernelGGL(tg::fq12_offset_scan_kernel, dim3(1), dim3(192), 0, st, d_ios, IOW, K, d_start, d_outs);
    hipLaunchKernelGGL(tg::fq12_rebase_kernel, dim3((unsigned)(K * (size_t)(steps + 1))), dim3(192), 0, st, d_ios, IOW, steps, cb, d_outs);
    J.mark();
  }
  if (mb) {   // the same on a segmented list: one workgroup per segment walks its own running product ("segmented chained lists")
    const size_t S = mb->segments;
    hipLaunchKernelGGL(tg::fq12_seg_scan_kernel, dim3((unsigned)S), dim3(192), 0, st, d_ios, IOW, K, mb->M, d_aux, d_aux + S, d_aux + 2 * S, mb->start_count, d_outs);
    hipLaunchKernelGGL(tg::fq12_rebase_kernel, dim3((unsigned)(K * (size_t)(steps + 1))), dim3(192), 0, st, d_ios, IOW, steps, cb, d_outs);
    J.mark();
  }
  // one lane per (row, output coefficient) by default; SBN_FQ12_ROW_KERNEL=1: round 2's one lane per row (A/B)
  const bool row_kernel = P->set.fq12_row_kernel;
  if (row_kernel) hipLaunchKernelGGL(tg::fq12_row_kernel, blocks(n, 64), dim3(64), 0, st, d_ios, IOW, log_rpb, ca, cb, n, P->d_trace, d_err);
  else hipLaunchKernelGGL(tg::fq12_gadget_kernel, blocks(12 * n, 256), dim3(256), 0, st, d_ios, IOW, log_rpb, ca, cb, n, P->d_trace, d_err);
  J.mark();
  hipLaunchKernelGGL(tg::split_range_check_kernel, dim3((unsigned)J.sh.num_rc), dim3(256), 0, st, P->d_trace, n, J.sh.rc_start, J.sh.start_lookups, d_err);
  J.mark();
  HIPC(hipGetLastError());
  int err = 0;
  HIPC(hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
  std::vector<u64> chain_out;                 // B[steps] of every instance (the outputs among the public inputs) when the chains ran on the device
  if (pw) {   // d_ios follows d_outs in the scratch (take() above): the outputs = the powers and the derived list in ONE download
    const size_t ios_u64 = (IOW * K + 1) / 2;
    chain_out.resize(K * 48 + ios_u64);
    HIPC(hipMemcpyAsync(chain_out.data(), d_outs, chain_out.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
    ios = (const uint32_t*)(chain_out.data() + K * 48);   // where the derived list lands
  } else if (!host_chain) {
    chain_out.resize(K * 48);
    HIPC(hipMemcpyAsync(chain_out.data(), d_outs, K * 48 * sizeof(u64), hipMemcpyDeviceToHost, st));
  }
  if (ch || mb) HIPC(hipMemcpyAsync(derived.data(), d_ios, IOW * K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  static const char* const names[] = {"flags+pulses", "chains", "row_witness", "range_check"};
  static const char* const names_chained[] = {"flags+pulses", "chains", "chain_offsets", "row_witness", "range_check"};
  static const char* const names_tower[] = {"flags+pulses", "tower_links", "tower_pads", "row_witness", "range_check"};
  if (int rc = J.end(pw ? names_tower : (ch || mb) ? names_chained : names)) return rc;
  // public inputs: x, offset as 16-bit limbs, exp_val, output = b at the last row (fq12/exp.rs:95-117)
  const int rc = J.finish(err, pi_out, [&](size_t k, u64* p) {
    for (int c = 0; c < 24; c++)
      for (int i = 0; i < 16; i++) p[16 * c + i] = (ios[IOW * k + 8 * c + (i >> 1)] >> (16 * (i & 1))) & 0xffff;
    if (u64e) p[384] = (u64)ios[IOW * k + 192] | ((u64)ios[IOW * k + 193] << 32);
    else for (int i = 0; i < 8; i++) p[384 + i] = ios[IOW * k + 192 + i];
    const u64* out = host_chain ? P->h_chain + cw + ((k * (steps + 1) + steps) * 12) * 4 : chain_out.data() + k * 48;  // B[steps]
    const int ob = 384 + J.sh.n_exp_slots;
    for (int c = 0; c < 12; c++) for (int i = 0; i < 16; i++) p[ob + 16 * c + i] = (out[4 * c + (i >> 2)] >> (16 * (i & 3))) & 0xffff;
  });
  if (rc == SBN_OK && ch && ch->ios_out) memcpy(ch->ios_out, ios, IOW * K * sizeof(uint32_t));
  if (rc == SBN_OK && mb) {
    if (mb->ios_out) memcpy(mb->ios_out, ios, IOW * K * sizeof(uint32_t));
    if (mb->finals_out)   // [segments][96] u32 = the outputs of the segment tails, standard form
      for (size_t s = 0; s < mb->segments; s++) {
        const u64* out = chain_out.data() + 48 * (size_t)(aux[s] + aux[mb->segments + s] - 1);
        for (size_t i = 0; i < 48; i++) { mb->finals_out[96 * s + 2 * i] = (uint32_t)out[i]; mb->finals_out[96 * s + 2 * i + 1] = (uint32_t)(out[i] >> 32); }
      }
  }
  if (rc == SBN_OK && pw) {
    if (pw->ios_out) memcpy(pw->ios_out, ios, IOW * K * sizeof(uint32_t));
    if (pw->powers_out)   // [count][depth][96] u32 = the outputs of the M real instances, standard form
      for (size_t i = 0; i < 48 * M; i++) { pw->powers_out[2 * i] = (uint32_t)chain_out[i]; pw->powers_out[2 * i + 1] = (uint32_t)(chain_out[i] >> 32); }
  }
  return rc;
}

// FqExpStark: chains on host threads (512 Montgomery products per instance), rows and the u16 range check on the device.
static int generate_trace_device_fq(sbn_prover* P, const uint32_t* ios, size_t K, uint64_t* pi_out) {
  const size_t IOW = 24;
  if (int rc = check_below_p(ios, IOW, 2, K, "value")) return rc;
  HIPC(hipSetDevice(P->device));
  TraceJob J(P, K, IOW);
  const size_t n = J.n;
  const hipStream_t st = J.st;
  const size_t cw = 257 * 4 * K;
  u64* ca = J.take(cw); u64* cb = J.take(cw);
  u64* inv = J.take(n);
  uint32_t* d_ios = (uint32_t*)J.take(IOW * K / 2 + 1);
  int* d_err = (int*)J.take(1);
  unsigned int* d_cnt = J.take_histograms();
  if (int rc = J.fits()) return rc;
  if (int rc = range_check_setup(P->device)) return rc;
  if (int rc = J.begin(ios, d_ios, d_err)) return rc;
  J.launch_common_columns(tg::flags_kernel, d_ios, inv, 65535);
  if (int rc = pinned_reserve(&P->h_chain, &P->h_chain_words, 2 * cw)) return rc;
  tracegen_host_chains_fq(ios, K, P->h_chain, P->h_chain + cw);
  HIPC(hipMemcpyAsync(ca, P->h_chain, 2 * cw * sizeof(u64), hipMemcpyHostToDevice, st));  // ca and cb are adjacent
  J.mark();
  hipLaunchKernelGGL(tg::fq_row_kernel, blocks(n, 128), dim3(128), 0, st, d_ios, ca, cb, n, P->d_trace, d_err);
  J.mark();
  if (int rc = J.launch_u16_range_check(d_cnt, d_err)) return rc;
  J.mark();
  HIPC(hipGetLastError());
  int err = 0;
  HIPC(hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
  static const char* const names[] = {"flags+pulses", "chains", "row_witness", "range_check"};
  if (int rc = J.end(names)) return rc;
  // public inputs: x, offset, exp_val, output = b at the last row, as u32 limbs (fq/exp.rs:98-108)
  return J.finish(err, pi_out, [&](size_t k, u64* p) {
    for (size_t i = 0; i < IOW; i++) p[i] = ios[IOW * k + i];
    const u64* out = P->h_chain + cw + (k * 257 + 256) * 4;  // B[256]
    for (int i = 0; i < 8; i++) p[24 + i] = (out[i >> 1] >> (32 * (i & 1))) & 0xffffffffULL;
  });
}

// sbn_prover_generate_trace on the list sbn_chain_instances derives from (terms, start), the offsets built on the device where the
// chains already run there: G1 / G2 under chain_mode 1 and 2, Fq12 / Fq12U64 unless SBN_FQ12_HOST_CHAIN.  Elsewhere (host-pool
// curve chains, FqExpStark) the chains are host work anyway and so is the list.
extern "C" int sbn_prover_generate_trace_chained(sbn_prover* P, const uint32_t* terms, size_t num_io, const uint32_t* start, uint64_t* pi_out, uint32_t* ios_out) {
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  P->loaded = false;   // before any check, as sbn_prover_generate_trace
  if (!terms || !start) return fail(SBN_ERR_BAD_ARG, "null argument");
  const int kind = P->air.kind;
  if (!is_exp_air(kind)) return fail(SBN_ERR_UNSUPPORTED, "device witness generation covers the Exp tables (use sbn_generate_trace_g1_op + sbn_prover_load_trace)");
  if (num_io != P->air.num_io) return fail(SBN_ERR_BAD_ARG, "prover was created for %u instances, got %zu", P->air.num_io, num_io);
  if (P->n != exp_rows_per_instance(kind) * num_io) return fail(SBN_ERR_BAD_ARG, "degree_bits does not match the rows per instance");
  const bool fq12 = kind == SBN_AIR_FQ12_EXP || kind == SBN_AIR_FQ12_EXP_U64;
  if (!fq12 && (P->n < 65536 || P->n > 262144)) return fail(SBN_ERR_UNSUPPORTED, "device witness generation of the u16-range-check tables covers 2^16 .. 2^18 rows");
  if (kind == SBN_AIR_FQ_EXP || (fq12 ? P->set.fq12_host_chain : P->chain_mode == 0)) {
    std::vector<uint32_t> ios(exp_io_words(kind) * num_io);
    if (int rc = chain_instances_host(kind, terms, num_io, start, ios.data(), nullptr)) return rc;
    const int rc = sbn_prover_generate_trace(P, ios.data(), num_io, pi_out);
    if (rc == SBN_OK && ios_out) memcpy(ios_out, ios.data(), ios.size() * sizeof(uint32_t));
    return rc;
  }
  const ChainedIn ch{terms, start, ios_out};
  if (fq12) return generate_trace_device_fq12(P, nullptr, num_io, pi_out, &ch);
  return kind == SBN_AIR_G1_EXP ? generate_trace_device<1>(P, nullptr, num_io, pi_out, &ch) : generate_trace_device<2>(P, nullptr, num_io, pi_out, &ch);
}

// sbn_prover_generate_trace on the list sbn_scalar_mul_instances derives from (points, scalars, offset), one unit: where the curve
// chains run on the device (chain_mode 1 and 2) the list is expanded and un-offset there; with host-pool chains the list is host
// work anyway and takes the explicit path.
extern "C" int sbn_prover_generate_trace_scalar_muls(sbn_prover* P, const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t num_io,
                                                     const uint32_t* offset, uint64_t* pi_out, uint32_t* products_out, uint8_t* infinity_out, uint32_t* ios_out) {
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  P->loaded = false;   // before any check, as sbn_prover_generate_trace
  const int kind = P->air.kind;
  if (kind != SBN_AIR_G1_EXP && kind != SBN_AIR_G2_EXP) return fail(SBN_ERR_UNSUPPORTED, "scalar multiplications cover the curve tables G1_EXP and G2_EXP");
  if (!points || !scalars || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument or no instance");
  if (scalar_count != 1 && scalar_count != num_io) return fail(SBN_ERR_BAD_ARG, "scalar_count must be 1 (one shared scalar) or count = %zu, got %zu", num_io, scalar_count);
  if (num_io != P->air.num_io) return fail(SBN_ERR_BAD_ARG, "prover was created for %u instances, got %zu", P->air.num_io, num_io);
  if (P->n != exp_rows_per_instance(kind) * num_io) return fail(SBN_ERR_BAD_ARG, "degree_bits does not match the rows per instance");
  if (P->n < 65536 || P->n > 262144) return fail(SBN_ERR_UNSUPPORTED, "device witness generation of the u16-range-check tables covers 2^16 .. 2^18 rows");
  const int E = kind == SBN_AIR_G1_EXP ? 1 : 2;
  if (!offset) offset = curve_generator_words(E);
  if (P->chain_mode == 0) {
    std::vector<uint32_t> ios(exp_io_words(kind) * num_io);
    if (int rc = sbn_scalar_mul_instances(kind, points, scalars, scalar_count, num_io, num_io, offset, ios.data(), products_out, infinity_out)) return rc;
    const int rc = sbn_prover_generate_trace(P, ios.data(), num_io, pi_out);
    if (rc == SBN_OK && ios_out) memcpy(ios_out, ios.data(), ios.size() * sizeof(uint32_t));
    return rc;
  }
  const ScalarMulIn sm{points, scalars, scalar_count, offset, products_out, infinity_out, ios_out};
  return E == 1 ? generate_trace_device<1>(P, nullptr, num_io, pi_out, nullptr, &sm) : generate_trace_device<2>(P, nullptr, num_io, pi_out, nullptr, &sm);
}

// sbn_prover_generate_trace on the one-unit list sbn_msm_batch_instances derives from (terms, lengths, starts): where the table's
// chains run on the device (G1 / G2 under chain_mode 1 and 2, Fq12 / Fq12U64 unless SBN_FQ12_HOST_CHAIN) the offsets, the finals and
// the sums are derived there; elsewhere (host-pool curve chains, FqExpStark) the list is host work anyway and takes the explicit path.
extern "C" int sbn_prover_generate_trace_msm_batch(sbn_prover* P, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts,
                                                   size_t start_count, uint64_t* pi_out, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out,
                                                   uint32_t* ios_out) {
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  P->loaded = false;   // before any check, as sbn_prover_generate_trace
  const int kind = P->air.kind;
  const size_t num_io = P->air.num_io;
  size_t M = 0;
  if (int rc = msm_batch_check_args(kind, terms, lengths, segments, &starts, &start_count, num_io, sums_out, infinity_out, &M)) return rc;
  if (M > num_io) return fail(SBN_ERR_BAD_ARG, "%zu segments of %zu instances do not fit one unit of %zu instances", segments, M, num_io);
  if (P->n != exp_rows_per_instance(kind) * num_io) return fail(SBN_ERR_BAD_ARG, "degree_bits does not match the rows per instance");
  const bool fq12 = kind == SBN_AIR_FQ12_EXP || kind == SBN_AIR_FQ12_EXP_U64;
  if (!fq12 && (P->n < 65536 || P->n > 262144)) return fail(SBN_ERR_UNSUPPORTED, "device witness generation of the u16-range-check tables covers 2^16 .. 2^18 rows");
  if (kind == SBN_AIR_FQ_EXP || (fq12 ? P->set.fq12_host_chain : P->chain_mode == 0)) {
    std::vector<uint32_t> ios(exp_io_words(kind) * num_io);
    if (int rc = msm_batch_derive(kind, terms, lengths, segments, starts, start_count, M, num_io, ios.data(), finals_out, sums_out, infinity_out)) return rc;
    const int rc = sbn_prover_generate_trace(P, ios.data(), num_io, pi_out);
    if (rc == SBN_OK && ios_out) memcpy(ios_out, ios.data(), ios.size() * sizeof(uint32_t));
    return rc;
  }
  const BatchIn mb{terms, lengths, segments, starts, start_count, M, finals_out, sums_out, infinity_out, ios_out};
  if (fq12) return generate_trace_device_fq12(P, nullptr, num_io, pi_out, nullptr, nullptr, &mb);
  return kind == SBN_AIR_G1_EXP ? generate_trace_device<1>(P, nullptr, num_io, pi_out, nullptr, nullptr, &mb)
                                : generate_trace_device<2>(P, nullptr, num_io, pi_out, nullptr, nullptr, &mb);
}

// sbn_prover_generate_trace on the one-unit list sbn_power_instances derives from (bases, exps, depth): on an Fq12 table whose
// chains run on the device the towers are linked and walked there (one workgroup per tower) and the pads filled there; FqExpStark
// (host-pool chains) and an Fq12 prover under SBN_FQ12_HOST_CHAIN walk the towers on the host pool and take the explicit path.
extern "C" int sbn_prover_generate_trace_powers(sbn_prover* P, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count, size_t depth,
                                                uint64_t* pi_out, uint32_t* powers_out, uint32_t* ios_out) {
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  P->loaded = false;   // before any check, as sbn_prover_generate_trace
  const int kind = P->air.kind;
  if (!power_elem_words(kind)) return fail(SBN_ERR_UNSUPPORTED, "field powers cover the field tables FQ_EXP, FQ12_EXP and FQ12_EXP_U64");
  if (!bases || !exps || count == 0 || depth == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no tower or depth = 0");
  if (exp_count != 1 && exp_count != count) return fail(SBN_ERR_BAD_ARG, "exp_count must be 1 (one shared exponent) or count = %zu, got %zu", count, exp_count);
  const size_t num_io = P->air.num_io;
  if (count > num_io || depth > num_io / count) return fail(SBN_ERR_BAD_ARG, "%zu towers of depth %zu do not fit one unit of %zu instances", count, depth, num_io);
  if (P->n != exp_rows_per_instance(kind) * num_io) return fail(SBN_ERR_BAD_ARG, "degree_bits does not match the rows per instance");
  const bool fq12 = kind != SBN_AIR_FQ_EXP;
  if (!fq12 && (P->n < 65536 || P->n > 262144)) return fail(SBN_ERR_UNSUPPORTED, "device witness generation of the u16-range-check tables covers 2^16 .. 2^18 rows");
  if (!fq12 || P->set.fq12_host_chain) {
    std::vector<uint32_t> ios(exp_io_words(kind) * num_io);
    if (int rc = sbn_power_instances(kind, bases, exps, exp_count, count, depth, num_io, ios.data(), powers_out)) return rc;
    const int rc = sbn_prover_generate_trace(P, ios.data(), num_io, pi_out);
    if (rc == SBN_OK && ios_out) memcpy(ios_out, ios.data(), ios.size() * sizeof(uint32_t));
    return rc;
  }
  const PowerIn pw{bases, exps, exp_count, count, depth, powers_out, ios_out};
  return generate_trace_device_fq12(P, nullptr, num_io, pi_out, nullptr, &pw);
}

extern "C" int sbn_prover_generate_trace(sbn_prover* P, const uint32_t* ios, size_t num_io, uint64_t* pi_out) {
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  P->loaded = false;   // before any check: a refused instance list must not leave the previous trace provable
  if (!ios) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (!is_exp_air(P->air.kind)) return fail(SBN_ERR_UNSUPPORTED, "device witness generation covers the Exp tables (use sbn_generate_trace_g1_op + sbn_prover_load_trace)");
  if (num_io != P->air.num_io) return fail(SBN_ERR_BAD_ARG, "prover was created for %u instances, got %zu", P->air.num_io, num_io);
  if (P->n != exp_rows_per_instance(P->air.kind) * num_io) return fail(SBN_ERR_BAD_ARG, "degree_bits does not match the rows per instance");
  if (P->air.kind == SBN_AIR_FQ12_EXP || P->air.kind == SBN_AIR_FQ12_EXP_U64) return generate_trace_device_fq12(P, ios, num_io, pi_out);
  if (P->n < 65536 || P->n > 262144) return fail(SBN_ERR_UNSUPPORTED, "device witness generation of the u16-range-check tables covers 2^16 .. 2^18 rows");
  if (P->air.kind == SBN_AIR_FQ_EXP) return generate_trace_device_fq(P, ios, num_io, pi_out);
  return P->air.kind == SBN_AIR_G1_EXP ? generate_trace_device<1>(P, ios, num_io, pi_out) : generate_trace_device<2>(P, ios, num_io, pi_out);
}

extern "C" int sbn_bn254_fq_batch(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, int on_device) {
  using namespace tg;
  if (op < FQB_MUL || op > FQB_FQ2_INV) return fail(SBN_ERR_BAD_ARG, "unknown op %d", op);
  const bool binary = op == FQB_MUL || op == FQB_ADD || op == FQB_SUB || op == FQB_FQ2_INV;
  if (!a || !out || (binary && !b)) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (op == FQB_BATCH_INV && count % TG_INV_BATCH) return fail(SBN_ERR_BAD_ARG, "batch inverse needs a multiple of %d values", TG_INV_BATCH);
  for (size_t i = 0; i < count; i++) {
    if (bnw::geq_p(a + 4 * i) || (binary && bnw::geq_p(b + 4 * i))) return fail(SBN_ERR_NON_CANONICAL, "element %zu is not below p", i);
    const bool za = !(a[4 * i] | a[4 * i + 1] | a[4 * i + 2] | a[4 * i + 3]);
    const bool zb = !binary || !(b[4 * i] | b[4 * i + 1] | b[4 * i + 2] | b[4 * i + 3]);
    if ((op == FQB_INV || op == FQB_BATCH_INV) && za) return fail(SBN_ERR_BAD_ARG, "element %zu is zero: no inverse", i);
    if (op == FQB_FQ2_INV && za && zb) return fail(SBN_ERR_BAD_ARG, "element %zu is zero: no inverse", i);
  }
  const size_t items = op == FQB_BATCH_INV ? count / TG_INV_BATCH : count, out_words = 4 * count * (op == FQB_FQ2_INV ? 2 : 1);
  if (!on_device) {
    for (size_t i = 0; i < items; i++) fq_batch_item(op, a, b, out, i);
    return SBN_OK;
  }
  if (int rc = use_current_device("no CPU fallback")) return rc;
  if (count == 0) return SBN_OK;
  u64* d = nullptr;
  HIPC(hipMalloc((void**)&d, (8 * count + out_words) * sizeof(u64)));
  hipError_t e = hipMemcpy(d, a, 4 * count * sizeof(u64), hipMemcpyHostToDevice);
  if (e == hipSuccess && binary) e = hipMemcpy(d + 4 * count, b, 4 * count * sizeof(u64), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fq_batch_kernel, dim3((unsigned)((items + 63) / 64)), dim3(64), 0, 0, op, d, d + 4 * count, d + 8 * count, items);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, d + 8 * count, out_words * sizeof(u64), hipMemcpyDeviceToHost);
  }
  (void)hipFree(d);
  if (e != hipSuccess) return fail(SBN_ERR_HIP, "sbn_bn254_fq_batch: %s", hipGetErrorString(e));
  return SBN_OK;
}
