// On-device witness generation of the Exp tables (sbn_prover_generate_trace) and the parity hook of the BN254 field helpers
// (sbn_bn254_fq_batch): the one unit that includes kernels_tracegen.cuh, whose kernels are ordinary external definitions.
#include "prover_ctx.hpp"
#include "kernels_tracegen.cuh"
#include "instance_lists.hpp"
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
    HIPC(hipFuncSetAttribute((const void*)tg::range_check_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tg::RC_TALL_LDS_BYTES));
    done[d].store(true);
  }
  return 0;
}
// The words tg::periodic_kernel and tg::io_pulse_kernel write, compared with `block` = columns fixed_columns_range() of a trace of n
// rows, on `s`: *d_mismatch (zeroed here, in front of the kernel) becomes 1 at the first other word.  The caller waits and reads it.
int launch_fixed_columns_check(const u64* block, size_t ncols, size_t n, const ExpShape& sh, unsigned long long* d_mismatch, hipStream_t s) {
  if (ncols != (size_t)(sh.start_periodic >= 0 ? 4 : 2) + 4 * (size_t)sh.num_io || ncols > 65535) return fail(SBN_ERR_BAD_ARG, "internal: not the shape-constant block of this table");
  HIPC(hipMemsetAsync(d_mismatch, 0, sizeof *d_mismatch, s));
  hipLaunchKernelGGL(tg::fixed_columns_check_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)ncols), dim3(256), 0, s, block, n, sh.start_periodic >= 0 ? 1 : 0, (size_t)sh.rpb,
                     exp_table_max(sh), d_mismatch);
  HIPC(hipGetLastError());
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
    if (!curve_host::below_p(ios + IOW * k, values)) return fail(SBN_ERR_BAD_ARG, "%s >= p (instance %zu)", what, k);
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

// ---- the list sources: what each sbn_prover_generate_trace_* call hands its driver -----------------------------------------------
// sbn_prover_generate_trace_chained: the offsets are derived on the device from `terms` (instance rows without their offset words)
// and `start`.
struct ChainedIn { const uint32_t* terms; const uint32_t* start; uint32_t* ios_out; };

// sbn_prover_generate_trace_scalar_muls: every instance carries `offset`; the list is expanded on the device from the points, the
// one-or-K scalars and the offset, and the products output + (-offset) are computed there (kernels_tracegen.cuh, "independent
// scalar multiplications").  G1 / G2 only.
struct ScalarMulIn { const uint32_t* points; const uint32_t* scalars; size_t scalar_count; const uint32_t* offset; uint32_t* products_out; uint8_t* infinity_out; uint32_t* ios_out; };

// sbn_prover_generate_trace_powers: `count` towers of `depth` levels on an Fq12 table whose chains run on the device; level 0 takes
// its x from `bases`, level l from the output of level l - 1, derived on the device (kernels_tracegen.cuh, "power towers").
struct PowerIn { const uint32_t* bases; const uint32_t* exps; size_t exp_count, count, depth; uint32_t* powers_out; uint32_t* ios_out; };

// sbn_prover_generate_trace_program: `count` nodes on an Fq12 table whose chains run on the device; x and offset of a node are a
// literal of `values`, one, or the output of an earlier node, resolved on the device level by level (kernels_tracegen.cuh, "field
// programs").  maps (optional, [count]): the Frobenius maps of the links of a mapped program, applied on the device too
// (kernels_tracegen.cuh, "mapped links").
struct ProgramIn { const sbn_program_node* nodes; const uint32_t* maps; size_t count; const uint32_t* values; const uint32_t* exps; uint32_t* outs_out; uint32_t* ios_out; };

// sbn_prover_generate_trace_curve_program: `count` nodes on a curve table whose chains run on the device; x and offset of a node
// are a literal of `points`, the start (candidate 0), or the output of an earlier node, resolved on the device level by level
// (kernels_tracegen.cuh, "curve programs"); the values output + (-blind) are computed there from the blinds the host derives.
struct CurveProgramIn {
  const sbn_program_node* nodes; size_t count; const uint32_t* points; const uint32_t* exps;
  uint32_t* outs_out; uint32_t* values_out; uint8_t* infinity_out; uint32_t* ios_out;
};

// sbn_prover_generate_trace_msm_batch: one unit of `segments` chained lists, M real instances and num_io - M pads; the offsets are
// derived on the device from the terms, the heads and the starts (kernels_tracegen.cuh, "segmented chained lists"), the finals
// are the instance outputs at the segment tails and, on the curves, the sums final + (-start) are computed there too.
struct BatchIn {
  const uint32_t* terms; const uint64_t* lengths; size_t segments; const uint32_t* starts; size_t start_count, M;
  uint32_t* finals_out; uint32_t* sums_out; uint8_t* infinity_out; uint32_t* ios_out;
  // complete sums (null: the starts are the caller's): choice[s] in, every entry 0 with `starts` = candidate 0 for every segment;
  // out: the candidate segment s starts from, its words in starts_out[s]
  uint8_t* choice = nullptr; uint32_t* starts_out = nullptr;
};
// the preliminary list of a segmented one (a chained list is one segment): row g carries x and exponent of instance min(g, M - 1)
// and `offset_of(segment)` as its offset (xw words each, ew of the exponent); head_of[g] = the head of the segment of that
// instance (optional); seg_head / seg_len: per segment
static std::vector<uint32_t> preliminary_list(const uint32_t* terms, const uint64_t* lengths, size_t segments, size_t M, size_t K, size_t xw, size_t ew,
                                              const std::function<const uint32_t*(size_t)>& offset_of, std::vector<uint32_t>& seg_head, std::vector<uint32_t>& seg_len,
                                              std::vector<uint32_t>* head_of = nullptr) {
  std::vector<uint32_t> ios((2 * xw + ew) * K);
  seg_head.resize(segments); seg_len.resize(segments);
  if (head_of) head_of->resize(K);
  size_t g = 0;
  for (size_t s = 0; s < segments; s++) {
    seg_head[s] = (uint32_t)g; seg_len[s] = (uint32_t)lengths[s];
    for (size_t j = 0; j < lengths[s]; j++, g++) {
      uint32_t* io = ios.data() + (2 * xw + ew) * g;
      memcpy(io, terms + (xw + ew) * g, xw * sizeof(uint32_t));
      memcpy(io + xw, offset_of(s), xw * sizeof(uint32_t));
      memcpy(io + 2 * xw, terms + (xw + ew) * g + xw, ew * sizeof(uint32_t));
      if (head_of) (*head_of)[g] = seg_head[s];
    }
  }
  curve_host::pad_rows(ios.data(), 2 * xw + ew, M, K);
  for (; head_of && g < K; g++) (*head_of)[g] = (uint32_t)g;   // (never read: the scan's lanes stop at M)
  return ios;
}
static std::vector<uint32_t> preliminary_list(const ChainedIn& ch, size_t K, size_t xw, size_t ew, const uint32_t* offset) {
  const uint64_t length = K;
  std::vector<uint32_t> head, len;
  return preliminary_list(ch.terms, &length, 1, K, K, xw, ew, [&](size_t) { return offset; }, head, len);
}
// the preliminary list of a program: row g carries the literals and the exponent of node min(g, M - 1) in place, `special_words` (one,
// the start) where its offset is `special`, and zeros where the device will resolve a link; aux = the node table [K][3], then `order`
static std::vector<uint32_t> program_prelim(const sbn_program_node* nodes, size_t M, size_t K, size_t xw, size_t ew, const uint32_t* literals, const uint32_t* exps,
                                            uint32_t special, const uint32_t* special_words, const std::vector<uint32_t>& order, std::vector<uint32_t>& aux) {
  std::vector<uint32_t> ios((2 * xw + ew) * K, 0u);
  aux.resize(3 * K);
  for (size_t g = 0; g < K; g++) {
    const sbn_program_node& nd = nodes[g < M ? g : M - 1];
    uint32_t* io = ios.data() + (2 * xw + ew) * g;
    if (!curve_host::linked(nd.x)) memcpy(io, literals + xw * nd.x, xw * sizeof(uint32_t));
    if (nd.offset == special) memcpy(io + xw, special_words, xw * sizeof(uint32_t));
    else if (!curve_host::linked(nd.offset)) memcpy(io + xw, literals + xw * nd.offset, xw * sizeof(uint32_t));
    memcpy(io + 2 * xw, exps + ew * nd.exp, ew * sizeof(uint32_t));
    aux[3 * g] = nd.x; aux[3 * g + 1] = nd.offset; aux[3 * g + 2] = nd.exp;
  }
  aux.insert(aux.end(), order.begin(), order.end());
  return ios;
}

// ---- the stages -----------------------------------------------------------------------------------------------------------------
// One sbn_prover_generate_trace* call: the scratch carver, the launches every table has, the SBN_TRACE_TIMING marks and the tail.
// The two jobs below add the buffers and the stages of their tables.  A stage launches what it always launched and never asks
// which list source called it; one driver per source calls the stages top to bottom, carves what only its source needs behind
// the shared buffers (which so stay where they were) and owns its staging layout, its output copies and its error naming.
struct TraceJob : LdeScratch {   // (the scratch carver: prover_ctx.hpp; the LDE buffer is not yet in use)
  const size_t K, IOW, n;   // K instances of IOW u32 words each
  const hipStream_t st;
  const ExpShape sh;
  bool common_written = false;   // launch_common_columns ran: the shape-constant columns hold the generators' words (finish)
  struct Mark { hipEvent_t ev; const char* closes; };
  std::vector<Mark> marks;
  TraceJob(sbn_prover* P, size_t K, size_t IOW) : LdeScratch(P), K(K), IOW(IOW), n(P->n), st(P->stream), sh(exp_shape(P->air)) {}

  unsigned int* take_histograms() { return n > 65536 ? (unsigned int*)take((size_t)sh.num_rc * 32768) : nullptr; }   // u32 histograms of the range-checked columns

  // SBN_TRACE_TIMING: a point on the stream; `closes` names the span that ends here (begin() opens the first one)
  void mark(const char* closes) {
    hipEvent_t e;
    if (P->set.trace_timing && hipEventCreate(&e) == hipSuccess && hipEventRecord(e, st) == hipSuccess) marks.push_back({e, closes});
  }
  // the timed span opens (EX_TRACEGEN_MS); the instance list goes in from `h_ios`, the caller's memory or a pinned copy of it
  // (`words`: u32 words that go up when it is not the whole list: the compact form of the scalar multiplications)
  int begin(const void* h_ios, uint32_t* d_ios, int* d_err, size_t words = 0) {
    HIPC(hipEventRecord(P->abs_ev[0], st));
    HIPC(hipMemcpyAsync(d_ios, h_ios, (words ? words : IOW * K) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPC(hipMemsetAsync(d_err, 0, sizeof(int), st));
    mark(nullptr);
    return 0;
  }
  // the input-independent columns; table_max: the last entry of the lookup table (u16 tables 65535, the split check's 255)
  template <typename FlagsKernel>
  void launch_common_columns(FlagsKernel flags, const uint32_t* d_ios, u64* inv, u64 table_max) {
    hipLaunchKernelGGL(flags, blocks(n, 256), dim3(256), 0, st, d_ios, IOW, n, sh.start_flags, P->d_trace);
    launch_shape_columns(inv, table_max);
    mark("flags+pulses");
  }
  // their part that reads no instance list: the inverse table, the periodic pulse, the io-pulse counter and pairs, the table column
  // (launch_derived_columns runs it alone: the flags of a row-major load are the caller's)
  void launch_shape_columns(u64* inv, u64 table_max) {
    hipLaunchKernelGGL(tg::small_inverse_kernel, blocks(n, 256), dim3(256), 0, st, inv, n);
    hipLaunchKernelGGL(tg::periodic_kernel, blocks(n, 256), dim3(256), 0, st, inv, n, sh.start_periodic, sh.start_io_pulses, sh.start_lookups, table_max, P->d_trace);
    hipLaunchKernelGGL(tg::io_pulse_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)(2 * K)), dim3(256), 0, st, inv, n, (size_t)sh.rpb, sh.witness_col(0), P->d_trace);
    common_written = true;
  }
  // the last launches of the u16 tables, then whatever a launch since begin() left as an error
  int launch_u16_range_check(unsigned int* d_cnt, int* d_err) {
    if (n > 65536) {   // multiplicities beyond u16: histogram of every target column in HBM first (kernels_tracegen.cuh)
      HIPC(hipMemsetAsync(d_cnt, 0, (size_t)sh.num_rc * 65536 * sizeof(unsigned int), st));
      hipLaunchKernelGGL(tg::range_count_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)sh.num_rc), dim3(256), 0, st, P->d_trace, n, sh.rc_start, d_cnt, d_err);
      if (n > 262144)   // more crossings of 2^16 than the BIG form keeps, a cut of heavy[] that grows with n (kernels_tracegen.cuh)
        hipLaunchKernelGGL((tg::range_check_kernel<true, true>), dim3((unsigned)sh.num_rc), dim3(tg::RC_THREADS), tg::RC_TALL_LDS_BYTES, st, P->d_trace, n, sh.rc_start, sh.start_lookups, d_err, d_cnt, P->set.range_check);
      else
        hipLaunchKernelGGL(tg::range_check_kernel<true>, dim3((unsigned)sh.num_rc), dim3(tg::RC_THREADS), tg::RC_LDS_BYTES, st, P->d_trace, n, sh.rc_start, sh.start_lookups, d_err, d_cnt, P->set.range_check);
    } else {
      hipLaunchKernelGGL(tg::range_check_kernel<false>, dim3((unsigned)sh.num_rc), dim3(tg::RC_THREADS), tg::RC_LDS_BYTES, st, P->d_trace, n, sh.rc_start, sh.start_lookups, d_err, (const unsigned int*)nullptr, P->set.range_check);
    }
    mark("range_check");
    HIPC(hipGetLastError());
    return 0;
  }
  // the timed span closes and the stream drains: the copies back to the host, queued before this, have landed; the spans print
  int end() {
    HIPC(hipEventRecord(P->abs_ev[1], st));
    HIPC(hipStreamSynchronize(st));
    float ms = 0; HIPC(hipEventElapsedTime(&ms, P->abs_ev[0], P->abs_ev[1]));
    P->stage_ms[ST_COUNT + EX_TRACEGEN_MS] = ms;
    if (P->set.trace_timing) {
      for (size_t i = 0; i + 1 < marks.size(); i++) { float t = 0; (void)hipEventElapsedTime(&t, marks[i].ev, marks[i + 1].ev); fprintf(stderr, "[device tracegen] %-14s %8.3f ms\n", marks[i + 1].closes, t); }
      for (const Mark& m : marks) (void)hipEventDestroy(m.ev);
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
    P->fixed_match = common_written && P->fixed_f1 > P->fixed_f0;   // by construction: those very kernels wrote the columns
    P->loaded = true;
    return SBN_OK;
  }
};

// G1ExpStark / G2ExpStark (E = 1 / 2)
template <int E>
struct CurveJob : TraceJob {
  static constexpr size_t PW = 16 * E;   // u32 words of a point = u64 words of one instance's output in d_out
  const size_t cw = 257 * 12 * E * K;    // one Jacobian chain of every instance
  const size_t list_words = (IOW * K + 1) / 2, out_words = PW * K + 1;   // pinned staging, u64 words: the list; the outputs + error word
  u64 *ja, *jb, *sv, *inv, *d_out;
  unsigned char* row_op;
  uint32_t *d_ios, *d_prog[2];   // (chain programs: <= 64 levels of 64 micro-operations)
  int* d_err;
  unsigned int* d_cnt;
  u64 *pre, *terms, *scan[2], *carry;  int* err_pre;                // carve_scan()
  size_t np = 0;  u64* jp;  uint32_t* prod;  unsigned char* inf;    // carve_products()
  u64* h_out = nullptr;                                             // ready()
  CurveJob(sbn_prover* P, size_t K) : TraceJob(P, K, 8 * (4 * E + 1)) {   // u32 words per instance: x and offset (2E Fq each) + exp_val
    ja = take(cw); jb = take(cw);
    sv = take(28 * E * n); inv = take(n);
    d_out = take(PW * K);
    row_op = (unsigned char*)take(n / 8 + 1);
    d_ios = (uint32_t*)take(IOW * K / 2 + 1);
    d_prog[0] = (uint32_t*)take(64 * tg::CP_LANES / 2); d_prog[1] = (uint32_t*)take(64 * tg::CP_LANES / 2);
    d_err = (int*)take(1);
    d_cnt = take_histograms();
  }
  // chain offsets: the partial sums of every instance, e_k x_k, the two scan buffers, the flags of the preliminary chains (never read),
  // one carry per block of a list of more than CS_LANES instances
  void carve_scan() {
    pre = take(12 * E * tg::CT_LANES * K); terms = take(12 * E * K); scan[0] = take(12 * E * K); scan[1] = take(12 * E * K); err_pre = (int*)take(1);
    carry = take(12 * E * (K / tg::CS_LANES + 1));
  }
  // un-offset of `count` outputs: the Jacobian products between the two passes of a lane, the affine products ([count][16E] u32), their infinity flags
  void carve_products(size_t count) { np = count; jp = take(12 * E * np); prod = (uint32_t*)take(8 * E * np); inf = (unsigned char*)take(np / 8 + 1); }
  // after the last take().  Pinned staging as the driver lays it out: `in_words` u64 words go up, the outputs + error word land
  // behind them at h_out, `back_words` more behind those at h_back()
  int ready(size_t in_words, size_t back_words = 0) {
    if (int rc = fits()) return rc;
    if (int rc = range_check_setup(P->device)) return rc;
    if (int rc = pinned_reserve(&P->h_io, &P->h_io_words, in_words + out_words + back_words)) return rc;
    h_out = P->h_io + in_words;
    return 0;
  }
  u64* h_back() const { return h_out + out_words; }
  int upload_list(const uint32_t* ios) {   // the whole list, explicit or preliminary
    memcpy(P->h_io, ios, IOW * K * sizeof(uint32_t));
    return begin(P->h_io, d_ios, d_err);
  }
  void common_columns() { launch_common_columns(tg::flags_kernel, d_ios, inv, 65535); }
  // both 256-step chains of every instance on the device, flags into `errw`.  chain_mode (SBN_TRACEGEN_DEVICE_CHAIN; create_ctx
  // picks by the host pool's size): 2 = one wave per instance walking levels of independent Fq operations (tg::chain_coop_kernel),
  // 1 = one lane per instance (tg::chain_kernel, 13 ms), 0 = host_chains()
  int launch_chains(int* errw) {
    if (P->chain_mode == 2) {
      tg::ChainProgDev cp{};
      if (int rc = upload_chain_program(cp)) return rc;
      hipLaunchKernelGGL(tg::chain_coop_kernel<E>, dim3((unsigned)K), dim3(tg::CP_LANES), 0, st, d_ios, K, ja, jb, errw, cp);
    } else hipLaunchKernelGGL(tg::chain_kernel<E>, blocks(K, 64), dim3(64), 0, st, d_ios, K, ja, jb, errw);
    return 0;
  }
  // the chain step as levels of micro-operations (build_chain_program) in d_prog, and the slots the one-wave kernels read and write
  int upload_chain_program(tg::ChainProgDev& cp) {
    static const ChainProgram prog = build_chain_program(E);
    if (prog.levels[0] <= 0 || prog.levels[0] > 24 || prog.levels[1] > 24) return fail(SBN_ERR_UNSUPPORTED, "internal: chain program does not fit");
    for (int b = 0; b < 2; b++) {
      HIPC(hipMemcpyAsync(d_prog[b], prog.ops[b].data(), prog.ops[b].size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      cp.ops[b] = d_prog[b]; cp.levels[b] = prog.levels[b];
    }
    for (int v = 0; v < 4; v++) for (int q = 0; q < E; q++) cp.in_slot[v * E + q] = (unsigned char)((v < 2 ? v : v + 1) * E + q);   // a.X a.Y | b.X b.Y
    cp.one_slot[0] = (unsigned char)(2 * E); cp.one_slot[1] = (unsigned char)(5 * E);
    cp.zero_slot[0] = (unsigned char)(2 * E + 1); cp.zero_slot[1] = (unsigned char)(5 * E + 1);
    for (int i = 0; i < 6 * E; i++) cp.coord[i] = (unsigned char)i;
    return 0;
  }
  // host threads while the device writes the input-independent columns, then a pinned upload
  int host_chains(const uint32_t* ios) {
    if (int rc = pinned_reserve(&P->h_chain, &P->h_chain_words, 2 * cw)) return rc;
    if (tracegen_host_chains(E, ios, K, P->h_chain, P->h_chain + cw)) return fail(SBN_ERR_WITNESS, "degenerate affine operation (x1 == x2 or y == 0)");
    HIPC(hipMemcpyAsync(ja, P->h_chain, cw * sizeof(u64), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(jb, P->h_chain + cw, cw * sizeof(u64), hipMemcpyHostToDevice, st));
    return 0;
  }
  // chain offsets on the device (kernels_tracegen.cuh, "chained instance lists", "segmented chained lists"): the chains of the
  // preliminary list and the partial sums of every instance, then a scan over the list, or over M instances in segments with
  // head d_head_of[k], writes the offsets into d_ios
  int chain_scan(size_t M = 0, const uint32_t* d_head_of = nullptr) {
    if (int rc = chain_terms()) return rc;
    scan_offsets(M, d_head_of, d_err);
    mark("chain_offsets");
    return 0;
  }
  // its two halves: what no start enters (the A chains, the partial sums of every instance and the terms e_k x_k), and the scan from
  // the starts in the offset words of the head rows, an offset at infinity flagged in `errw`
  int chain_terms() {
    if (int rc = launch_chains(err_pre)) return rc;
    hipLaunchKernelGGL(tg::chain_prefix_kernel<E>, dim3((unsigned)K), dim3(tg::CT_LANES), 0, st, d_ios, K, ja, pre, terms);
    return 0;
  }
  void scan_offsets(size_t M, const uint32_t* d_head_of, int* errw) {
    if (K > (size_t)tg::CS_LANES) {   // in blocks of CS_LANES instances: three kernels, ordered by their boundaries
      const size_t real = d_head_of ? M : K;
      hipLaunchKernelGGL(tg::chain_block_scan_kernel<E>, blocks(real, tg::CS_LANES), dim3(tg::CS_LANES), 0, st, d_ios, real, d_head_of, terms, scan[0], scan[1]);
      hipLaunchKernelGGL(tg::chain_block_carry_kernel<E>, dim3(1), dim3(64), 0, st, real, d_head_of, scan[1], carry);
      hipLaunchKernelGGL(tg::chain_block_tail_kernel<E>, blocks((K + tg::TG_INV_BATCH - 1) / tg::TG_INV_BATCH, 64), dim3(64), 0, st, d_ios, K, real, d_head_of, scan[1], carry, scan[0], errw);
    } else if (d_head_of) hipLaunchKernelGGL(tg::chain_seg_scan_kernel<E>, dim3(1), dim3(tg::CS_LANES), 0, st, d_ios, K, M, d_head_of, terms, scan[0], scan[1], errw);
    else hipLaunchKernelGGL(tg::chain_scan_kernel<E>, dim3(1), dim3(tg::CS_LANES), 0, st, d_ios, K, terms, scan[0], scan[1], errw);
  }
  // complete sums, one round: the failing segments of the round before start from their next candidate (d_choice: one index per
  // segment), the scan and the rebase run again, and every segment with a bad event of the table's walk gets a status word; the
  // words come back to h_status and the stream drains.  The offset-at-infinity flag of the scan goes to the word nobody reads
  // (err_pre): the status kernel finds that event as the output at infinity of the instance before.
  int choice_round(bool restart, size_t M, size_t S, const uint32_t* d_head_of, const uint32_t* d_seg_head, const uint32_t* d_seg_of, const uint32_t* d_choice,
                   const uint32_t* d_candidates, int* d_status, int* h_status) {
    HIPC(hipMemsetAsync(d_status, 0, S * sizeof(int), st));
    if (restart) hipLaunchKernelGGL(tg::chain_seg_start_kernel<E>, blocks(S * PW, 256), dim3(256), 0, st, d_ios, S, d_seg_head, d_choice, d_candidates);
    scan_offsets(M, d_head_of, err_pre);
    hipLaunchKernelGGL(tg::chain_rebase_kernel<E>, blocks(K * 257, 64), dim3(64), 0, st, d_ios, K, pre, jb);
    hipLaunchKernelGGL(tg::chain_seg_status_kernel<E>, blocks(M * 257, 256), dim3(256), 0, st, d_ios, M, ja, jb, d_seg_of, d_status);
    HIPC(hipMemcpyAsync(h_status, d_status, S * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    HIPC(hipGetLastError());
    return 0;
  }
  void rebase() {   // the chain of b onto the derived offsets; A is in ja already
    hipLaunchKernelGGL(tg::chain_rebase_kernel<E>, blocks(K * 257, 64), dim3(64), 0, st, d_ios, K, pre, jb);
    mark("chains");
  }
  void affine_lambda() {
    hipLaunchKernelGGL(tg::affine_lambda_kernel<E>, blocks((n + tg::TG_ROWS - 1) / tg::TG_ROWS, 64), dim3(64), 0, st, d_ios, K, ja, jb, n, sv, row_op, d_out, d_err);
    mark("affine+lambda");
  }
  // output + (-offset) of np instances from what affine_lambda() left in d_out: of instance i, or output d_out_at[i] and the offset
  // of instance d_off_at[i]
  void un_offset(const uint32_t* d_out_at = nullptr, const uint32_t* d_off_at = nullptr) {
    hipLaunchKernelGGL(tg::scalar_mul_unoffset_kernel<E>, blocks((np + tg::TG_INV_BATCH - 1) / tg::TG_INV_BATCH, 64), dim3(64), 0, st, d_ios, np, d_out, jp, prod, inf, d_out_at, d_off_at);
    mark("un_offset");
  }
  // the last launches; the outputs and the error word come back
  int witness_and_range_check() {
    hipLaunchKernelGGL(tg::gadget_witness_kernel<E>, blocks(3 * E * n, 256), dim3(256), 0, st, sv, row_op, n, sh.gadget_col, P->d_trace, d_err);
    mark("row_witness");
    if (int rc = launch_u16_range_check(d_cnt, d_err)) return rc;
    HIPC(hipMemcpyAsync(h_out, d_out, PW * K * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(h_out + PW * K, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    return 0;
  }
  int download_list(u64* h_list) {   // the list as the device derived it
    HIPC(hipMemcpyAsync(h_list, d_ios, IOW * K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return 0;
  }
  int download_products(u64* h_prod) {   // the flags land 8E * np u64 words behind the products
    HIPC(hipMemcpyAsync(h_prod, prod, PW * np * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(h_prod + 8 * E * np, inf, np, hipMemcpyDeviceToHost, st));
    return 0;
  }
  int error_word() const { return (int)(h_out[PW * K] & 0xffffffffu); }   // after publish()
  // the span closes; public inputs: x, offset, exp_val, output as u32 limbs (g1/exp.rs:124-135, g2/exp.rs:139-156); `ios` to ios_out
  int publish(const uint32_t* ios, uint64_t* pi_out, uint32_t* ios_out = nullptr) {
    if (int rc = end()) return rc;
    const int rc = finish(error_word(), pi_out, [&](size_t k, u64* p) {
      for (size_t i = 0; i < IOW; i++) p[i] = ios[IOW * k + i];
      for (size_t i = 0; i < PW; i++) p[IOW + i] = h_out[PW * k + i];
    });
    if (rc == SBN_OK && ios_out) memcpy(ios_out, ios, IOW * K * sizeof(uint32_t));
    return rc;
  }
};

template <int E>
static int curve_trace_explicit(sbn_prover* P, const uint32_t* ios, size_t K, uint64_t* pi_out) {
  CurveJob<E> J(P, K);
  if (int rc = check_below_p(ios, J.IOW, 4 * E, K, "coordinate")) return rc;
  HIPC(hipSetDevice(P->device));
  if (int rc = J.ready(J.list_words)) return rc;
  if (int rc = J.upload_list(ios)) return rc;
  J.common_columns();
  if (int rc = P->chain_mode ? J.launch_chains(J.d_err) : J.host_chains(ios)) return rc;
  J.mark("chains");
  J.affine_lambda();
  if (int rc = J.witness_and_range_check()) return rc;
  return J.publish(ios, pi_out);
}

// chained: x, start, exp_val of every instance go up; the device rewrites the offsets and the derived list comes back behind the
// outputs.  Only chain_mode 1 and 2 come here, as to the two drivers below.
template <int E>
static int curve_trace_chained(sbn_prover* P, const ChainedIn& ch, size_t K, uint64_t* pi_out) {
  if (int rc = chain_terms_check_curve(E, ch.terms, K, ch.start)) return rc;
  const std::vector<uint32_t> prelim = preliminary_list(ch, K, 16 * E, 8, ch.start);
  HIPC(hipSetDevice(P->device));
  CurveJob<E> J(P, K);
  J.carve_scan();
  if (int rc = J.ready(J.list_words, J.list_words)) return rc;
  if (int rc = J.upload_list(prelim.data())) return rc;
  if (int rc = J.chain_scan()) return rc;
  J.common_columns();
  J.rebase();
  J.affine_lambda();
  if (int rc = J.witness_and_range_check()) return rc;
  if (int rc = J.download_list(J.h_back())) return rc;
  return J.publish((const uint32_t*)J.h_back(), pi_out, ch.ios_out);
}

// scalar multiplications: the host keeps its own explicit list for the public inputs; only the compact form (points, scalars,
// offset) goes up, and the products and their flags come back behind the outputs
template <int E>
static int curve_trace_scalar_muls(sbn_prover* P, const ScalarMulIn& sm, size_t K, uint64_t* pi_out) {
  if (int rc = scalar_mul_check_points(E, sm.points, K, sm.offset)) return rc;
  CurveJob<E> J(P, K);
  std::vector<uint32_t> ios(J.IOW * K);
  scalar_mul_explicit_list(E, sm.points, sm.scalars, sm.scalar_count, K, K, sm.offset, ios.data());
  HIPC(hipSetDevice(P->device));
  const size_t pts = 16 * E * K, cin_words = pts + 8 * sm.scalar_count + 16 * E;   // u32 words: the points, the compact upload
  uint32_t* d_cin = (uint32_t*)J.take(cin_words / 2 + 1);
  J.carve_products(K);
  if (int rc = J.ready((cin_words + 1) / 2, 8 * E * K + (K + 7) / 8)) return rc;
  uint32_t* h = (uint32_t*)P->h_io;
  memcpy(h, sm.points, pts * sizeof(uint32_t));
  memcpy(h + pts, sm.scalars, 8 * sm.scalar_count * sizeof(uint32_t));
  memcpy(h + pts + 8 * sm.scalar_count, sm.offset, 16 * E * sizeof(uint32_t));
  if (int rc = J.begin(h, d_cin, J.d_err, cin_words)) return rc;
  hipLaunchKernelGGL(tg::scalar_mul_list_kernel<E>, blocks(J.IOW * K, 256), dim3(256), 0, J.st, d_cin, K, sm.scalar_count, J.d_ios);
  J.mark("scalar_list");
  J.common_columns();
  if (int rc = J.launch_chains(J.d_err)) return rc;
  J.mark("chains");
  J.affine_lambda();
  J.un_offset();
  if (int rc = J.witness_and_range_check()) return rc;
  if (int rc = J.download_products(J.h_back())) return rc;
  const int rc = J.publish(ios.data(), pi_out, sm.ios_out);
  if (rc == SBN_ERR_WITNESS && (J.error_word() & tg::TG_ERR_DEGENERATE)) {
    // the kernels report an error word only: the host walk names the first instance the table cannot walk (error path)
    if (int named = scalar_mul_name_degenerate(E, ios.data(), K)) return named;
    return fail(SBN_ERR_WITNESS, "degenerate affine operation (x1 == x2 or y == 0)");
  }
  if (rc == SBN_OK && sm.products_out) memcpy(sm.products_out, J.h_back(), pts * sizeof(uint32_t));
  if (rc == SBN_OK && sm.infinity_out) memcpy(sm.infinity_out, J.h_back() + 8 * E * K, K);
  return rc;
}

// segmented: x, the start of its segment, exp_val of every instance go up with three index arrays (aux: the head of every lane's
// segment [K], then tail and head per segment); the derived list comes back behind the outputs, the sums final + (-start) and
// their flags behind the list.  Complete sums (mb.choice): three more arrays behind those (the segment of every instance [K], the
// start candidates [8][16E], the choice of every segment [S]); the offsets are derived in rounds (CurveJob::choice_round) until no
// segment reports a bad event, then the stages run on as for the caller's starts.
template <int E>
static int curve_trace_segmented(sbn_prover* P, const BatchIn& mb, size_t K, uint64_t* pi_out) {
  if (int rc = msm_batch_check_inputs(P->air.kind, mb.terms, mb.lengths, mb.segments, mb.starts, mb.start_count, mb.M)) return rc;
  const size_t S = mb.segments, W = 16 * E;
  const bool pick = mb.choice != nullptr;
  std::vector<uint32_t> aux, seg_head, seg_len;
  const std::vector<uint32_t> prelim = preliminary_list(mb.terms, mb.lengths, S, mb.M, K, W, 8, [&](size_t s) { return mb.starts + (mb.start_count == 1 ? 0 : W * s); },
                                                        seg_head, seg_len, &aux);
  for (size_t s = 0; s < S; s++) aux.push_back(seg_head[s] + seg_len[s] - 1);
  aux.insert(aux.end(), seg_head.begin(), seg_head.end());
  const size_t seg_of_at = aux.size(), cand_at = seg_of_at + K, choice_at = cand_at + SBN_START_CANDIDATES * W;
  if (pick) {
    aux.resize(choice_at + S, 0);
    for (size_t s = 0; s < S; s++) for (size_t g = seg_head[s]; g < seg_head[s] + seg_len[s]; g++) aux[seg_of_at + g] = (uint32_t)s;
    for (unsigned j = 0; j < SBN_START_CANDIDATES; j++) memcpy(&aux[cand_at + W * j], curve_start_candidate_words(E, j), W * sizeof(uint32_t));
  }
  HIPC(hipSetDevice(P->device));
  CurveJob<E> J(P, K);
  J.carve_scan();
  J.carve_products(S);
  uint32_t* d_aux = (uint32_t*)J.take(aux.size() / 2 + 1);
  int* d_status = pick ? (int*)J.take(S / 2 + 1) : nullptr;
  if (int rc = J.ready(J.list_words, J.list_words + 8 * E * S + (S + 7) / 8 + (pick ? S / 2 + 1 : 0))) return rc;
  const uint32_t* ios = (const uint32_t*)J.h_back();
  u64* const h_sums = J.h_back() + J.list_words;
  if (int rc = J.upload_list(prelim.data())) return rc;
  HIPC(hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice, J.st));
  if (!pick) { if (int rc = J.chain_scan(mb.M, d_aux)) return rc; }
  else {
    int* h_status = (int*)(h_sums + 8 * E * S + (S + 7) / 8);
    if (int rc = J.chain_terms()) return rc;
    for (bool restart = false;; restart = true) {
      if (restart) HIPC(hipMemcpyAsync(d_aux + choice_at, &aux[choice_at], S * sizeof(uint32_t), hipMemcpyHostToDevice, J.st));
      if (int rc = J.choice_round(restart, mb.M, S, d_aux, d_aux + K + S, d_aux + seg_of_at, d_aux + choice_at, d_aux + cand_at, d_status, h_status)) return rc;
      bool failed = false, exhausted = false;
      for (size_t s = 0; s < S; s++)
        if (h_status[s]) { failed = true; if (++aux[choice_at + s] == SBN_START_CANDIDATES) exhausted = true; }
      if (!failed) break;
      if (exhausted) {   // the host derivation words the refusal: the segment, how many there are, the instance candidate 7 fails at
        if (int why = msm_batch_complete_choose(P->air.kind, mb.terms, mb.lengths, S, mb.M, K, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return why;
        return fail(SBN_ERR_WITNESS, "the device refuses every start candidate of a segment the host derivation takes");
      }
    }
    J.mark("chain_offsets");
    for (size_t s = 0; s < S; s++) {
      mb.choice[s] = (uint8_t)aux[choice_at + s];
      memcpy(mb.starts_out + W * s, curve_start_candidate_words(E, aux[choice_at + s]), W * sizeof(uint32_t));
    }
  }
  J.common_columns();
  if (!pick) J.rebase();   // (the rounds of the complete sums end with the rebase of the chosen starts)
  J.affine_lambda();
  J.un_offset(d_aux + K, d_aux + K + S);   // final_s + (-start_s): indexed by the tail and the head of every segment
  if (int rc = J.witness_and_range_check()) return rc;
  if (int rc = J.download_list(J.h_back())) return rc;
  if (int rc = J.download_products(h_sums)) return rc;
  const int rc = J.publish(ios, pi_out, mb.ios_out);
  if (rc == SBN_ERR_WITNESS && !pick && (J.error_word() & (tg::TG_ERR_INFINITY | tg::TG_ERR_DEGENERATE))) {
    // the kernels report an error word only: the host derivation names the instance and its segment (error path)
    std::vector<uint32_t> named(J.IOW * K);
    if (int why = msm_batch_derive(P->air.kind, mb.terms, mb.lengths, S, mb.starts, mb.start_count, mb.M, K, named.data(), nullptr, nullptr, nullptr)) return why;
  }
  if (rc == SBN_OK && mb.finals_out)   // the instance outputs at the segment tails: one u32 limb per u64 word
    for (size_t s = 0; s < S; s++) for (int i = 0; i < 16 * E; i++) mb.finals_out[16 * E * s + i] = (uint32_t)J.h_out[16 * E * aux[K + s] + i];
  if (rc == SBN_OK && mb.sums_out) memcpy(mb.sums_out, h_sums, 16 * E * S * sizeof(uint32_t));
  if (rc == SBN_OK && mb.infinity_out) memcpy(mb.infinity_out, h_sums + 8 * E * S, S);
  return rc;
}

// programs: the literals, the start (candidate 0) and the exponents of every node go up in place (zeros where a link will be
// resolved; a pad row repeats the node words of node count - 1 and runs as one more node of its level) with the node table and
// the nodes sorted by level; per level one launch walks the chains and a status kernel behind it writes the affine outputs the
// next level links to and the one status word (kernels_tracegen.cuh, "curve programs").  The host derives the negated blinds
// while the levels run, reads the status word and uploads them; the values out + (-blind) are computed where the scalar
// multiplications compute their products, and outputs, values and the derived list come back in the one download.
// *fallback (with SBN_OK, nothing loaded): a node has a bad event under candidate 0; the caller derives on the host pool.
template <int E>
static int curve_trace_program(sbn_prover* P, const CurveProgramIn& pr, const ProgramPlan& plan, size_t K, uint64_t* pi_out, bool* fallback) {
  const size_t W = 16 * E, M = pr.count;
  ProgramPlan rows;   // the schedule of all K rows: a pad runs as one more node of the level of node M - 1
  curve_host::fill_plan(plan.level.data(), M, K, rows);
  const std::vector<uint32_t>& start = rows.level_start;
  std::vector<uint32_t> aux;   // the node table [K][3], then the order [K]
  const std::vector<uint32_t> prelim = program_prelim(pr.nodes, M, K, W, 8, pr.points, pr.exps, SBN_NODE_START, curve_start_candidate_words(E, 0), rows.order, aux);
  HIPC(hipSetDevice(P->device));
  CurveJob<E> J(P, K);
  J.carve_products(M);
  uint32_t* d_aux = (uint32_t*)J.take(2 * K + 1);
  uint32_t* d_pout = (uint32_t*)J.take(8 * E * K + 1);       // the affine outputs the links read: [K][16E] u32
  uint32_t* d_neg = (uint32_t*)J.take(8 * E * M + 1);        // -T of every node, and whether T is the point at infinity
  unsigned char* d_tinf = (unsigned char*)J.take(M / 8 + 1);
  int* d_status = (int*)J.take(1);                           // [0]: the status word; [1]: the chains' own flags, which nobody reads
  const size_t blind_words = 8 * E * M + (M + 7) / 8;        // pinned, u64 words: the list, then -T and its flags go up; the
  if (int rc = J.ready(J.list_words + blind_words, J.list_words + blind_words + 1)) return rc;   // list, the values and their flags, the status word come back
  uint32_t* h_neg = (uint32_t*)(P->h_io + J.list_words);
  uint8_t* h_tinf = (uint8_t*)(P->h_io + J.list_words + 8 * E * M);
  const uint32_t* ios = (const uint32_t*)J.h_back();
  u64* const h_vals = J.h_back() + J.list_words;
  int* const h_status = (int*)(h_vals + blind_words);
  if (int rc = J.upload_list(prelim.data())) return rc;
  HIPC(hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice, J.st));
  HIPC(hipMemsetAsync(d_status, 0, 2 * sizeof(int), J.st));
  tg::ChainProgDev cp{};
  if (P->chain_mode == 2) if (int rc = J.upload_chain_program(cp)) return rc;
  for (size_t l = 0; l < rows.depth(); l++) {   // the kernel boundary between two levels is the link: level l reads what levels < l stored
    const size_t cnt = start[l + 1] - start[l];
    const uint32_t* d_order = d_aux + 3 * K + start[l];
    if (P->chain_mode == 2) hipLaunchKernelGGL(tg::curve_program_level_coop_kernel<E>, dim3((unsigned)cnt), dim3(tg::CP_LANES), 0, J.st, J.d_ios, d_aux, d_order, J.ja, J.jb, d_pout, d_status + 1, cp);
    else hipLaunchKernelGGL(tg::curve_program_level_kernel<E>, blocks(cnt, 64), dim3(64), 0, J.st, J.d_ios, d_aux, d_order, cnt, J.ja, J.jb, d_pout, d_status + 1);
    hipLaunchKernelGGL(tg::curve_program_status_kernel<E>, blocks(cnt * 257, 256), dim3(256), 0, J.st, J.d_ios, d_order, cnt, J.ja, J.jb, d_pout, d_status);
  }
  J.mark("curve_program_levels");
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(h_status, d_status, sizeof(int), hipMemcpyDeviceToHost, J.st));
  curve_program_neg_blinds(E, plan, pr.nodes, pr.exps, 0, h_neg, h_tinf);   // on the host pool, while the levels run
  HIPC(hipStreamSynchronize(J.st));
  if (*h_status) { *fallback = true; return J.end(); }
  HIPC(hipMemcpyAsync(d_neg, h_neg, W * M * sizeof(uint32_t), hipMemcpyHostToDevice, J.st));
  HIPC(hipMemcpyAsync(d_tinf, h_tinf, M, hipMemcpyHostToDevice, J.st));
  J.common_columns();
  J.affine_lambda();
  hipLaunchKernelGGL(tg::curve_program_values_kernel<E>, blocks((M + tg::TG_INV_BATCH - 1) / tg::TG_INV_BATCH, 64), dim3(64), 0, J.st, M, J.d_out, d_neg, d_tinf, J.jp, J.prod, J.inf);
  J.mark("curve_program_values");
  if (int rc = J.witness_and_range_check()) return rc;
  if (int rc = J.download_list(J.h_back())) return rc;
  if (int rc = J.download_products(h_vals)) return rc;
  const int rc = J.publish(ios, pi_out, pr.ios_out);
  if (rc == SBN_OK && pr.outs_out)   // the instance outputs: one u32 limb per u64 word
    for (size_t i = 0; i < W * M; i++) pr.outs_out[i] = (uint32_t)J.h_out[i];
  if (rc == SBN_OK && pr.values_out) memcpy(pr.values_out, h_vals, W * M * sizeof(uint32_t));
  if (rc == SBN_OK && pr.infinity_out) memcpy(pr.infinity_out, h_vals + 8 * E * M, M);
  return rc;
}

// Fq12ExpStark / Fq12ExpU64Stark: the square-and-multiply chains (no inversion anywhere) in standard form, then one lane per
// (row, output coefficient) for the limb columns and the twelve modular-gadget witnesses, and the split range check per target column.
struct Fq12Job : TraceJob {
  const bool u64e;            // 128-row instances, one-element exponent
  const int steps, log_rpb;
  const size_t cw;            // one chain of every instance, standard form
  u64 *ca, *cb, *inv, *d_outs;
  uint32_t* d_ios;
  int* d_err;
  int err = 0;                // the kernels' error word and what came back from d_outs on, after publish()
  std::vector<u64> h_outs;
  Fq12Job(sbn_prover* P, size_t K)
      : TraceJob(P, K, P->air.kind == SBN_AIR_FQ12_EXP_U64 ? 194 : 200), u64e(IOW == 194), steps(u64e ? 64 : 256), log_rpb(u64e ? 7 : 9), cw((size_t)(steps + 1) * 48 * K) {
    ca = take(cw); cb = take(cw);
    inv = take(n);
    d_outs = take(K * 48 + IOW * K / 2 + 1);   // the outputs and, right behind them, the list: ONE block, so that a source whose
    d_ios = (uint32_t*)(d_outs + K * 48);      // list is derived in place (the towers) takes both back in one download
    d_err = (int*)take(1);
  }
  // after the last take(): the list that goes up is canonical (coefficients below p, a u64 exponent below the Goldilocks prime), the
  // scratch fits; the timed span opens
  int upload_list(const uint32_t* ios) {
    if (int rc = check_below_p(ios, IOW, 24, K, "coefficient")) return rc;
    HIPC(hipSetDevice(P->device));
    if (u64e)
      for (size_t k = 0; k < K; k++)
        if (((u64)ios[IOW * k + 192] | ((u64)ios[IOW * k + 193] << 32)) >= GLP) return fail(SBN_ERR_NON_CANONICAL, "exponent of instance %zu is not a canonical field element", k);
    if (int rc = fits()) return rc;
    return begin(ios, d_ios, d_err);
  }
  void common_columns() {
    if (u64e) launch_common_columns(tg::flags_u64_kernel, d_ios, inv, 255);
    else launch_common_columns(tg::flags_kernel, d_ios, inv, 255);
  }
  // one workgroup per instance (kernels_tracegen.cuh fq12_chain_kernel): the chains, and B[steps] of every instance in d_outs
  void device_chains() {
    hipLaunchKernelGGL(tg::fq12_chain_kernel, dim3((unsigned)K), dim3(320), 0, st, d_ios, IOW, steps, ca, cb, d_outs);
    mark("chains");
  }
  // SBN_FQ12_HOST_CHAIN=1: the library's host threads + a pinned upload, as in round 2 (A/B); the outputs stay in P->h_chain
  int host_chains(const uint32_t* ios) {
    if (int rc = pinned_reserve(&P->h_chain, &P->h_chain_words, 2 * cw)) return rc;
    tracegen_host_chains_fq12(ios, IOW, steps, K, P->h_chain, P->h_chain + cw);
    HIPC(hipMemcpyAsync(ca, P->h_chain, 2 * cw * sizeof(u64), hipMemcpyHostToDevice, st));  // ca and cb are adjacent
    mark("chains");
    return 0;
  }
  // chain offsets (kernels_tracegen.cuh, "chained instance lists"): the chains ran on offsets of one, so x^e of every instance is in
  // d_outs; the driver's running product has written the offsets into d_ios and the chain of b is rebased onto them
  void rebase() {
    hipLaunchKernelGGL(tg::fq12_rebase_kernel, dim3((unsigned)(K * (size_t)(steps + 1))), dim3(192), 0, st, d_ios, IOW, steps, cb, d_outs);
    mark("chain_offsets");
  }
  // the last launches (one lane per (row, output coefficient) by default; SBN_FQ12_ROW_KERNEL=1: round 2's one lane per row, A/B);
  // the error word comes back and `words` u64 words from d_outs on: B[steps] of every instance, K * 48, or the list as well
  int witness_and_range_check(size_t words) {
    if (P->set.fq12_row_kernel) hipLaunchKernelGGL(tg::fq12_row_kernel, blocks(n, 64), dim3(64), 0, st, d_ios, IOW, log_rpb, ca, cb, n, P->d_trace, d_err);
    else hipLaunchKernelGGL(tg::fq12_gadget_kernel, blocks(12 * n, 256), dim3(256), 0, st, d_ios, IOW, log_rpb, ca, cb, n, P->d_trace, d_err);
    mark("row_witness");
    hipLaunchKernelGGL(tg::split_range_check_kernel, dim3((unsigned)sh.num_rc), dim3(256), 0, st, P->d_trace, n, sh.rc_start, sh.start_lookups, d_err);
    mark("range_check");
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    h_outs.resize(words);
    if (words) HIPC(hipMemcpyAsync(h_outs.data(), d_outs, words * sizeof(u64), hipMemcpyDeviceToHost, st));
    return 0;
  }
  int download_list(std::vector<uint32_t>& h_list) {   // the list as the device derived it
    h_list.resize(IOW * K);
    HIPC(hipMemcpyAsync(h_list.data(), d_ios, IOW * K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return 0;
  }
  // the span closes; public inputs: x, offset as 16-bit limbs, exp_val, output = b at the last row (fq12/exp.rs:95-117), the 48
  // words at outs + stride * k for instance k; `ios` to ios_out
  int publish(const uint32_t* ios, const u64* outs, size_t stride, uint64_t* pi_out, uint32_t* ios_out = nullptr) {
    if (int rc = end()) return rc;
    const int rc = finish(err, pi_out, [&](size_t k, u64* p) {
      for (int c = 0; c < 24; c++)
        for (int i = 0; i < 16; i++) p[16 * c + i] = (ios[IOW * k + 8 * c + (i >> 1)] >> (16 * (i & 1))) & 0xffff;
      if (u64e) p[384] = (u64)ios[IOW * k + 192] | ((u64)ios[IOW * k + 193] << 32);
      else for (int i = 0; i < 8; i++) p[384 + i] = ios[IOW * k + 192 + i];
      const u64* out = outs + stride * k;
      const int ob = 384 + sh.n_exp_slots;
      for (int c = 0; c < 12; c++) for (int i = 0; i < 16; i++) p[ob + 16 * c + i] = (out[4 * c + (i >> 2)] >> (16 * (i & 3))) & 0xffff;
    });
    if (rc == SBN_OK && ios_out) memcpy(ios_out, ios, IOW * K * sizeof(uint32_t));
    return rc;
  }
};

static int fq12_trace_explicit(sbn_prover* P, const uint32_t* ios, size_t K, uint64_t* pi_out) {
  Fq12Job J(P, K);
  if (int rc = J.upload_list(ios)) return rc;
  J.common_columns();
  if (!P->set.fq12_host_chain) {
    J.device_chains();
    if (int rc = J.witness_and_range_check(K * 48)) return rc;
    return J.publish(ios, J.h_outs.data(), 48, pi_out);
  }
  if (int rc = J.host_chains(ios)) return rc;
  if (int rc = J.witness_and_range_check(0)) return rc;
  return J.publish(ios, P->h_chain + J.cw + (size_t)J.steps * 48, (size_t)(J.steps + 1) * 48, pi_out);   // B[steps] of the uploaded chains
}

// chained: x, one, exp_val of every instance go up; a running product from `start` writes the offsets and the derived list comes
// back.  Only device chains come here, as to the two drivers below.
static int fq12_trace_chained(sbn_prover* P, const ChainedIn& ch, size_t K, uint64_t* pi_out) {
  if (int rc = check_below_p(ch.start, 96, 12, 1, "coefficient of start")) return rc;
  Fq12Job J(P, K);
  const uint32_t one[96] = {1};
  const std::vector<uint32_t> prelim = preliminary_list(ch, K, 96, J.IOW - 192, one);
  std::vector<uint32_t> ios;
  uint32_t* d_start = (uint32_t*)J.take(48);
  if (int rc = J.upload_list(prelim.data())) return rc;
  HIPC(hipMemcpyAsync(d_start, ch.start, 96 * sizeof(uint32_t), hipMemcpyHostToDevice, J.st));
  J.common_columns();
  J.device_chains();
  hipLaunchKernelGGL(tg::fq12_offset_scan_kernel, dim3(1), dim3(192), 0, J.st, J.d_ios, J.IOW, K, d_start, J.d_outs);
  J.rebase();
  if (int rc = J.witness_and_range_check(K * 48)) return rc;
  if (int rc = J.download_list(ios)) return rc;
  return J.publish(ios.data(), J.h_outs.data(), 48, pi_out, ch.ios_out);
}

// segmented: x, one, exp_val of every instance (a pad row repeats row M - 1) go up with aux = head[S], len[S] and the starts
// ([start_count][96]); one workgroup per segment walks its own running product and the derived list comes back
static int fq12_trace_segmented(sbn_prover* P, const BatchIn& mb, size_t K, uint64_t* pi_out) {
  if (int rc = msm_batch_check_inputs(P->air.kind, mb.terms, mb.lengths, mb.segments, mb.starts, mb.start_count, mb.M)) return rc;
  Fq12Job J(P, K);
  const size_t S = mb.segments;
  const uint32_t one[96] = {1};
  std::vector<uint32_t> aux, seg_len, ios;
  const std::vector<uint32_t> prelim = preliminary_list(mb.terms, mb.lengths, S, mb.M, K, 96, J.IOW - 192, [&](size_t) { return one; }, aux, seg_len);
  aux.insert(aux.end(), seg_len.begin(), seg_len.end());
  aux.insert(aux.end(), mb.starts, mb.starts + 96 * mb.start_count);
  uint32_t* d_aux = (uint32_t*)J.take(aux.size() / 2 + 1);
  if (int rc = J.upload_list(prelim.data())) return rc;
  HIPC(hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice, J.st));
  J.common_columns();
  J.device_chains();
  hipLaunchKernelGGL(tg::fq12_seg_scan_kernel, dim3((unsigned)S), dim3(192), 0, J.st, J.d_ios, J.IOW, K, mb.M, d_aux, d_aux + S, d_aux + 2 * S, mb.start_count, J.d_outs);
  J.rebase();
  if (int rc = J.witness_and_range_check(K * 48)) return rc;
  if (int rc = J.download_list(ios)) return rc;
  const int rc = J.publish(ios.data(), J.h_outs.data(), 48, pi_out, mb.ios_out);
  if (rc == SBN_OK && mb.finals_out)   // [segments][96] u32 = the outputs of the segment tails, standard form
    for (size_t s = 0; s < S; s++) {
      const u64* out = J.h_outs.data() + 48 * (size_t)(aux[s] + aux[S + s] - 1);
      for (size_t i = 0; i < 48; i++) { mb.finals_out[96 * s + 2 * i] = (uint32_t)out[i]; mb.finals_out[96 * s + 2 * i + 1] = (uint32_t)(out[i] >> 32); }
    }
  return rc;
}

// towers: x of level 0, zeros above it (the device writes them), one and the tower's exponent go up, a pad row repeating row
// M - 1; one workgroup per tower links and walks its levels, the pads are filled behind them, and the outputs (= the powers) come
// back together with the derived list in one download: the job carved them as one block
static int fq12_trace_towers(sbn_prover* P, const PowerIn& pw, size_t K, uint64_t* pi_out) {
  if (int rc = power_check_inputs(P->air.kind, pw.bases, pw.exps, pw.exp_count, pw.count)) return rc;
  Fq12Job J(P, K);
  const size_t IOW = J.IOW, ew = IOW - 192, M = pw.count * pw.depth;   // M real instances; rows [M, K) are pads
  std::vector<uint32_t> prelim(IOW * K, 0u);
  for (size_t g = 0; g < K; g++) {
    const size_t r = g < M ? g : M - 1, k = r / pw.depth;
    uint32_t* io = prelim.data() + IOW * g;
    if (r % pw.depth == 0) memcpy(io, pw.bases + 96 * k, 96 * sizeof(uint32_t));
    io[96] = 1;
    memcpy(io + 192, pw.exps + (pw.exp_count == 1 ? 0 : ew * k), ew * sizeof(uint32_t));
  }
  if (int rc = J.upload_list(prelim.data())) return rc;
  J.common_columns();
  hipLaunchKernelGGL(tg::fq12_tower_kernel, dim3((unsigned)pw.count), dim3(320), 0, J.st, J.d_ios, IOW, J.steps, pw.depth, J.ca, J.cb, J.d_outs);
  J.mark("tower_links");
  if (M < K) hipLaunchKernelGGL(tg::fq12_tower_pad_kernel, dim3((unsigned)(K - M)), dim3(256), 0, J.st, J.d_ios, IOW, M, K, (size_t)(J.steps + 1) * 48, J.ca, J.cb, J.d_outs);
  J.mark("tower_pads");
  if (int rc = J.witness_and_range_check(K * 48 + (IOW * K + 1) / 2)) return rc;
  const int rc = J.publish((const uint32_t*)(J.h_outs.data() + K * 48), J.h_outs.data(), 48, pi_out, pw.ios_out);
  if (rc == SBN_OK && pw.powers_out)   // [count][depth][96] u32 = the outputs of the M real instances, standard form
    for (size_t i = 0; i < 48 * M; i++) { pw.powers_out[2 * i] = (uint32_t)J.h_outs[i]; pw.powers_out[2 * i + 1] = (uint32_t)(J.h_outs[i] >> 32); }
  return rc;
}

// programs: the literals, ones and exponents of every node go up in place (zeros where a link will be resolved; a pad row repeats
// row count - 1) with the node table and the nodes sorted by level; one launch per level, one workgroup per node of that level,
// resolves the links from the outputs of earlier launches and walks the chains (kernels_tracegen.cuh, "field programs"), the pads
// are filled behind them, and the outputs come back together with the derived list in one download, as for the towers.  A mapped
// operand (pr.maps) goes into the table of the pre-pass of its level -- (node, field, source node, map), level by level -- and is a
// literal (zero words, bit 31 clear) in the device copy of the node table: the pre-pass launched in front of that level's launch
// writes the mapped words into the node's row, and the level kernel, unchanged, loads them from there.
static int fq12_trace_program(sbn_prover* P, const ProgramIn& pr, const ProgramPlan& plan, size_t K, uint64_t* pi_out) {
  Fq12Job J(P, K);
  const size_t IOW = J.IOW, M = pr.count;   // M real instances; rows [M, K) are pads
  const uint32_t one[96] = {1};
  std::vector<uint32_t> aux;                // the node table [K][3], then the order [M]: the pads are filled, not walked
  const std::vector<uint32_t> prelim = program_prelim(pr.nodes, M, K, 96, IOW - 192, pr.values, pr.exps, SBN_NODE_ONE, one, plan.order, aux);
  const size_t map_at = aux.size();         // behind them the table of the pre-passes, [4] per mapped operand, level by level
  std::vector<size_t> map_start(plan.depth() + 1, 0);
  for (size_t l = 0; l < plan.depth() && pr.maps; l++) {
    for (size_t i = plan.level_start[l]; i < plan.level_start[l + 1]; i++) {
      const uint32_t g = plan.order[i], op[2] = {pr.nodes[g].x, pr.nodes[g].offset};
      for (uint32_t f = 0; f < 2; f++)
        if (const unsigned m = curve_host::map_of(pr.maps, g, (int)f)) {
          aux.insert(aux.end(), {g, f, curve_host::link_of(op[f]), (uint32_t)m});
          for (size_t r = g; r < (g + 1 == M ? K : g + 1); r++) aux[3 * r + f] = 0;   // (a pad repeats the table row of node M - 1; nothing walks it)
        }
    }
    map_start[l + 1] = (aux.size() - map_at) / 4;
  }
  uint32_t* d_aux = (uint32_t*)J.take(aux.size() / 2 + 1);
  if (int rc = J.upload_list(prelim.data())) return rc;
  HIPC(hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice, J.st));
  J.common_columns();
  for (size_t l = 0; l < plan.depth(); l++) {   // the kernel boundary between two levels is the link: level l reads what levels < l stored
    if (pr.maps && map_start[l + 1] > map_start[l])
      hipLaunchKernelGGL(tg::fq12_program_map_kernel, dim3((unsigned)(map_start[l + 1] - map_start[l])), dim3(64), 0, J.st, J.d_ios, IOW, d_aux + map_at + 4 * map_start[l], J.d_outs);
    hipLaunchKernelGGL(tg::fq12_program_level_kernel, dim3((unsigned)(plan.level_start[l + 1] - plan.level_start[l])), dim3(320), 0, J.st, J.d_ios, IOW, J.steps,
                       d_aux, d_aux + 3 * K + plan.level_start[l], J.ca, J.cb, J.d_outs);
  }
  J.mark("program_levels");
  if (M < K) hipLaunchKernelGGL(tg::fq12_tower_pad_kernel, dim3((unsigned)(K - M)), dim3(256), 0, J.st, J.d_ios, IOW, M, K, (size_t)(J.steps + 1) * 48, J.ca, J.cb, J.d_outs);
  J.mark("program_pads");
  if (int rc = J.witness_and_range_check(K * 48 + (IOW * K + 1) / 2)) return rc;
  const int rc = J.publish((const uint32_t*)(J.h_outs.data() + K * 48), J.h_outs.data(), 48, pi_out, pr.ios_out);
  if (rc == SBN_OK && pr.outs_out)   // [count][96] u32 = the outputs of the M real instances, standard form
    for (size_t i = 0; i < 48 * M; i++) { pr.outs_out[2 * i] = (uint32_t)J.h_outs[i]; pr.outs_out[2 * i + 1] = (uint32_t)(J.h_outs[i] >> 32); }
  return rc;
}

// FqExpStark: chains on host threads (512 Montgomery products per instance), rows and the u16 range check on the device.
static int fq_trace_explicit(sbn_prover* P, const uint32_t* ios, size_t K, uint64_t* pi_out) {
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
  J.mark("chains");
  hipLaunchKernelGGL(tg::fq_row_kernel, blocks(n, 128), dim3(128), 0, st, d_ios, ca, cb, n, P->d_trace, d_err);
  J.mark("row_witness");
  if (int rc = J.launch_u16_range_check(d_cnt, d_err)) return rc;
  int err = 0;
  HIPC(hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
  if (int rc = J.end()) return rc;
  // public inputs: x, offset, exp_val, output = b at the last row, as u32 limbs (fq/exp.rs:98-108)
  return J.finish(err, pi_out, [&](size_t k, u64* p) {
    for (size_t i = 0; i < IOW; i++) p[i] = ios[IOW * k + i];
    const u64* out = P->h_chain + cw + (k * 257 + 256) * 4;  // B[256]
    for (int i = 0; i < 8; i++) p[24 + i] = (out[i >> 1] >> (32 * (i & 1))) & 0xffffffffULL;
  });
}

// ---- the entry points: argument checks of their own, the gate, then the explicit-list fallback or the source's driver -------------
// every entry point starts here, before any check: a refused call must not leave the previous trace provable
static int unload(sbn_prover* P) {
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  P->loaded = false;
  P->fixed_match = false;
  return 0;
}
static bool is_fq12(int kind) { return kind == SBN_AIR_FQ12_EXP || kind == SBN_AIR_FQ12_EXP_U64; }
// what every entry point asks of the prover.  *device_chains: the table's chains run on the device (G1 / G2 under chain_mode 1 and
// 2, Fq12 / Fq12U64 unless SBN_FQ12_HOST_CHAIN), so a derived list is derived there; elsewhere (host-pool curve chains,
// FqExpStark) the chains are host work anyway and so is the list
static int trace_gate(sbn_prover* P, size_t num_io, bool* device_chains) {
  const int kind = P->air.kind;
  if (!is_exp_air(kind)) return fail(SBN_ERR_UNSUPPORTED, "device witness generation covers the Exp tables (use sbn_generate_trace_g1_op + sbn_prover_load_trace)");
  if (num_io != P->air.num_io) return fail(SBN_ERR_BAD_ARG, "prover was created for %u instances, got %zu", P->air.num_io, num_io);
  if (P->n != exp_rows_per_instance(kind) * num_io) return fail(SBN_ERR_BAD_ARG, "degree_bits does not match the rows per instance");
  if (!is_fq12(kind) && !u16_device_witness_covers(P->n)) return fail(SBN_ERR_UNSUPPORTED, "device witness generation of the u16-range-check tables %s", U16_DEVICE_WITNESS_ROWS);
  *device_chains = kind != SBN_AIR_FQ_EXP && (is_fq12(kind) ? !P->set.fq12_host_chain : P->chain_mode != 0);
  return 0;
}
// the fallback: `derive(ios)` writes the explicit list on the host and the explicit call takes it
template <typename Derive>
static int trace_from_host_list(sbn_prover* P, size_t num_io, uint64_t* pi_out, uint32_t* ios_out, Derive derive) {
  std::vector<uint32_t> ios(exp_io_words(P->air.kind) * num_io);
  if (int rc = derive(ios.data())) return rc;
  const int rc = sbn_prover_generate_trace(P, ios.data(), num_io, pi_out);
  if (rc == SBN_OK && ios_out) memcpy(ios_out, ios.data(), ios.size() * sizeof(uint32_t));
  return rc;
}

// ---- the derived columns of a row-major load (trace_load.hip; include/sbn.h sbn_prover_load_trace_rows, main-row mode) --------------
// The main columns [0, num_main) are resident; everything behind them is a function of those and of the shape, written by the
// kernels the generators above end with.  The same gate as trace_gate (u16_device_witness_covers, host_common.hpp): the u16 tables
// from 2^16 rows up, the Fq12 kinds at any height.
int derived_columns_covered(const AirShape& as, size_t n) {
  if (!is_exp_air(as.kind)) return fail(SBN_ERR_UNSUPPORTED, "main-row mode covers the five Exp tables (hand in whole rows)");
  if (!is_fq12(as.kind) && !u16_device_witness_covers(n))
    return fail(SBN_ERR_UNSUPPORTED, "main-row mode of the u16-range-check tables %s on the device (use sbn_trace_from_rows_host + sbn_prover_load_trace)", U16_DEVICE_WITNESS_ROWS);
  return 0;
}
int launch_derived_columns(sbn_prover* P) {
  if (int rc = derived_columns_covered(P->air, P->n)) return rc;
  if (P->n != exp_rows_per_instance(P->air.kind) * P->air.num_io) return fail(SBN_ERR_BAD_ARG, "degree_bits does not match the rows per instance");
  HIPC(hipSetDevice(P->device));
  TraceJob J(P, P->air.num_io, 0);
  u64* inv = J.take(J.n);
  int* d_err = (int*)J.take(1);
  unsigned int* d_cnt = J.sh.split_rc ? nullptr : J.take_histograms();   // carved exactly as the generators of the u16 tables do
  if (int rc = J.fits()) return rc;
  if (!J.sh.split_rc) if (int rc = range_check_setup(P->device)) return rc;
  HIPC(hipEventRecord(P->abs_ev[0], J.st));
  HIPC(hipMemsetAsync(d_err, 0, sizeof(int), J.st));
  J.mark(nullptr);
  J.launch_shape_columns(inv, exp_table_max(J.sh));
  J.mark("pulses");
  if (J.sh.split_rc) {
    hipLaunchKernelGGL(tg::split_range_check_kernel, dim3((unsigned)J.sh.num_rc), dim3(256), 0, J.st, P->d_trace, J.n, J.sh.rc_start, J.sh.start_lookups, d_err);
    J.mark("range_check");
    HIPC(hipGetLastError());
  } else if (int rc = J.launch_u16_range_check(d_cnt, d_err)) return rc;
  int err = 0;
  HIPC(hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, J.st));
  if (int rc = J.end()) return rc;
  if (err & tg::TG_ERR_RANGE) return fail(SBN_ERR_WITNESS, "range-checked column holds a value >= 2^16");
  P->fixed_match = P->fixed_f1 > P->fixed_f0;   // by construction, as TraceJob::finish: those very kernels wrote the columns
  P->loaded = true;
  return SBN_OK;
}

extern "C" int sbn_prover_generate_trace(sbn_prover* P, const uint32_t* ios, size_t num_io, uint64_t* pi_out) {
  if (int rc = unload(P)) return rc;
  if (!ios) return fail(SBN_ERR_BAD_ARG, "null argument");
  bool device_chains;
  if (int rc = trace_gate(P, num_io, &device_chains)) return rc;
  const int kind = P->air.kind;
  if (is_fq12(kind)) return fq12_trace_explicit(P, ios, num_io, pi_out);
  if (kind == SBN_AIR_FQ_EXP) return fq_trace_explicit(P, ios, num_io, pi_out);
  return kind == SBN_AIR_G1_EXP ? curve_trace_explicit<1>(P, ios, num_io, pi_out) : curve_trace_explicit<2>(P, ios, num_io, pi_out);
}

// sbn_prover_generate_trace on the list sbn_chain_instances derives from (terms, start)
extern "C" int sbn_prover_generate_trace_chained(sbn_prover* P, const uint32_t* terms, size_t num_io, const uint32_t* start, uint64_t* pi_out, uint32_t* ios_out) {
  if (int rc = unload(P)) return rc;
  if (!terms || !start) return fail(SBN_ERR_BAD_ARG, "null argument");
  bool device_chains;
  if (int rc = trace_gate(P, num_io, &device_chains)) return rc;
  const int kind = P->air.kind;
  if (!device_chains) return trace_from_host_list(P, num_io, pi_out, ios_out, [&](uint32_t* ios) { return chain_instances_host(kind, terms, num_io, start, ios, nullptr); });
  const ChainedIn ch{terms, start, ios_out};
  if (is_fq12(kind)) return fq12_trace_chained(P, ch, num_io, pi_out);
  return kind == SBN_AIR_G1_EXP ? curve_trace_chained<1>(P, ch, num_io, pi_out) : curve_trace_chained<2>(P, ch, num_io, pi_out);
}

// sbn_prover_generate_trace on the list sbn_scalar_mul_instances derives from (points, scalars, offset), one unit
extern "C" int sbn_prover_generate_trace_scalar_muls(sbn_prover* P, const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t num_io,
                                                     const uint32_t* offset, uint64_t* pi_out, uint32_t* products_out, uint8_t* infinity_out, uint32_t* ios_out) {
  if (int rc = unload(P)) return rc;
  const int kind = P->air.kind;
  if (kind != SBN_AIR_G1_EXP && kind != SBN_AIR_G2_EXP) return fail(SBN_ERR_UNSUPPORTED, "scalar multiplications cover the curve tables G1_EXP and G2_EXP");
  if (!points || !scalars || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument or no instance");
  if (scalar_count != 1 && scalar_count != num_io) return fail(SBN_ERR_BAD_ARG, "scalar_count must be 1 (one shared scalar) or count = %zu, got %zu", num_io, scalar_count);
  bool device_chains;
  if (int rc = trace_gate(P, num_io, &device_chains)) return rc;
  const int E = kind == SBN_AIR_G1_EXP ? 1 : 2;
  if (!offset) offset = curve_generator_words(E);
  if (!device_chains)
    return trace_from_host_list(P, num_io, pi_out, ios_out, [&](uint32_t* ios) {
      return sbn_scalar_mul_instances(kind, points, scalars, scalar_count, num_io, num_io, offset, ios, products_out, infinity_out);
    });
  const ScalarMulIn sm{points, scalars, scalar_count, offset, products_out, infinity_out, ios_out};
  return E == 1 ? curve_trace_scalar_muls<1>(P, sm, num_io, pi_out) : curve_trace_scalar_muls<2>(P, sm, num_io, pi_out);
}

// sbn_prover_generate_trace on the one-unit list sbn_msm_batch_instances derives from (terms, lengths, starts)
extern "C" int sbn_prover_generate_trace_msm_batch(sbn_prover* P, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts,
                                                   size_t start_count, uint64_t* pi_out, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out,
                                                   uint32_t* ios_out) {
  if (int rc = unload(P)) return rc;
  const int kind = P->air.kind;
  const size_t num_io = P->air.num_io;
  size_t M = 0;
  if (int rc = msm_batch_check_args(kind, terms, lengths, segments, &starts, &start_count, num_io, sums_out, infinity_out, &M)) return rc;
  if (M > num_io) return fail(SBN_ERR_BAD_ARG, "%zu segments of %zu instances do not fit one unit of %zu instances", segments, M, num_io);
  bool device_chains;
  if (int rc = trace_gate(P, num_io, &device_chains)) return rc;
  if (!device_chains)
    return trace_from_host_list(P, num_io, pi_out, ios_out, [&](uint32_t* ios) {
      return msm_batch_derive(kind, terms, lengths, segments, starts, start_count, M, num_io, ios, finals_out, sums_out, infinity_out);
    });
  const BatchIn mb{terms, lengths, segments, starts, start_count, M, finals_out, sums_out, infinity_out, ios_out};
  if (is_fq12(kind)) return fq12_trace_segmented(P, mb, num_io, pi_out);
  return kind == SBN_AIR_G1_EXP ? curve_trace_segmented<1>(P, mb, num_io, pi_out) : curve_trace_segmented<2>(P, mb, num_io, pi_out);
}

// sbn_prover_generate_trace on the one-unit list sbn_msm_batch_instances_complete derives from (terms, term_infinity, lengths).  Where
// the chains run on the device the segmented driver above derives the list there, every segment from candidate 0 first, in rounds
// until no segment reports a bad event.  Placement 0 and a list that exhausts the candidates derive on the host pool.
extern "C" int sbn_prover_generate_trace_msm_batch_complete(sbn_prover* P, const uint32_t* terms, const uint8_t* term_infinity, const uint64_t* lengths,
                                                            size_t segments, uint64_t* pi_out, uint32_t* terms_out, uint32_t* starts_out, uint8_t* choice_out,
                                                            uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out, uint32_t* ios_out) {
  if (int rc = unload(P)) return rc;
  const int kind = P->air.kind;
  const size_t num_io = P->air.num_io;
  size_t M = 0;
  if (int rc = msm_batch_complete_args(kind, terms, lengths, segments, num_io, &M)) return rc;
  if (M > num_io) return fail(SBN_ERR_BAD_ARG, "%zu segments of %zu instances do not fit one unit of %zu instances", segments, M, num_io);
  bool device_chains;
  if (int rc = trace_gate(P, num_io, &device_chains)) return rc;
  const size_t W = pi_layout(kind).xw, T = pi_layout(kind).T();
  std::vector<uint32_t> own_terms, own_starts;
  std::vector<uint8_t> own_choice;
  if (!terms_out) { own_terms.resize(T * M); terms_out = own_terms.data(); }
  if (!starts_out) { own_starts.resize(W * segments); starts_out = own_starts.data(); }
  if (!choice_out) { own_choice.resize(segments); choice_out = own_choice.data(); }
  if (int rc = msm_batch_effective_terms(kind, terms, term_infinity, lengths, segments, M, terms_out)) return rc;
  if (!device_chains)
    return trace_from_host_list(P, num_io, pi_out, ios_out, [&](uint32_t* ios) {
      return msm_batch_complete_choose(kind, terms_out, lengths, segments, M, num_io, ios, starts_out, choice_out, finals_out, sums_out, infinity_out);
    });
  const int E = kind == SBN_AIR_G1_EXP ? 1 : 2;
  for (size_t s = 0; s < segments; s++) memcpy(starts_out + W * s, curve_start_candidate_words(E, 0), W * sizeof(uint32_t));
  memset(choice_out, 0, segments);
  BatchIn mb{terms_out, lengths, segments, starts_out, segments, M, finals_out, sums_out, infinity_out, ios_out};
  mb.choice = choice_out; mb.starts_out = starts_out;
  return E == 1 ? curve_trace_segmented<1>(P, mb, num_io, pi_out) : curve_trace_segmented<2>(P, mb, num_io, pi_out);
}

// sbn_prover_generate_trace on the one-unit list sbn_power_instances derives from (bases, exps, depth)
extern "C" int sbn_prover_generate_trace_powers(sbn_prover* P, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count, size_t depth,
                                                uint64_t* pi_out, uint32_t* powers_out, uint32_t* ios_out) {
  if (int rc = unload(P)) return rc;
  const int kind = P->air.kind;
  if (!pi_layout(kind).field()) return fail(SBN_ERR_UNSUPPORTED, "field powers cover the field tables FQ_EXP, FQ12_EXP and FQ12_EXP_U64");
  if (!bases || !exps || count == 0 || depth == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no tower or depth = 0");
  if (exp_count != 1 && exp_count != count) return fail(SBN_ERR_BAD_ARG, "exp_count must be 1 (one shared exponent) or count = %zu, got %zu", count, exp_count);
  const size_t num_io = P->air.num_io;
  if (count > num_io || depth > num_io / count) return fail(SBN_ERR_BAD_ARG, "%zu towers of depth %zu do not fit one unit of %zu instances", count, depth, num_io);
  bool device_chains;
  if (int rc = trace_gate(P, num_io, &device_chains)) return rc;
  if (!device_chains)
    return trace_from_host_list(P, num_io, pi_out, ios_out, [&](uint32_t* ios) { return sbn_power_instances(kind, bases, exps, exp_count, count, depth, num_io, ios, powers_out); });
  const PowerIn pw{bases, exps, exp_count, count, depth, powers_out, ios_out};
  return fq12_trace_towers(P, pw, num_io, pi_out);
}

// sbn_prover_generate_trace on the one-unit list sbn_program_instances derives from (nodes, values, exps); maps (optional, [count]):
// the list of sbn_program_m_instances
static int generate_trace_program(sbn_prover* P, const sbn_program_node* nodes, const uint32_t* maps, size_t count, const uint32_t* values, size_t n_values,
                                  const uint32_t* exps, size_t n_exps, uint64_t* pi_out, uint32_t* outs_out, uint32_t* ios_out) {
  if (int rc = unload(P)) return rc;
  const int kind = P->air.kind;
  if (!pi_layout(kind).field()) return fail(SBN_ERR_UNSUPPORTED, "field programs cover the field tables FQ_EXP, FQ12_EXP and FQ12_EXP_U64");
  if (!nodes || !values || !exps || count == 0) return fail(SBN_ERR_BAD_ARG, "null argument or no node");
  const size_t num_io = P->air.num_io;
  if (count > num_io) return fail(SBN_ERR_BAD_ARG, "a program of %zu nodes does not fit one unit of %zu instances", count, num_io);
  bool device_chains;
  if (int rc = trace_gate(P, num_io, &device_chains)) return rc;
  if (!device_chains)
    return trace_from_host_list(P, num_io, pi_out, ios_out, [&](uint32_t* ios) { return program_instances(kind, nodes, maps, count, values, n_values, exps, n_exps, num_io, ios, outs_out); });
  ProgramPlan plan;
  if (int rc = program_plan(kind, nodes, count, values, n_values, exps, n_exps, num_io, plan, maps)) return rc;
  const ProgramIn pr{nodes, maps, count, values, exps, outs_out, ios_out};
  return fq12_trace_program(P, pr, plan, num_io, pi_out);
}
extern "C" int sbn_prover_generate_trace_program(sbn_prover* P, const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values,
                                                 const uint32_t* exps, size_t n_exps, uint64_t* pi_out, uint32_t* outs_out, uint32_t* ios_out) {
  return generate_trace_program(P, nodes, nullptr, count, values, n_values, exps, n_exps, pi_out, outs_out, ios_out);
}
// (a table that does not fit the unit is refused before a node is read, so only one that fits is split)
extern "C" int sbn_prover_generate_trace_program_m(sbn_prover* P, const sbn_program_node_m* nodes, size_t count, const uint32_t* values, size_t n_values,
                                                   const uint32_t* exps, size_t n_exps, uint64_t* pi_out, uint32_t* outs_out, uint32_t* ios_out) {
  std::vector<sbn_program_node> plain; std::vector<uint32_t> maps;
  if (P && nodes && count && count <= P->air.num_io) curve_host::split_nodes(nodes, count, plain, maps);
  return generate_trace_program(P, plain.empty() ? (const sbn_program_node*)nodes : plain.data(), maps.data(), count, values, n_values, exps, n_exps, pi_out, outs_out, ios_out);
}

// sbn_prover_generate_trace on the one-unit list sbn_curve_program_instances derives from (nodes, points, exps).  Where the chains
// run on the device the links are resolved there from candidate 0; a bad event there, like placement 0, derives on the host pool,
// which walks the candidates and words the refusal of a program that exhausts them.
extern "C" int sbn_prover_generate_trace_curve_program(sbn_prover* P, const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points,
                                                       const uint32_t* exps, size_t n_exps, uint64_t* pi_out, uint32_t* outs_out, uint32_t* values_out,
                                                       uint8_t* infinity_out, uint8_t* choice_out, uint32_t* ios_out) {
  if (int rc = unload(P)) return rc;
  const int kind = P->air.kind;
  if (kind != SBN_AIR_G1_EXP && kind != SBN_AIR_G2_EXP) return fail(SBN_ERR_UNSUPPORTED, "curve programs cover the curve tables G1_EXP and G2_EXP");
  if (!nodes || !points || !exps || count == 0) return fail(SBN_ERR_BAD_ARG, "null argument or no node");
  const size_t num_io = P->air.num_io;
  if (count > num_io) return fail(SBN_ERR_BAD_ARG, "a program of %zu nodes does not fit one unit of %zu instances", count, num_io);
  bool device_chains;
  if (int rc = trace_gate(P, num_io, &device_chains)) return rc;
  const auto on_host = [&] {
    return trace_from_host_list(P, num_io, pi_out, ios_out, [&](uint32_t* ios) {
      return sbn_curve_program_instances(kind, nodes, count, points, n_points, exps, n_exps, num_io, ios, outs_out, values_out, infinity_out, choice_out);
    });
  };
  if (!device_chains) return on_host();
  ProgramPlan plan;
  if (int rc = curve_program_plan(kind, nodes, count, points, n_points, exps, n_exps, num_io, plan)) return rc;
  const CurveProgramIn pr{nodes, count, points, exps, outs_out, values_out, infinity_out, ios_out};
  bool fallback = false;
  const int rc = kind == SBN_AIR_G1_EXP ? curve_trace_program<1>(P, pr, plan, num_io, pi_out, &fallback) : curve_trace_program<2>(P, pr, plan, num_io, pi_out, &fallback);
  if (rc != SBN_OK) return rc;
  if (fallback) return on_host();
  if (choice_out) *choice_out = 0;
  return SBN_OK;
}

extern "C" int sbn_bn254_fq_batch(int op,const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, int on_device) {
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
