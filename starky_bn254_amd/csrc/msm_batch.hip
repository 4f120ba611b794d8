// Batches of short MSMs (include/sbn.h, "Batches of short MSMs"): SEGMENTED chained lists packed into shared units.  The
// reference's g1_exp_circuit (src/curves/g1/circuit.rs:262-304) takes any list of inputs and the caller wires the offsets: some
// inputs continue a chain, others start a new one -- one public-key aggregation per signature, one product of a few x_k^e_k per
// pairing check.  sbn_msm_instances is one segment, sbn_scalar_mul_instances is segments of length 1 with a shared start; here
//  * sbn_msm_batch_instances derives the whole explicit list on the host pool by the scheme of chain_instances.hip: the terms
//    e_k x_k (x_k^e_k) in parallel, one pass of complete additions (products) per segment from the segment's own start, ONE
//    inversion for the affine form of every offset, final and sum, then the table's own walk of the explicit list;
//  * sbn_msm_batch_check is what the `connect` calls of a circuit are: it reads the public inputs of the unit proofs and checks that
//    every head starts from its start, that every other offset is the output before it, and that the pads repeat the last instance.
//    It verifies no proof.
// Host code only: no kernel is launched from this unit (tracegen_device.hip holds the device form of the derivation).
#include "curve_host.hpp"
#include <cstring>

using namespace sbn;

namespace {
using namespace bnw;
using namespace sbn::curve_host;

// word counts of a table: x / offset value (xw), exponent (ew), in `terms`, `starts` and `ios`; N = Fq components of a value
struct Tab {
  int E;          // 1 / 2 on the curves, 0 in the fields
  size_t xw, ew;
  size_t T() const { return xw + ew; }
  size_t IOW() const { return 2 * xw + ew; }
  int values() const { return (int)(xw / 8); }
};
bool table_of(int kind, Tab& t) {
  switch (kind) {
    case SBN_AIR_G1_EXP: t = {1, 16, 8}; return true;
    case SBN_AIR_G2_EXP: t = {2, 32, 8}; return true;
    case SBN_AIR_FQ_EXP: t = {0, 8, 8}; return true;
    case SBN_AIR_FQ12_EXP: t = {0, 96, 8}; return true;
    case SBN_AIR_FQ12_EXP_U64: t = {0, 96, 2}; return true;
    default: return false;
  }
}
const uint32_t FIELD_ONE[96] = {1};

// head[s] = the global index of the first instance of segment s (head[segments] = M); seg[g] = the segment of instance g
struct Layout {
  std::vector<size_t> head;
  std::vector<uint32_t> seg;
  Layout(const uint64_t* lengths, size_t segments, size_t M) : head(segments + 1), seg(M) {
    size_t at = 0;
    for (size_t s = 0; s < segments; s++) { head[s] = at; for (size_t j = 0; j < lengths[s]; j++) seg[at + j] = (uint32_t)s; at += (size_t)lengths[s]; }
    head[segments] = at;
  }
};

// the smallest index in [0, K) for which bad(k) holds, on the host pool; K when there is none
template <typename F> size_t first_bad(size_t K, F bad) {
  std::atomic<size_t> at(K);
  host_parallel_for(K, [&](size_t k) {
    if (k > at.load() || !bad(k)) return;
    size_t cur = at.load(); while (k < cur && !at.compare_exchange_weak(cur, k)) {}
  });
  return at.load();
}

// ---- the refusals of the inputs, in the header's order: >= p, off the curve, a non-canonical u64 exponent --------------------------
template <int E> int check_curve_inputs(const uint32_t* terms, size_t M, const Layout& L, const uint32_t* starts, size_t start_count) {
  const size_t T = 16 * E + 8;
  for (size_t s = 0; s < start_count; s++)
    if (!below_p(starts + 16 * E * s, 2 * E)) return fail(SBN_ERR_BAD_ARG, "coordinate >= p (start %zu)", s);
  for (size_t g = 0; g < M; g++)
    if (!below_p(terms + T * g, 2 * E)) return fail(SBN_ERR_BAD_ARG, "coordinate >= p (instance %zu, segment %u)", g, L.seg[g]);
  const Co<E> b = curve_b<E>();
  for (size_t s = 0; s < start_count; s++) {
    const Jac<E> p = ld_point<E>(starts + 16 * E * s);
    if (!on_curve<E>(p.X, p.Y, b)) return fail(SBN_ERR_BAD_ARG, "start %zu is not a point of the curve", s);
  }
  const size_t bad = first_bad(M, [&](size_t g) { const Jac<E> p = ld_point<E>(terms + T * g); return !on_curve<E>(p.X, p.Y, b); });
  if (bad < M) return fail(SBN_ERR_BAD_ARG, "x of instance %zu (segment %u) is not a point of the curve", bad, L.seg[bad]);
  return SBN_OK;
}
int check_field_inputs(const Tab& t, const uint32_t* terms, size_t M, const Layout& L, const uint32_t* starts, size_t start_count) {
  const char* what = t.xw == 8 ? "value" : "coefficient";
  for (size_t s = 0; s < start_count; s++)
    if (!below_p(starts + t.xw * s, t.values())) return fail(SBN_ERR_BAD_ARG, "%s >= p (start %zu)", what, s);
  for (size_t g = 0; g < M; g++)
    if (!below_p(terms + t.T() * g, t.values())) return fail(SBN_ERR_BAD_ARG, "%s >= p (instance %zu, segment %u)", what, g, L.seg[g]);
  if (t.ew == 2)
    for (size_t g = 0; g < M; g++)
      if (((u64)terms[t.T() * g + 96] | ((u64)terms[t.T() * g + 97] << 32)) >= GLP)
        return fail(SBN_ERR_NON_CANONICAL, "exponent of instance %zu (segment %u) is not a canonical field element", g, L.seg[g]);
  return SBN_OK;
}

// rows [M, total) <- row M - 1: the reference's resize rule (src/curves/g1/circuit.rs:273-277)
void pad_rows(uint32_t* ios, size_t IOW, size_t M, size_t total) {
  for (size_t g = M; g < total; g++) memcpy(ios + IOW * g, ios + IOW * (M - 1), IOW * sizeof(uint32_t));
}

// ---- the curve tables ------------------------------------------------------------------------------------------------------------
template <int E>
int derive_curve(const uint32_t* terms, size_t M, const Layout& L, size_t segments, const uint32_t* starts, size_t start_count, size_t total,
                 uint32_t* ios, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out) {
  const size_t T = 16 * E + 8, IOW = 32 * E + 8, W = 16 * E;
  if (int rc = check_curve_inputs<E>(terms, M, L, starts, start_count)) return rc;
  std::vector<Jac<E>> term(M);
  host_parallel_for(M, [&](size_t g) { term[g] = scalar_mul_jac<E>(ld_point<E>(terms + T * g), terms + T * g + W); });
  // pts: the M offsets, then the finals, then the sums final + (-start) of every segment
  std::vector<Jac<E>> pts(M + 2 * segments);
  host_parallel_for(segments, [&](size_t s) {
    const Jac<E> st = ld_point<E>(starts + (start_count == 1 ? 0 : W * s));
    Jac<E> acc = st;
    for (size_t g = L.head[s]; g < L.head[s + 1]; g++) { pts[g] = acc; acc = jac_add_complete<E>(acc, term[g]); }
    pts[M + s] = acc;
    pts[M + segments + s] = jac_add_complete<E>(acc, neg_point<E>(st));
  });
  for (size_t g = 0; g < M; g++) {   // in instance order: the table cannot hold the point at infinity
    const size_t s = L.seg[g];
    if (czero<E>(pts[g].Z)) return fail(SBN_ERR_WITNESS, "the offset of instance %zu (segment %zu) is the point at infinity", g, s);
    if (g + 1 == L.head[s + 1] && czero<E>(pts[M + s].Z)) return fail(SBN_ERR_WITNESS, "the output of instance %zu (segment %zu) is the point at infinity", g, s);
  }
  std::vector<uint32_t> aff(W * pts.size());
  std::vector<uint8_t> inf(pts.size());
  affine_or_infinity<E>(pts, aff.data(), inf.data());   // one inversion for every Z
  for (size_t g = 0; g < M; g++) {
    uint32_t* io = ios + IOW * g;
    memcpy(io, terms + T * g, W * sizeof(uint32_t));
    memcpy(io + W, aff.data() + W * g, W * sizeof(uint32_t));
    memcpy(io + 2 * W, terms + T * g + W, 8 * sizeof(uint32_t));
  }
  pad_rows(ios, IOW, M, total);
  if (finals_out) memcpy(finals_out, aff.data() + W * M, W * segments * sizeof(uint32_t));
  if (sums_out) memcpy(sums_out, aff.data() + W * (M + segments), W * segments * sizeof(uint32_t));
  if (infinity_out) memcpy(infinity_out, inf.data() + M + segments, segments);
  // the table's own walk of the real instances (g1/exp.rs:165-230), 512 at a time to bound the chain storage; the first instance it
  // cannot walk is named through the one-instance form of the same walk
  const size_t CH = 512;
  std::vector<u64> chains(2 * 257 * 12 * E * (M < CH ? M : CH));
  for (size_t at = 0; at < M; at += CH) {
    const size_t k = M - at < CH ? M - at : CH, cw = 257 * 12 * E * k;
    if (!tracegen_host_chains(E, ios + IOW * at, k, chains.data(), chains.data() + cw)) continue;
    const size_t bad = first_bad(k, [&](size_t i) {
      std::vector<u64> ja(257 * 12 * E), jb(257 * 12 * E);
      return exp_chains<E>(ios + IOW * (at + i), 0, ja.data(), jb.data()) != 0;
    });
    if (bad == k) return fail(SBN_ERR_WITNESS, "degenerate affine operation (x1 == x2 or y == 0)");
    return fail(SBN_ERR_WITNESS, "instance %zu (segment %u): degenerate affine operation in the table's walk (B[t] = +-2^t x at a set bit): pick another start",
                at + bad, L.seg[at + bad]);
  }
  return SBN_OK;
}

// ---- the field tables: N = 1 (FQ_EXP) or 12 (the flat basis of the Fq12 tables) ------------------------------------------------------
template <int N> void fmul(const Fq* a, const Fq* b, Fq* out) {
  if (N == 1) { out[0] = mmul(a[0], b[0]); return; }
  Fq prod[12]; fq12_mul_m(a, b, prod); memcpy(out, prod, N * sizeof(Fq));
}
template <int N>
int derive_field(const Tab& t, const uint32_t* terms, size_t M, const Layout& L, size_t segments, const uint32_t* starts, size_t start_count, size_t total,
                 uint32_t* ios, uint32_t* finals_out) {
  const size_t W = 8 * N, T = t.T(), IOW = t.IOW();
  if (int rc = check_field_inputs(t, terms, M, L, starts, start_count)) return rc;
  std::vector<Fq> term((size_t)N * M);
  host_parallel_for(M, [&](size_t g) {   // x^e by the table's square-and-multiply, least significant bit first
    Fq a[N], b[N];
    for (int c = 0; c < N; c++) { u64 t4[4]; ld_u32(terms + T * g + 8 * c, t4); a[c] = to_m(t4); b[c] = Fq{{0, 0, 0, 0}}; }
    b[0] = fq_one();
    const uint32_t* e = terms + T * g + W;
    for (int i = 0; i < (int)(32 * t.ew); i++) { if ((e[i >> 5] >> (i & 31)) & 1) fmul<N>(a, b, b); fmul<N>(a, a, a); }
    memcpy(&term[(size_t)N * g], b, sizeof b);
  });
  host_parallel_for(segments, [&](size_t s) {
    Fq off[N];
    for (int c = 0; c < N; c++) { u64 t4[4]; ld_u32(starts + (start_count == 1 ? 0 : W * s) + 8 * c, t4); off[c] = to_m(t4); }
    for (size_t g = L.head[s]; g < L.head[s + 1]; g++) {
      uint32_t* io = ios + IOW * g;
      memcpy(io, terms + T * g, W * sizeof(uint32_t));
      for (int c = 0; c < N; c++) st_u32(off[c], io + W + 8 * c);
      memcpy(io + 2 * W, terms + T * g + W, t.ew * sizeof(uint32_t));
      fmul<N>(off, &term[(size_t)N * g], off);
    }
    if (finals_out) for (int c = 0; c < N; c++) st_u32(off[c], finals_out + W * s + 8 * c);
  });
  pad_rows(ios, IOW, M, total);
  return SBN_OK;
}

// ---- sbn_msm_batch_check: the public inputs of one instance are x[W] offset[W] exp[EW] output[W] (g1_exp_io_to_columns,
// src/curves/g1/exp.rs:124-135, and its twins): u32 limbs on the curves and in Fq, 16-bit limbs in Fq12 -----------------------------
// (PiLayout: host_common.hpp)
bool same(const uint64_t* a, const uint64_t* b, size_t n) { return memcmp(a, b, n * sizeof(uint64_t)) == 0; }

template <int E>
int check_curve_outputs(const std::vector<uint32_t>& outs, size_t M, const Layout& L, size_t segments, const uint32_t* starts, size_t start_count,
                        uint32_t* sums_out, uint8_t* infinity_out) {
  const size_t W = 16 * E;
  const Co<E> b = curve_b<E>();
  for (size_t g = 0; g < M; g++) {
    const uint32_t* o = outs.data() + W * g;
    if (!below_p(o, 2 * E)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %u): output has a coordinate >= p", g, L.seg[g]);
    const Jac<E> q = ld_point<E>(o);
    if (!on_curve<E>(q.X, q.Y, b)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %u): output is not a point of the curve", g, L.seg[g]);
  }
  if (!sums_out && !infinity_out) return SBN_OK;
  std::vector<Jac<E>> sum(segments);
  for (size_t s = 0; s < segments; s++)
    sum[s] = jac_add_complete<E>(ld_point<E>(outs.data() + W * (L.head[s + 1] - 1)), neg_point<E>(ld_point<E>(starts + (start_count == 1 ? 0 : W * s))));
  affine_or_infinity<E>(sum, sums_out, infinity_out);
  return SBN_OK;
}
}  // namespace

namespace sbn {
int msm_batch_check_args(int kind, const void* terms, const uint64_t* lengths, size_t segments, const uint32_t** starts, size_t* start_count, size_t num_io,
                         const void* sums_out, const void* infinity_out, size_t* M_out) {
  Tab t;
  if (!table_of(kind, t)) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not an Exp table: segmented lists cover the five Exp tables", kind);
  if (!terms || !lengths) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (segments == 0) return fail(SBN_ERR_BAD_ARG, "no segment");
  size_t M = 0;
  for (size_t s = 0; s < segments; s++) {
    if (lengths[s] == 0) return fail(SBN_ERR_BAD_ARG, "segment %zu has length 0 (it would start at instance %zu): every segment holds at least one instance", s, M);
    if (lengths[s] > (uint64_t)((size_t)-1 / 512 - M)) return fail(SBN_ERR_BAD_ARG, "the lengths do not fit (segment %zu)", s);
    M += (size_t)lengths[s];
  }
  *M_out = M;   // (known from here on, also when a later refusal returns)
  if (!*starts) { *starts = t.E ? curve_generator_words(t.E) : FIELD_ONE; *start_count = 1; }   // the generator / one, shared
  if (*start_count != 1 && *start_count != segments)
    return fail(SBN_ERR_BAD_ARG, "start_count must be 1 (one shared start) or segments = %zu, got %zu", segments, *start_count);
  if (num_io == 0) return fail(SBN_ERR_BAD_ARG, "num_io = 0");
  if (!t.E && (sums_out || infinity_out)) return fail(SBN_ERR_BAD_ARG, "sums_out / infinity_out are outputs of the curve tables (with the default start a field final is the product)");
  return SBN_OK;
}

int msm_batch_check_inputs(int kind, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts, size_t start_count, size_t M) {
  Tab t;
  if (!table_of(kind, t)) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not an Exp table", kind);
  const Layout L(lengths, segments, M);
  if (t.E == 1) return check_curve_inputs<1>(terms, M, L, starts, start_count);
  if (t.E == 2) return check_curve_inputs<2>(terms, M, L, starts, start_count);
  return check_field_inputs(t, terms, M, L, starts, start_count);
}

int msm_batch_derive(int kind, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts, size_t start_count, size_t M,
                     size_t total, uint32_t* ios, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out) {
  Tab t;
  if (!table_of(kind, t)) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not an Exp table", kind);
  const Layout L(lengths, segments, M);
  if (t.E == 1) return derive_curve<1>(terms, M, L, segments, starts, start_count, total, ios, finals_out, sums_out, infinity_out);
  if (t.E == 2) return derive_curve<2>(terms, M, L, segments, starts, start_count, total, ios, finals_out, sums_out, infinity_out);
  if (t.xw == 8) return derive_field<1>(t, terms, M, L, segments, starts, start_count, total, ios, finals_out);
  return derive_field<12>(t, terms, M, L, segments, starts, start_count, total, ios, finals_out);
}
}  // namespace sbn

extern "C" int sbn_msm_batch_instances(int32_t kind, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts, size_t start_count,
                                       size_t num_io, uint32_t* ios_out, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out) {
  size_t M = 0;
  if (int rc = msm_batch_check_args((int)kind, terms, lengths, segments, &starts, &start_count, num_io, sums_out, infinity_out, &M)) return rc;
  const size_t total = sbn_msm_num_units(M, num_io) * num_io;
  std::vector<uint32_t> own;
  uint32_t* ios = ios_out;
  if (!ios) { own.resize(exp_io_words((int)kind) * total); ios = own.data(); }
  return msm_batch_derive((int)kind, terms, lengths, segments, starts, start_count, M, total, ios, finals_out, sums_out, infinity_out);
}

extern "C" int sbn_msm_batch_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, const uint64_t* lengths, size_t segments,
                                   const uint32_t* terms /*optional*/, const uint32_t* starts, size_t start_count, uint32_t* finals_out, uint32_t* sums_out,
                                   uint8_t* infinity_out) {
  size_t M = 0;
  Tab t;
  if (!table_of((int)kind, t)) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not an Exp table: segmented lists cover the five Exp tables", (int)kind);
  if (!public_inputs) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (int rc = msm_batch_check_args((int)kind, public_inputs, lengths, segments, &starts, &start_count, num_io, sums_out, infinity_out, &M)) return rc;
  if (units != sbn_msm_num_units(M, num_io))
    return fail(SBN_ERR_VERIFY_FAILED, "%zu units given, %zu segments of %zu instances in tables of %zu have %zu units", units, segments, M, num_io, sbn_msm_num_units(M, num_io));
  for (size_t u = 0; u < units; u++) if (!public_inputs[u]) return fail(SBN_ERR_BAD_ARG, "null public inputs (unit %zu)", u);
  if (!below_p(starts, t.values() * (int)start_count)) return fail(SBN_ERR_BAD_ARG, "%s >= p (starts)", t.E ? "coordinate" : "coefficient");
  const Layout L(lengths, segments, M);
  const PiLayout P = pi_layout((int)kind);
  const size_t per = P.per(), oX = 0, oOff = P.W, oExp = 2 * P.W, oOut = 2 * P.W + P.EW;
  auto inst = [&](size_t g) { return public_inputs[g / num_io] + per * (g % num_io); };
  const uint64_t lim = P.limb16 ? 0xffffULL : 0xffffffffULL;
  const uint64_t* last = inst(M - 1);
  std::vector<uint64_t> want(P.W);
  std::vector<uint32_t> outs(t.xw * M);
  for (size_t g = 0; g < units * num_io; g++) {
    const uint64_t* p = inst(g);
    if (g >= M) {   // a pad instance is instance M - 1 again
      static const char* const field[4] = {"x", "offset", "exponent", "output"};
      const size_t at[4] = {oX, oOff, oExp, oOut}, len[4] = {P.W, P.W, P.EW, P.W};
      for (int f = 0; f < 4; f++)
        if (!same(p + at[f], last + at[f], len[f])) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (pad): %s differs from instance %zu", g, field[f], M - 1);
      continue;
    }
    const size_t s = L.seg[g];
    if (terms) {
      value_to_pi(P, terms + t.T() * g, want.data());
      if (!same(p + oX, want.data(), P.W)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %zu): x differs from the caller's term", g, s);
      const uint32_t* e = terms + t.T() * g + t.xw;
      uint64_t ep[8];
      exp_to_pi(P, e, ep);
      if (!same(p + oExp, ep, P.EW)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %zu): exponent differs from the caller's term", g, s);
    }
    if (g == L.head[s]) {
      value_to_pi(P, starts + (start_count == 1 ? 0 : t.xw * s), want.data());
      if (!same(p + oOff, want.data(), P.W)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %zu): offset differs from the start of the segment", g, s);
    } else if (!same(p + oOff, inst(g - 1) + oOut, P.W))
      return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %zu): offset differs from the output of instance %zu", g, s, g - 1);
    // a limb wider than its slot is no output of the table
    for (size_t i = 0; i < P.W; i++)
      if (p[oOut + i] > lim) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %zu): output limb %zu is out of range", g, s, i);
    uint32_t* o = outs.data() + t.xw * g;
    if (!P.limb16) for (size_t i = 0; i < t.xw; i++) o[i] = (uint32_t)p[oOut + i];
    else for (size_t i = 0; i < t.xw; i++) o[i] = (uint32_t)(p[oOut + 2 * i] | (p[oOut + 2 * i + 1] << 16));
  }
  if (t.E == 1) { if (int rc = check_curve_outputs<1>(outs, M, L, segments, starts, start_count, sums_out, infinity_out)) return rc; }
  else if (t.E == 2) { if (int rc = check_curve_outputs<2>(outs, M, L, segments, starts, start_count, sums_out, infinity_out)) return rc; }
  if (finals_out) for (size_t s = 0; s < segments; s++) memcpy(finals_out + t.xw * s, outs.data() + t.xw * (L.head[s + 1] - 1), t.xw * sizeof(uint32_t));
  return SBN_OK;
}
