// Batches of short MSMs (include/sbn.h, "Batches of short MSMs"): SEGMENTED chained lists packed into shared units.  The
// reference's g1_exp_circuit (src/curves/g1/circuit.rs:262-304) takes any list of inputs and the caller wires the offsets: some
// inputs continue a chain, others start a new one -- one public-key aggregation per signature, one product of a few x_k^e_k per
// pairing check.  sbn_chain_instances / sbn_msm_instances is one segment (and derived here: segmented_derive),
// sbn_scalar_mul_instances is segments of length 1 with a shared start; here
//  * sbn_msm_batch_instances derives the whole explicit list on the host pool: the terms e_k x_k (x_k^e_k) in parallel, one pass
//    of complete additions (products) per segment from the segment's own start, ONE inversion for the affine form of every
//    offset, final and sum, then the table's own walk of the explicit list.  On the curves the terms run in Jacobian coordinates
//    with the COMPLETE addition of bn254w.cuh (a term may be the identity, and the double-and-add inside a term meets equal
//    operands when e has a leading 1 only): a collision in this derivation says nothing about the table's own walk and is not
//    an error; only that walk, or an offset at infinity, refuses a list;
//  * sbn_msm_batch_check is what the `connect` calls of a circuit are: it reads the public inputs of the unit proofs and checks that
//    every head starts from its start, that every other offset is the output before it, and that the pads repeat the last instance.
//    It verifies no proof.
// Host code only: no kernel is launched from this unit (tracegen_device.hip holds the device form of the derivation).
#include "instance_lists.hpp"

using namespace sbn;

namespace {
using namespace bnw;
using namespace sbn::curve_host;

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

// ---- the refusals of the inputs, in the header's order: >= p, off the curve, a non-canonical u64 exponent --------------------------
template <int E> int check_curve_inputs(const PiLayout& t, const uint32_t* terms, size_t M, const Layout& L, const uint32_t* starts, size_t start_count) {
  const size_t T = t.T();
  for (size_t s = 0; s < start_count; s++)
    if (!below_p(starts + t.xw * s, 2 * E)) return fail(SBN_ERR_BAD_ARG, "coordinate >= p (start %zu)", s);
  for (size_t g = 0; g < M; g++)
    if (!below_p(terms + T * g, 2 * E)) return fail(SBN_ERR_BAD_ARG, "coordinate >= p (instance %zu, segment %u)", g, L.seg[g]);
  const Co<E> b = curve_b<E>();
  for (size_t s = 0; s < start_count; s++) {
    const Jac<E> p = ld_point<E>(starts + t.xw * s);
    if (!on_curve<E>(p.X, p.Y, b)) return fail(SBN_ERR_BAD_ARG, "start %zu is not a point of the curve", s);
  }
  const size_t bad = first_bad(M, [&](size_t g) { const Jac<E> p = ld_point<E>(terms + T * g); return !on_curve<E>(p.X, p.Y, b); });
  if (bad < M) return fail(SBN_ERR_BAD_ARG, "x of instance %zu (segment %u) is not a point of the curve", bad, L.seg[bad]);
  return SBN_OK;
}
int check_field_inputs(const PiLayout& t, const uint32_t* terms, size_t M, const Layout& L, const uint32_t* starts, size_t start_count) {
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
int check_inputs(const PiLayout& t, const uint32_t* terms, size_t M, const Layout& L, const uint32_t* starts, size_t start_count) {
  if (t.E == 1) return check_curve_inputs<1>(t, terms, M, L, starts, start_count);
  if (t.E == 2) return check_curve_inputs<2>(t, terms, M, L, starts, start_count);
  return check_field_inputs(t, terms, M, L, starts, start_count);
}

// ---- the derivation: what it cannot derive goes into `why`, worded by the entry point; it asks no one who called ------------------
template <int E>
bool derive_curve(const PiLayout& t, const uint32_t* terms, size_t M, const Layout& L, size_t segments, const uint32_t* starts, size_t start_count, size_t total,
                  uint32_t* ios, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out, ListRefusal* why) {
  const size_t T = t.T(), IOW = t.IOW(), W = t.xw;
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
    if (czero<E>(pts[g].Z)) { *why = {ListRefusal::OFFSET_AT_INFINITY, g}; return false; }
    if (g + 1 == L.head[s + 1] && czero<E>(pts[M + s].Z)) { *why = {ListRefusal::OUTPUT_AT_INFINITY, g}; return false; }
  }
  std::vector<uint32_t> aff(W * pts.size());
  std::vector<uint8_t> inf(pts.size());
  affine_or_infinity<E>(pts, aff.data(), inf.data());   // one inversion for every Z
  for (size_t g = 0; g < M; g++) {
    uint32_t* io = ios + IOW * g;
    memcpy(io, terms + T * g, W * sizeof(uint32_t));
    memcpy(io + W, aff.data() + W * g, W * sizeof(uint32_t));
    memcpy(io + 2 * W, terms + T * g + W, t.ew * sizeof(uint32_t));
  }
  pad_rows(ios, IOW, M, total);
  if (finals_out) memcpy(finals_out, aff.data() + W * M, W * segments * sizeof(uint32_t));
  if (sums_out) memcpy(sums_out, aff.data() + W * (M + segments), W * segments * sizeof(uint32_t));
  if (infinity_out) memcpy(infinity_out, inf.data() + M + segments, segments);
  const size_t bad = walk_curve_list<E>(ios, M);   // the real instances: the pads repeat the last one
  if (bad == WALKS) return true;
  *why = {bad == UNNAMED ? ListRefusal::UNNAMED_WALK : ListRefusal::DEGENERATE_WALK, bad};
  return false;
}

// the field tables: N = 1 (FQ_EXP) or 12 (the flat basis of the Fq12 tables); an Fq power is short, so a pool task takes eight
template <int N>
void derive_field(const PiLayout& t, const uint32_t* terms, size_t M, const Layout& L, size_t segments, const uint32_t* starts, size_t start_count, size_t total,
                  uint32_t* ios, uint32_t* finals_out) {
  const size_t W = 8 * N, T = t.T(), IOW = t.IOW(), G = N == 1 ? 8 : 1;
  std::vector<Fq> term((size_t)N * M);
  host_parallel_for((M + G - 1) / G, [&](size_t i) {
    for (size_t g = G * i; g < M && g < G * i + G; g++) {
      Fq x[N];
      field_load<N>(terms + T * g, x);
      field_power<N>(x, terms + T * g + W, (int)(32 * t.ew), &term[(size_t)N * g]);
    }
  });
  host_parallel_for(segments, [&](size_t s) {
    Fq off[N];
    field_load<N>(starts + (start_count == 1 ? 0 : W * s), off);
    for (size_t g = L.head[s]; g < L.head[s + 1]; g++) {
      uint32_t* io = ios + IOW * g;
      memcpy(io, terms + T * g, W * sizeof(uint32_t));
      field_store<N>(off, io + W);
      memcpy(io + 2 * W, terms + T * g + W, t.ew * sizeof(uint32_t));
      field_mul<N>(off, &term[(size_t)N * g], off);
    }
    if (finals_out) field_store<N>(off, finals_out + W * s);
  });
  pad_rows(ios, IOW, M, total);
}

bool derive(const PiLayout& t, const uint32_t* terms, size_t M, const Layout& L, size_t segments, const uint32_t* starts, size_t start_count, size_t total,
            uint32_t* ios, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out, ListRefusal* why) {
  if (t.E == 1) return derive_curve<1>(t, terms, M, L, segments, starts, start_count, total, ios, finals_out, sums_out, infinity_out, why);
  if (t.E == 2) return derive_curve<2>(t, terms, M, L, segments, starts, start_count, total, ios, finals_out, sums_out, infinity_out, why);
  if (t.xw == 8) derive_field<1>(t, terms, M, L, segments, starts, start_count, total, ios, finals_out);
  else derive_field<12>(t, terms, M, L, segments, starts, start_count, total, ios, finals_out);
  return true;
}

// ---- the complete sums: the library picks the start of every segment -------------------------------------------------------------
// offset[g] = H + P[g] with P[g] = the sum of the segment's terms before g, which no start enters: the terms and their prefix sums
// are computed once, a candidate H costs one complete addition per instance (and one for the final) of the segments still open.
// Candidate j is tried on every open segment in one pass -- the offsets, one inversion for their affine forms, the table's walk of
// the rows with a per-instance status -- and only the segments with a bad event (an offset or the final at infinity, an instance
// the table cannot walk) stay open for candidate j + 1.  A segment's bad set depends on its own terms alone, so the choice of one
// segment never moves another.  The sum is P of the whole segment: final + (-start) in canonical affine words.
template <int E>
int complete_curve(const PiLayout& t, const uint32_t* terms, size_t M, const Layout& L, size_t segments, size_t total, uint32_t* ios,
                   uint32_t* starts_out, uint8_t* choice_out, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out) {
  const size_t T = t.T(), IOW = t.IOW(), W = t.xw, NONE = (size_t)-1;
  std::vector<Jac<E>> term(M), pre(M), tot(segments);
  host_parallel_for(M, [&](size_t g) { term[g] = scalar_mul_jac<E>(ld_point<E>(terms + T * g), terms + T * g + W); });
  host_parallel_for(segments, [&](size_t s) {
    Jac<E> acc = jac_infinity<E>();
    for (size_t g = L.head[s]; g < L.head[s + 1]; g++) { pre[g] = acc; acc = jac_add_complete<E>(acc, term[g]); }
    tot[s] = acc;
  });
  for (size_t g = 0; g < M; g++) {
    memcpy(ios + IOW * g, terms + T * g, W * sizeof(uint32_t));
    memcpy(ios + IOW * g + 2 * W, terms + T * g + W, t.ew * sizeof(uint32_t));
  }
  std::vector<size_t> open(segments), bad_at(segments, NONE);
  for (size_t s = 0; s < segments; s++) open[s] = s;
  for (unsigned j = 0; j < SBN_START_CANDIDATES && !open.empty(); j++) {
    const uint32_t* hw = curve_start_candidate_words(E, j);
    const Jac<E> H = ld_point<E>(hw);
    // slot[i]: the offsets of open segment i, then its final
    std::vector<size_t> slot(open.size() + 1, 0);
    for (size_t i = 0; i < open.size(); i++) slot[i + 1] = slot[i] + (L.head[open[i] + 1] - L.head[open[i]]) + 1;
    std::vector<Jac<E>> pts(slot.back());
    host_parallel_for(open.size(), [&](size_t i) {
      const size_t s = open[i], h = L.head[s], len = L.head[s + 1] - h;
      for (size_t q = 0; q < len; q++) pts[slot[i] + q] = jac_add_complete<E>(H, pre[h + q]);
      pts[slot[i] + len] = jac_add_complete<E>(H, tot[s]);
    });
    std::vector<uint32_t> aff(W * pts.size());
    std::vector<uint8_t> inf(pts.size());
    affine_or_infinity<E>(pts, aff.data(), inf.data());   // one inversion for every Z
    // the rows whose offset the table can hold, packed for the walk
    std::vector<uint32_t> rows;
    rows.reserve(IOW * (pts.size() - open.size()));
    for (size_t i = 0; i < open.size(); i++) {
      const size_t h = L.head[open[i]], len = slot[i + 1] - slot[i] - 1;
      for (size_t q = 0; q < len; q++) {
        if (inf[slot[i] + q]) continue;
        uint32_t* io = ios + IOW * (h + q);
        memcpy(io + W, aff.data() + W * (slot[i] + q), W * sizeof(uint32_t));
        rows.insert(rows.end(), io, io + IOW);
      }
    }
    std::vector<uint8_t> unwalkable(rows.size() / IOW + 1);
    if (!walk_status<E>(rows.data(), rows.size() / IOW, unwalkable.data())) return fail(SBN_ERR_WITNESS, UNNAMED_WALK_TEXT);
    std::vector<size_t> still;
    size_t r = 0;
    for (size_t i = 0; i < open.size(); i++) {
      const size_t s = open[i], h = L.head[s], len = slot[i + 1] - slot[i] - 1;
      size_t first = NONE;
      for (size_t q = 0; q < len; q++) {
        const bool bad = inf[slot[i] + q] ? true : unwalkable[r++] != 0;
        if (bad && first == NONE) first = h + q;
      }
      if (first == NONE && inf[slot[i] + len]) first = h + len - 1;   // the output of the segment's last instance
      if (first != NONE) { bad_at[s] = first; still.push_back(s); continue; }
      if (choice_out) choice_out[s] = (uint8_t)j;
      if (starts_out) memcpy(starts_out + W * s, hw, W * sizeof(uint32_t));
      if (finals_out) memcpy(finals_out + W * s, aff.data() + W * (slot[i] + len), W * sizeof(uint32_t));
    }
    open.swap(still);
  }
  if (!open.empty())
    return fail(SBN_ERR_WITNESS, "segment %zu: every one of the %d start candidates meets a degenerate affine operation or a point at infinity in the table's walk "
                "(%zu segment%s in this state; candidate %d fails at instance %zu): such a list is crafted, call sbn_msm_batch_instances with starts of your own",
                open[0], SBN_START_CANDIDATES, open.size(), open.size() == 1 ? "" : "s", SBN_START_CANDIDATES - 1, bad_at[open[0]]);
  affine_or_infinity<E>(tot, sums_out, infinity_out);
  pad_rows(ios, IOW, M, total);
  return SBN_OK;
}

// ---- sbn_msm_batch_check on the curves: the outputs are points, and final + (-start) per segment -------------------------------------
template <int E>
int check_curve_outputs(const PiLayout& t, const std::vector<uint32_t>& outs, size_t M, const Layout& L, size_t segments, const uint32_t* starts, size_t start_count,
                        uint32_t* sums_out, uint8_t* infinity_out) {
  const size_t W = t.xw;
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
  PiLayout t;
  if (!pi_layout(kind, t)) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not an Exp table: segmented lists cover the five Exp tables", kind);
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
  PiLayout t;
  if (!pi_layout(kind, t)) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not an Exp table", kind);
  return check_inputs(t, terms, M, Layout(lengths, segments, M), starts, start_count);
}

bool segmented_derive(int kind, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts, size_t start_count, size_t M,
                      size_t total, uint32_t* ios, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out, ListRefusal* why) {
  return derive(pi_layout(kind), terms, M, Layout(lengths, segments, M), segments, starts, start_count, total, ios, finals_out, sums_out, infinity_out, why);
}

int msm_batch_derive(int kind, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts, size_t start_count, size_t M,
                     size_t total, uint32_t* ios, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out) {
  PiLayout t;
  if (!pi_layout(kind, t)) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not an Exp table", kind);
  const Layout L(lengths, segments, M);
  if (int rc = check_inputs(t, terms, M, L, starts, start_count)) return rc;
  ListRefusal why;
  if (derive(t, terms, M, L, segments, starts, start_count, total, ios, finals_out, sums_out, infinity_out, &why)) return SBN_OK;
  const size_t g = why.at, s = why.what == ListRefusal::UNNAMED_WALK ? 0 : L.seg[g];
  switch (why.what) {
    case ListRefusal::OFFSET_AT_INFINITY: return fail(SBN_ERR_WITNESS, "the offset of instance %zu (segment %zu) is the point at infinity", g, s);
    case ListRefusal::OUTPUT_AT_INFINITY: return fail(SBN_ERR_WITNESS, "the output of instance %zu (segment %zu) is the point at infinity", g, s);
    case ListRefusal::DEGENERATE_WALK:
      return fail(SBN_ERR_WITNESS, "instance %zu (segment %zu): degenerate affine operation in the table's walk (B[t] = +-2^t x at a set bit): pick another start", g, s);
    default: return fail(SBN_ERR_WITNESS, UNNAMED_WALK_TEXT);
  }
}

int msm_batch_complete_args(int kind, const void* terms, const uint64_t* lengths, size_t segments, size_t num_io, size_t* M_out) {
  PiLayout t;
  if (pi_layout(kind, t) && !t.E)
    return fail(SBN_ERR_UNSUPPORTED, "complete sums cover the curve tables G1_EXP and G2_EXP (a field table's offset one is always legal: sbn_msm_batch_instances)");
  const uint32_t* starts = nullptr;
  size_t start_count = 1;
  return msm_batch_check_args(kind, terms, lengths, segments, &starts, &start_count, num_io, nullptr, nullptr, M_out);
}

int msm_batch_effective_terms(int kind, const uint32_t* terms, const uint8_t* term_infinity, const uint64_t* lengths, size_t segments, size_t M, uint32_t* terms_eff) {
  const PiLayout t = pi_layout(kind);
  const size_t T = t.T();
  for (size_t g = 0; g < M; g++) {
    if (term_infinity && term_infinity[g]) {   // the identity: a point of the curve with exponent 0, its walk has no addition
      memcpy(terms_eff + T * g, curve_generator_words(t.E), t.xw * sizeof(uint32_t));
      memset(terms_eff + T * g + t.xw, 0, t.ew * sizeof(uint32_t));
    } else memcpy(terms_eff + T * g, terms + T * g, T * sizeof(uint32_t));
  }
  return check_inputs(t, terms_eff, M, Layout(lengths, segments, M), nullptr, 0);
}

int msm_batch_complete_choose(int kind, const uint32_t* terms_eff, const uint64_t* lengths, size_t segments, size_t M, size_t total, uint32_t* ios,
                              uint32_t* starts_out, uint8_t* choice_out, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out) {
  const PiLayout t = pi_layout(kind);
  const Layout L(lengths, segments, M);
  std::vector<uint32_t> own;
  if (!ios) { own.resize(t.IOW() * total); ios = own.data(); }
  return t.E == 1 ? complete_curve<1>(t, terms_eff, M, L, segments, total, ios, starts_out, choice_out, finals_out, sums_out, infinity_out)
                  : complete_curve<2>(t, terms_eff, M, L, segments, total, ios, starts_out, choice_out, finals_out, sums_out, infinity_out);
}
}  // namespace sbn

extern "C" int sbn_msm_batch_instances_complete(int32_t kind, const uint32_t* terms, const uint8_t* term_infinity, const uint64_t* lengths, size_t segments, size_t num_io,
                                                uint32_t* ios_out, uint32_t* terms_out, uint32_t* starts_out, uint8_t* choice_out, uint32_t* finals_out,
                                                uint32_t* sums_out, uint8_t* infinity_out) {
  size_t M = 0;
  if (int rc = msm_batch_complete_args((int)kind, terms, lengths, segments, num_io, &M)) return rc;
  std::vector<uint32_t> own;
  if (!terms_out) { own.resize(pi_layout((int)kind).T() * M); terms_out = own.data(); }
  if (int rc = msm_batch_effective_terms((int)kind, terms, term_infinity, lengths, segments, M, terms_out)) return rc;
  return msm_batch_complete_choose((int)kind, terms_out, lengths, segments, M, sbn_msm_num_units(M, num_io) * num_io, ios_out, starts_out, choice_out, finals_out,
                                   sums_out, infinity_out);
}

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
  PiLayout t;
  if (!pi_layout((int)kind, t)) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not an Exp table: segmented lists cover the five Exp tables", (int)kind);
  if (!public_inputs) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (int rc = msm_batch_check_args((int)kind, public_inputs, lengths, segments, &starts, &start_count, num_io, sums_out, infinity_out, &M)) return rc;
  if (units != sbn_msm_num_units(M, num_io))
    return fail(SBN_ERR_VERIFY_FAILED, "%zu units given, %zu segments of %zu instances in tables of %zu have %zu units", units, segments, M, num_io, sbn_msm_num_units(M, num_io));
  const UnitInputs U((int)kind, num_io, public_inputs, units);
  if (int rc = U.null_unit()) return rc;
  if (!below_p(starts, t.values() * (int)start_count)) return fail(SBN_ERR_BAD_ARG, "%s >= p (starts)", t.E ? "coordinate" : "coefficient");
  const Layout L(lengths, segments, M);
  std::vector<uint32_t> outs(t.xw * M);
  for (size_t g = 0; g < U.rows(); g++) {
    if (g >= M) { if (int rc = U.pad(g, M - 1)) return rc; continue; }
    const size_t s = L.seg[g];
    if (terms) {
      if (!U.value_is(g, U.oX, terms + t.T() * g)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %zu): x differs from the caller's term", g, s);
      if (!U.exp_is(g, terms + t.T() * g + t.xw)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %zu): exponent differs from the caller's term", g, s);
    }
    if (g == L.head[s]) {
      if (!U.value_is(g, U.oOff, starts + (start_count == 1 ? 0 : t.xw * s)))
        return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %zu): offset differs from the start of the segment", g, s);
    } else if (!same(U.inst(g) + U.oOff, U.inst(g - 1) + U.oOut, t.W))
      return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %zu): offset differs from the output of instance %zu", g, s, g - 1);
    size_t limb;
    if (!U.output(g, outs.data() + t.xw * g, &limb)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (segment %zu): output limb %zu is out of range", g, s, limb);
  }
  if (t.E == 1) { if (int rc = check_curve_outputs<1>(t, outs, M, L, segments, starts, start_count, sums_out, infinity_out)) return rc; }
  else if (t.E == 2) { if (int rc = check_curve_outputs<2>(t, outs, M, L, segments, starts, start_count, sums_out, infinity_out)) return rc; }
  if (finals_out) for (size_t s = 0; s < segments; s++) memcpy(finals_out + t.xw * s, outs.data() + t.xw * (L.head[s + 1] - 1), t.xw * sizeof(uint32_t));
  return SBN_OK;
}
