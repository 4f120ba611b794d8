// Curve programs (include/sbn.h, "Curve programs"): the field programs of program.hip on the two curve tables G1ExpStark and
// G2ExpStark.  An instance is output = offset + e x; a program is a list of instances whose x and offset are each a literal point
// or the output of an EARLIER instance, and whose offset may be the start the library picks.  An output used as x drags a multiple
// of that start along, so every output is carried as value + blind: the blind T_g = T_off + e_g T_x is a function of the start,
// the exponents and the shape alone, and value_g = out_g + (-T_g) is what the caller means.  Here
//  * sbn_curve_program_instances derives outputs and blinds level by level (sbn_program_levels, unchanged) on the host pool in
//    Jacobian coordinates with the COMPLETE addition (a value may be the identity and says nothing about the table's walk), takes
//    ONE inversion for the affine form of every output, lays out the explicit list and lets the table walk it; a bad event (an
//    output at infinity, an instance the table cannot walk) sends the whole program to the next start candidate;
//  * sbn_curve_program_check reads the public inputs of the unit proofs, states the links a circuit would `connect`, recomputes the
//    blinds from the choice and the exponents and returns the values.  It verifies no proof.
// Host code only: no kernel is launched from this unit (tracegen_device.hip holds the device form).
#include "instance_lists.hpp"
#include <cstdio>

using namespace sbn;

namespace {
using namespace bnw;
using namespace sbn::curve_host;

constexpr size_t INDEX_LIMIT = 0x7fffffffu;   // count, n_points and n_exps stay below the sentinels: an index never reads as one
constexpr size_t NONE = (size_t)-1;
inline bool literal(uint32_t v) { return !linked(v) && v != SBN_NODE_START && v != SBN_NODE_ONE; }

// refusals 1 and 2
int check_args(int32_t kind, const void* nodes, const void* points, const void* exps, size_t count, size_t n_points, size_t n_exps, size_t num_io) {
  if (kind != SBN_AIR_G1_EXP && kind != SBN_AIR_G2_EXP)
    return fail(SBN_ERR_UNSUPPORTED, "curve programs cover the curve tables G1_EXP and G2_EXP (the field tables have sbn_program_instances)");
  if (!nodes || !points || !exps || count == 0 || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no node or num_io = 0");
  if (count >= INDEX_LIMIT || n_points >= INDEX_LIMIT || n_exps >= INDEX_LIMIT) return fail(SBN_ERR_BAD_ARG, "count, n_points and n_exps must be below 2^31 - 1");
  return SBN_OK;
}

// refusal 3, node by node
int check_nodes(const sbn_program_node* nodes, size_t count, size_t n_points, size_t n_exps) {
  static const char* const field[2] = {"x", "offset"};
  for (size_t g = 0; g < count; g++) {
    const uint32_t op[2] = {nodes[g].x, nodes[g].offset};
    for (int f = 0; f < 2; f++)
      if (linked(op[f]) && link_of(op[f]) >= g) return fail(SBN_ERR_BAD_ARG, "node %zu: %s links to node %u, which is no earlier node", g, field[f], link_of(op[f]));
    for (int f = 0; f < 2; f++)
      if (literal(op[f]) && op[f] >= n_points) return fail(SBN_ERR_BAD_ARG, "node %zu: %s is literal %u of %zu", g, field[f], op[f], n_points);
    for (int f = 0; f < 2; f++)
      if (op[f] == SBN_NODE_ONE) return fail(SBN_ERR_BAD_ARG, "node %zu: %s is SBN_NODE_ONE, which a curve table does not have", g, field[f]);
    if (op[0] == SBN_NODE_START) return fail(SBN_ERR_BAD_ARG, "node %zu: x is SBN_NODE_START, which only an offset may be", g);
    if (nodes[g].exp >= n_exps) return fail(SBN_ERR_BAD_ARG, "node %zu: exponent is index %u of %zu", g, nodes[g].exp, n_exps);
  }
  return SBN_OK;
}

// refusal 4: the literals some node uses, in index order; a coordinate >= p first, then a point off the curve
template <int E> int check_used_points(const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points) {
  const size_t W = 16 * E;
  std::vector<uint8_t> used(n_points, 0);
  for (size_t g = 0; g < count; g++) {
    if (literal(nodes[g].x)) used[nodes[g].x] = 1;
    if (literal(nodes[g].offset)) used[nodes[g].offset] = 1;
  }
  for (size_t i = 0; i < n_points; i++)
    if (used[i] && !below_p(points + W * i, 2 * E)) return fail(SBN_ERR_BAD_ARG, "coordinate >= p (literal %zu)", i);
  const Co<E> b = curve_b<E>();
  const size_t bad = first_bad(n_points, [&](size_t i) {
    if (!used[i]) return false;
    const Jac<E> p = ld_point<E>(points + W * i);
    return !on_curve<E>(p.X, p.Y, b);
  });
  if (bad < n_points) return fail(SBN_ERR_BAD_ARG, "literal %zu is not a point of the curve", bad);
  return SBN_OK;
}

// the schedule: sbn_program_levels, then fill_plan's sort by level
int schedule(const sbn_program_node* nodes, size_t count, ProgramPlan& plan) {
  plan.level.resize(count);
  if (int rc = sbn_program_levels(nodes, count, plan.level.data(), nullptr)) return rc;
  fill_plan(plan.level.data(), count, count, plan);
  return SBN_OK;
}

// T_g = T_off + e_g T_x from the start S, level by level: a literal contributes the identity, SBN_NODE_START contributes S
template <int E> std::vector<Jac<E>> blinds(const ProgramPlan& plan, const sbn_program_node* nodes, const uint32_t* exps, const Jac<E>& S) {
  std::vector<Jac<E>> T(plan.order.size());
  for (size_t l = 0; l < plan.depth(); l++) {
    const uint32_t* at = plan.order.data() + plan.level_start[l];
    host_parallel_for(plan.level_start[l + 1] - plan.level_start[l], [&](size_t i) {
      const size_t g = at[i];
      const sbn_program_node& nd = nodes[g];
      const Jac<E> tx = linked(nd.x) ? T[link_of(nd.x)] : jac_infinity<E>();
      const Jac<E> toff = linked(nd.offset) ? T[link_of(nd.offset)] : (nd.offset == SBN_NODE_START ? S : jac_infinity<E>());
      T[g] = czero<E>(tx.Z) ? toff : jac_add_complete<E>(toff, scalar_mul_jac<E>(tx, exps + 8 * nd.exp));
    });
  }
  return T;
}

// One candidate: the outputs of every node from the start `sw`, their affine form, rows [0, count) of ios, and the table's walk.
// Returns NONE when no node has a bad event, else the first node with one; *unnamed: the table refuses the list and no single
// instance of it (curve_host::UNNAMED).  out: the Jacobian outputs, aff: [count][W] affine words.
template <int E>
size_t derive_outputs(const ProgramPlan& plan, const sbn_program_node* nodes, size_t count, const uint32_t* points, const uint32_t* exps, const uint32_t* sw,
                      std::vector<Jac<E>>& out, std::vector<uint32_t>& aff, uint32_t* ios, bool* unnamed) {
  const size_t W = 16 * E, IOW = 2 * W + 8;
  const Jac<E> S = ld_point<E>(sw);
  out.resize(count);
  for (size_t l = 0; l < plan.depth(); l++) {
    const uint32_t* at = plan.order.data() + plan.level_start[l];
    host_parallel_for(plan.level_start[l + 1] - plan.level_start[l], [&](size_t i) {
      const size_t g = at[i];
      const sbn_program_node& nd = nodes[g];
      const Jac<E> x = linked(nd.x) ? out[link_of(nd.x)] : ld_point<E>(points + W * nd.x);
      const Jac<E> off = linked(nd.offset) ? out[link_of(nd.offset)] : (nd.offset == SBN_NODE_START ? S : ld_point<E>(points + W * nd.offset));
      out[g] = jac_add_complete<E>(off, scalar_mul_jac<E>(x, exps + 8 * nd.exp));
    });
  }
  aff.resize(W * count);
  std::vector<uint8_t> inf(count);
  affine_or_infinity<E>(out, aff.data(), inf.data());   // one inversion for every Z
  // An output at infinity is a bad event of its node, and everything before the first one has finite operands: those rows exist.
  size_t rows = count;
  for (size_t g = 0; g < count; g++) if (inf[g]) { rows = g; break; }
  for (size_t g = 0; g < rows; g++) {
    const sbn_program_node& nd = nodes[g];
    uint32_t* io = ios + IOW * g;
    memcpy(io, linked(nd.x) ? aff.data() + W * link_of(nd.x) : points + W * nd.x, W * sizeof(uint32_t));
    memcpy(io + W, linked(nd.offset) ? aff.data() + W * link_of(nd.offset) : (nd.offset == SBN_NODE_START ? sw : points + W * nd.offset), W * sizeof(uint32_t));
    memcpy(io + 2 * W, exps + 8 * nd.exp, 8 * sizeof(uint32_t));
  }
  *unnamed = false;
  const size_t bad = rows ? walk_curve_list<E>(ios, rows) : WALKS;
  if (bad == UNNAMED) { *unnamed = true; return 0; }
  if (bad != WALKS) return bad;
  return rows < count ? rows : NONE;
}

template <int E> void values_of(const std::vector<Jac<E>>& out, const std::vector<Jac<E>>& T, uint32_t* values_out, uint8_t* infinity_out) {
  if (!values_out && !infinity_out) return;
  std::vector<Jac<E>> v(out.size());
  host_parallel_for(out.size(), [&](size_t g) { v[g] = jac_add_complete<E>(out[g], neg_point<E>(T[g])); });
  affine_or_infinity<E>(v, values_out, infinity_out);
}

template <int E>
int instances(const ProgramPlan& plan, const sbn_program_node* nodes, size_t count, const uint32_t* points, const uint32_t* exps, size_t total,
              uint32_t* ios, uint32_t* outs_out, uint32_t* values_out, uint8_t* infinity_out, uint8_t* choice_out) {
  const size_t W = 16 * E, IOW = 2 * W + 8;
  std::vector<Jac<E>> out;
  std::vector<uint32_t> aff;
  size_t bad = NONE;
  for (unsigned j = 0; j < SBN_START_CANDIDATES; j++) {
    const uint32_t* sw = curve_start_candidate_words(E, j);
    bool unnamed;
    bad = derive_outputs<E>(plan, nodes, count, points, exps, sw, out, aff, ios, &unnamed);
    if (unnamed) return fail(SBN_ERR_WITNESS, UNNAMED_WALK_TEXT);
    if (bad != NONE) continue;
    values_of<E>(out, blinds<E>(plan, nodes, exps, ld_point<E>(sw)), values_out, infinity_out);
    if (outs_out) memcpy(outs_out, aff.data(), W * count * sizeof(uint32_t));
    if (choice_out) *choice_out = (uint8_t)j;
    pad_rows(ios, IOW, count, total);
    return SBN_OK;
  }
  // the node holds a start when SBN_NODE_START lies anywhere under it: only then does a candidate move its events
  std::vector<uint8_t> holds(count, 0);
  for (size_t g = 0; g <= bad; g++) {
    const sbn_program_node& nd = nodes[g];
    holds[g] = nd.offset == SBN_NODE_START || (linked(nd.x) && holds[link_of(nd.x)]) || (linked(nd.offset) && holds[link_of(nd.offset)]);
  }
  return fail(SBN_ERR_WITNESS, "every one of the %d start candidates meets a degenerate affine operation or a point at infinity in the table's walk "
              "(candidate %d fails at node %zu)%s", SBN_START_CANDIDATES, SBN_START_CANDIDATES - 1, bad,
              holds[bad] ? ": such a program is crafted from the published candidates"
                         : ": that node holds no SBN_NODE_START, its operands are the caller's literals and no candidate can mend it");
}

// 0: the W words are a point of the curve; 1: a coordinate >= p; 2: off the curve
template <int E> int output_fault(const uint32_t* o) {
  if (!below_p(o, 2 * E)) return 1;
  const Jac<E> q = ld_point<E>(o);
  return on_curve<E>(q.X, q.Y, curve_b<E>()) ? 0 : 2;
}

template <int E>
void check_values(const ProgramPlan& plan, const sbn_program_node* nodes, size_t count, const uint32_t* exps, unsigned choice, const std::vector<uint32_t>& outs,
                  uint32_t* values_out, uint8_t* infinity_out) {
  std::vector<Jac<E>> out(count);
  for (size_t g = 0; g < count; g++) out[g] = ld_point<E>(outs.data() + 16 * E * g);
  values_of<E>(out, blinds<E>(plan, nodes, exps, ld_point<E>(curve_start_candidate_words(E, choice))), values_out, infinity_out);
}
}  // namespace

namespace sbn {
int curve_program_plan(int kind, const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points, const uint32_t* exps, size_t n_exps,
                       size_t num_io, ProgramPlan& plan) {
  if (int rc = check_args(kind, nodes, points, exps, count, n_points, n_exps, num_io)) return rc;
  if (int rc = check_nodes(nodes, count, n_points, n_exps)) return rc;
  if (int rc = kind == SBN_AIR_G1_EXP ? check_used_points<1>(nodes, count, points, n_points) : check_used_points<2>(nodes, count, points, n_points)) return rc;
  return schedule(nodes, count, plan);
}

void curve_program_neg_blinds(int E, const ProgramPlan& plan, const sbn_program_node* nodes, const uint32_t* exps, unsigned choice, uint32_t* neg_blinds,
                              uint8_t* flag) {
  const uint32_t* sw = curve_start_candidate_words(E, choice);
  if (E == 1) {
    std::vector<Jac<1>> T = blinds<1>(plan, nodes, exps, ld_point<1>(sw));
    for (Jac<1>& t : T) t = neg_point<1>(t);
    affine_or_infinity<1>(T, neg_blinds, flag);
  } else {
    std::vector<Jac<2>> T = blinds<2>(plan, nodes, exps, ld_point<2>(sw));
    for (Jac<2>& t : T) t = neg_point<2>(t);
    affine_or_infinity<2>(T, neg_blinds, flag);
  }
}
}  // namespace sbn

extern "C" int sbn_curve_program_instances(int32_t kind, const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points,
                                           const uint32_t* exps, size_t n_exps, size_t num_io, uint32_t* ios_out, uint32_t* outs_out,
                                           uint32_t* values_out, uint8_t* infinity_out, uint8_t* choice_out) {
  ProgramPlan plan;
  if (int rc = curve_program_plan((int)kind, nodes, count, points, n_points, exps, n_exps, num_io, plan)) return rc;
  const size_t total = sbn_msm_num_units(count, num_io) * num_io;
  std::vector<uint32_t> own;
  uint32_t* ios = ios_out;
  if (!ios) { own.resize(exp_io_words((int)kind) * total); ios = own.data(); }
  return kind == SBN_AIR_G1_EXP ? instances<1>(plan, nodes, count, points, exps, total, ios, outs_out, values_out, infinity_out, choice_out)
                                : instances<2>(plan, nodes, count, points, exps, total, ios, outs_out, values_out, infinity_out, choice_out);
}

extern "C" int sbn_curve_program_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units,
                                       const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points,
                                       const uint32_t* exps, size_t n_exps, uint32_t choice, uint32_t* outs_out, uint32_t* values_out,
                                       uint8_t* infinity_out) {
  if (int rc = check_args(kind, nodes, points, exps, count, n_points, n_exps, num_io)) return rc;
  if (int rc = check_nodes(nodes, count, n_points, n_exps)) return rc;
  if (!public_inputs) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (choice >= SBN_START_CANDIDATES) return fail(SBN_ERR_BAD_ARG, "choice %u: there are %d start candidates", choice, SBN_START_CANDIDATES);
  if (units != sbn_msm_num_units(count, num_io))
    return fail(SBN_ERR_VERIFY_FAILED, "%zu units given, a program of %zu nodes in tables of %zu has %zu units", units, count, num_io, sbn_msm_num_units(count, num_io));
  const UnitInputs U((int)kind, num_io, public_inputs, units);
  if (int rc = U.null_unit()) return rc;
  const PiLayout& L = U.L;
  const uint32_t* sw = curve_start_candidate_words(L.E, choice);
  std::vector<uint32_t> outs(L.xw * count);
  char not_start[48];
  snprintf(not_start, sizeof not_start, "differs from start candidate %u", choice);
  const int links = check_program_links(U, nodes, count, points, exps,
    [&](uint32_t op, const char** what) -> const uint32_t* { *what = not_start; return op == SBN_NODE_START ? sw : nullptr; },
    [&](size_t g) {
      size_t limb;
      if (!U.output(g, outs.data() + L.xw * g, &limb)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output limb %zu is out of range", g, limb);
      const int fault = L.E == 1 ? output_fault<1>(outs.data() + L.xw * g) : output_fault<2>(outs.data() + L.xw * g);
      if (fault) return fail(SBN_ERR_VERIFY_FAILED, fault == 1 ? "instance %zu: output has a coordinate >= p" : "instance %zu: output is not a point of the curve", g);
      return (int)SBN_OK;
    });
  if (links != SBN_OK) return links;
  if (values_out || infinity_out) {
    ProgramPlan plan;
    if (int rc = schedule(nodes, count, plan)) return rc;
    if (L.E == 1) check_values<1>(plan, nodes, count, exps, choice, outs, values_out, infinity_out);
    else check_values<2>(plan, nodes, count, exps, choice, outs, values_out, infinity_out);
  }
  if (outs_out) memcpy(outs_out, outs.data(), outs.size() * sizeof(uint32_t));
  return SBN_OK;
}
