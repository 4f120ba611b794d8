// Field programs (include/sbn.h, "Field programs"): the general form of the linked lists of the three field Exp tables FqExpStark,
// Fq12ExpStark and Fq12ExpU64Stark.  An instance is output = offset * x^e; a program is a list of instances whose x and offset
// are each a literal or the output of an EARLIER instance, which covers the chained list (offset = the previous output), the tower
// (x = the previous output) and everything between them: products of two earlier results, Frobenius maps, Horner over the limbs of
// a long exponent.  Here
//  * sbn_program_levels is the schedule: level 0 for a node without links, otherwise 1 + the largest level it links to.  The nodes
//    of one level are independent, so the host pool takes a level at a time and the device one launch per level
//    (kernels_tracegen.cuh, "field programs");
//  * sbn_program_instances builds the explicit, padded, unit-cut list and the outputs on the host pool by the table's own walk;
//  * sbn_program_check reads the public inputs of the unit proofs and states the links a circuit would `connect`.  It verifies no
//    proof;
//  * the sbn_program_m_* twins take nodes with a fourth word, the Frobenius maps of x and offset (include/sbn.h, "Mapped links and
//    the final exponentiation"): an entry point splits them into the unmapped nodes and a vector of maps, and everything behind it
//    takes (nodes, maps), maps null for the unmapped calls; sbn_fq12_frobenius and sbn_fq12_inverse are the host helpers.
// Host code only: no kernel is launched from this unit (tracegen_device.hip holds the device form).
#include "instance_lists.hpp"

using namespace sbn;

namespace {
using namespace bnw;
using namespace sbn::curve_host;

constexpr size_t INDEX_LIMIT = 0x7fffffffu;   // count, n_values and n_exps stay below SBN_NODE_ONE: an index never reads as a link or as one

// Refusal 3 of the header, node by node; no_bound: structure only (sbn_program_levels knows no n_values and no n_exps).  Fills
// level[count] (optional) and *depth.  maps (optional, [count]): the added refusals of a mapped program, node by node behind the
// existing ones of that node; fq: the table is FQ_EXP, which takes no map (sbn_program_m_levels knows no table: false).
int walk_nodes(const sbn_program_node* nodes, const uint32_t* maps, bool fq, size_t count, size_t n_values, size_t n_exps, bool no_bound, uint32_t* level, uint32_t* depth) {
  std::vector<uint32_t> own;
  if (!level) { own.resize(count); level = own.data(); }
  uint32_t deepest = 0;
  for (size_t g = 0; g < count; g++) {
    const uint32_t op[2] = {nodes[g].x, nodes[g].offset};
    static const char* const field[2] = {"x", "offset"};
    for (int f = 0; f < 2; f++)
      if (linked(op[f]) && link_of(op[f]) >= g) return fail(SBN_ERR_BAD_ARG, "node %zu: %s links to node %u, which is no earlier node", g, field[f], link_of(op[f]));
    if (!no_bound)
      for (int f = 0; f < 2; f++)
        if (!linked(op[f]) && op[f] != SBN_NODE_ONE && op[f] >= n_values)
          return fail(SBN_ERR_BAD_ARG, "node %zu: %s is literal %u of %zu", g, field[f], op[f], n_values);
    if (op[0] == SBN_NODE_ONE) return fail(SBN_ERR_BAD_ARG, "node %zu: x is SBN_NODE_ONE, which only an offset may be", g);
    if (!no_bound && nodes[g].exp >= n_exps) return fail(SBN_ERR_BAD_ARG, "node %zu: exponent is index %u of %zu", g, nodes[g].exp, n_exps);
    if (maps && maps[g]) {
      if (maps[g] >> 16) return fail(SBN_ERR_BAD_ARG, "node %zu: maps has bits 16..31 set (0x%08x)", g, maps[g]);
      for (int f = 0; f < 2; f++) if (map_of(maps, g, f) > 11) return fail(SBN_ERR_BAD_ARG, "node %zu: the map of %s is %u, a Frobenius map is 0 .. 11", g, field[f], map_of(maps, g, f));
      for (int f = 0; f < 2; f++)
        if (map_of(maps, g, f) && !linked(op[f])) return fail(SBN_ERR_BAD_ARG, "node %zu: %s carries map %u and is no link (the caller maps a literal itself)", g, field[f], map_of(maps, g, f));
      if (fq) return fail(SBN_ERR_UNSUPPORTED, "node %zu: %s carries map %u, and a Frobenius map is an Fq12 notion (FQ_EXP takes none)", g, field[map_of(maps, g, 0) ? 0 : 1], map_of(maps, g, map_of(maps, g, 0) ? 0 : 1));
    }
    uint32_t l = 0;
    for (int f = 0; f < 2; f++) if (linked(op[f]) && level[link_of(op[f])] + 1 > l) l = level[link_of(op[f])] + 1;
    level[g] = l;
    if (l > deepest) deepest = l;
  }
  if (depth) *depth = deepest + 1;
  return SBN_OK;
}

// refusals 1 and 2
int check_args(int32_t kind, const void* nodes, const void* values, const void* exps, size_t count, size_t n_values, size_t n_exps, size_t num_io) {
  if (!pi_layout((int)kind).field()) return fail(SBN_ERR_UNSUPPORTED, "field programs cover the field tables FQ_EXP, FQ12_EXP and FQ12_EXP_U64 (a curve output drags its start along)");
  if (!nodes || !values || !exps || count == 0 || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no node or num_io = 0");
  if (count >= INDEX_LIMIT || n_values >= INDEX_LIMIT || n_exps >= INDEX_LIMIT) return fail(SBN_ERR_BAD_ARG, "count, n_values and n_exps must be below 2^31 - 1");
  return SBN_OK;
}

// refusal 4: the literals, then the exponents, that some node uses, in index order
int check_used_values(int kind, const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values, const uint32_t* exps, size_t n_exps) {
  const PiLayout t = pi_layout(kind);
  std::vector<uint8_t> used_v(n_values, 0), used_e(n_exps, 0);
  for (size_t g = 0; g < count; g++) {
    if (!linked(nodes[g].x)) used_v[nodes[g].x] = 1;
    if (!linked(nodes[g].offset) && nodes[g].offset != SBN_NODE_ONE) used_v[nodes[g].offset] = 1;
    used_e[nodes[g].exp] = 1;
  }
  for (size_t i = 0; i < n_values; i++)
    if (used_v[i] && !below_p(values + t.xw * i, t.values())) return fail(SBN_ERR_BAD_ARG, "%s >= p (literal %zu)", t.xw == 8 ? "value" : "coefficient", i);
  if (kind == SBN_AIR_FQ12_EXP_U64)
    for (size_t i = 0; i < n_exps; i++)
      if (used_e[i] && ((u64)exps[2 * i] | ((u64)exps[2 * i + 1] << 32)) >= GLP) return fail(SBN_ERR_NON_CANONICAL, "exponent %zu is not a canonical field element", i);
  return SBN_OK;
}

// the nodes, level by level; out: [count][N] Montgomery outputs; rows [0, count) of ios (optional) and outs (optional, [count][8N])
template <int N>
void run_levels(const PiLayout& t, const ProgramPlan& plan, const sbn_program_node* nodes, const uint32_t* maps, const uint32_t* values, const uint32_t* exps, uint32_t* ios, uint32_t* outs) {
  const size_t W = t.xw, ew = t.ew, IOW = t.IOW();
  std::vector<Fq> out(plan.order.size() * N);
  for (size_t l = 0; l < plan.depth(); l++) {
    const uint32_t* at = plan.order.data() + plan.level_start[l];
    host_parallel_for(plan.level_start[l + 1] - plan.level_start[l], [&](size_t i) {
      const size_t g = at[i];
      const sbn_program_node& nd = nodes[g];
      const uint32_t* e = exps + ew * nd.exp;
      Fq x[N], off[N], pw[N];
      if (linked(nd.x)) memcpy(x, out.data() + (size_t)N * link_of(nd.x), sizeof x);
      else field_load<N>(values + W * nd.x, x);
      if (linked(nd.offset)) memcpy(off, out.data() + (size_t)N * link_of(nd.offset), sizeof off);
      else if (nd.offset == SBN_NODE_ONE) { for (int c = 0; c < N; c++) off[c] = Fq{{0, 0, 0, 0}}; off[0] = fq_one(); }
      else field_load<N>(values + W * nd.offset, off);
      if (N == 12) {   // a mapped link (walk_nodes: only a link carries a map, and only on the Fq12 tables)
        if (const unsigned m = map_of(maps, g, 0)) fq12_frobenius_m(x, m, x);
        if (const unsigned m = map_of(maps, g, 1)) fq12_frobenius_m(off, m, off);
      }
      if (ios) {
        uint32_t* io = ios + IOW * g;
        field_store<N>(x, io);
        field_store<N>(off, io + W);
        memcpy(io + 2 * W, e, ew * sizeof(uint32_t));
      }
      field_power<N>(x, e, (int)(32 * ew), pw);
      field_mul<N>(off, pw, out.data() + (size_t)N * g);
      if (outs) field_store<N>(out.data() + (size_t)N * g, outs + W * g);
    });
  }
}
}  // namespace

namespace sbn {
int program_plan(int kind, const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values, const uint32_t* exps, size_t n_exps,
                 size_t num_io, ProgramPlan& plan, const uint32_t* maps) {
  if (int rc = check_args(kind, nodes, values, exps, count, n_values, n_exps, num_io)) return rc;
  plan.level.resize(count);
  if (int rc = walk_nodes(nodes, maps, kind == SBN_AIR_FQ_EXP, count, n_values, n_exps, false, plan.level.data(), nullptr)) return rc;
  if (int rc = check_used_values(kind, nodes, count, values, n_values, exps, n_exps)) return rc;
  fill_plan(plan.level.data(), count, count, plan);
  return SBN_OK;
}
}  // namespace sbn

extern "C" int sbn_program_levels(const sbn_program_node* nodes, size_t count, uint32_t* level_out, uint32_t* depth_out) {
  if (!nodes || count == 0) return fail(SBN_ERR_BAD_ARG, "null argument or no node");
  if (count >= INDEX_LIMIT) return fail(SBN_ERR_BAD_ARG, "count must be below 2^31 - 1");
  return walk_nodes(nodes, nullptr, false, count, 0, 0, true, level_out, depth_out);
}
extern "C" int sbn_program_m_levels(const sbn_program_node_m* nodes, size_t count, uint32_t* level_out, uint32_t* depth_out) {
  if (!nodes || count == 0) return fail(SBN_ERR_BAD_ARG, "null argument or no node");
  if (count >= INDEX_LIMIT) return fail(SBN_ERR_BAD_ARG, "count must be below 2^31 - 1");
  std::vector<sbn_program_node> plain; std::vector<uint32_t> maps;
  split_nodes(nodes, count, plain, maps);
  return walk_nodes(plain.data(), maps.data(), false, count, 0, 0, true, level_out, depth_out);
}

namespace sbn {
int program_instances(int kind, const sbn_program_node* nodes, const uint32_t* maps, size_t count, const uint32_t* values, size_t n_values,
                      const uint32_t* exps, size_t n_exps, size_t num_io, uint32_t* ios_out, uint32_t* outs_out) {
  ProgramPlan plan;
  if (int rc = program_plan(kind, nodes, count, values, n_values, exps, n_exps, num_io, plan, maps)) return rc;
  const PiLayout t = pi_layout(kind);
  if (t.values() == 1) run_levels<1>(t, plan, nodes, maps, values, exps, ios_out, outs_out);
  else run_levels<12>(t, plan, nodes, maps, values, exps, ios_out, outs_out);
  if (ios_out) pad_rows(ios_out, t.IOW(), count, sbn_msm_num_units(count, num_io) * num_io);
  return SBN_OK;
}
}  // namespace sbn

extern "C" int sbn_program_instances(int32_t kind, const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values,
                                     const uint32_t* exps, size_t n_exps, size_t num_io, uint32_t* ios_out, uint32_t* outs_out) {
  return program_instances((int)kind, nodes, nullptr, count, values, n_values, exps, n_exps, num_io, ios_out, outs_out);
}
// The unmapped twin of a mapped node table for the two calls below.  A table that refusal 2 turns away (null, empty, too long) is
// not split: it goes on as it is, null or not, and is refused there before a node is read.
static const sbn_program_node* split_or_pass(const sbn_program_node_m* nodes, size_t count, std::vector<sbn_program_node>& plain, std::vector<uint32_t>& maps) {
  if (!nodes || count == 0 || count >= INDEX_LIMIT) return (const sbn_program_node*)nodes;
  split_nodes(nodes, count, plain, maps);
  return plain.data();
}
extern "C" int sbn_program_m_instances(int32_t kind, const sbn_program_node_m* nodes, size_t count, const uint32_t* values, size_t n_values,
                                       const uint32_t* exps, size_t n_exps, size_t num_io, uint32_t* ios_out, uint32_t* outs_out) {
  std::vector<sbn_program_node> plain; std::vector<uint32_t> maps;
  const sbn_program_node* twin = split_or_pass(nodes, count, plain, maps);
  return program_instances((int)kind, twin, maps.data(), count, values, n_values, exps, n_exps, num_io, ios_out, outs_out);
}

static int program_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units,
                         const sbn_program_node* nodes, const uint32_t* maps, size_t count, const uint32_t* values, size_t n_values,
                         const uint32_t* exps, size_t n_exps, uint32_t* outs_out) {
  if (int rc = check_args(kind, nodes, values, exps, count, n_values, n_exps, num_io)) return rc;
  if (int rc = walk_nodes(nodes, maps, kind == SBN_AIR_FQ_EXP, count, n_values, n_exps, false, nullptr, nullptr)) return rc;
  if (!public_inputs) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (units != sbn_msm_num_units(count, num_io))
    return fail(SBN_ERR_VERIFY_FAILED, "%zu units given, a program of %zu nodes in tables of %zu has %zu units", units, count, num_io, sbn_msm_num_units(count, num_io));
  const UnitInputs U((int)kind, num_io, public_inputs, units);
  if (int rc = U.null_unit()) return rc;
  const PiLayout& L = U.L;
  const uint32_t one[96] = {1};
  std::vector<uint32_t> out(L.xw);
  return check_program_links(U, nodes, count, values, exps,
    [&](uint32_t op, const char** what) -> const uint32_t* { *what = "is not one"; return op == SBN_NODE_ONE ? one : nullptr; },
    [&](size_t g) {   // a limb wider than its slot, or a coefficient >= p, is no output of the table
      size_t limb;
      if (!U.output(g, out.data(), &limb)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output limb %zu is out of range", g, limb);
      if (!below_p(out.data(), L.values())) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output has a coefficient >= p", g);
      if (outs_out) memcpy(outs_out + L.xw * g, out.data(), L.xw * sizeof(uint32_t));
      return (int)SBN_OK;
    }, maps);
}
extern "C" int sbn_program_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units,
                                 const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values,
                                 const uint32_t* exps, size_t n_exps, uint32_t* outs_out) {
  return program_check(kind, num_io, public_inputs, units, nodes, nullptr, count, values, n_values, exps, n_exps, outs_out);
}
extern "C" int sbn_program_m_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units,
                                   const sbn_program_node_m* nodes, size_t count, const uint32_t* values, size_t n_values,
                                   const uint32_t* exps, size_t n_exps, uint32_t* outs_out) {
  std::vector<sbn_program_node> plain; std::vector<uint32_t> maps;
  const sbn_program_node* twin = split_or_pass(nodes, count, plain, maps);
  return program_check(kind, num_io, public_inputs, units, twin, maps.data(), count, values, n_values, exps, n_exps, outs_out);
}

// ---- the two host helpers of the mapped links ---------------------------------------------------------------------------------------
extern "C" int sbn_fq12_frobenius(const uint32_t in[96], uint32_t m, uint32_t out[96]) {
  if (!in || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (m > 11) return fail(SBN_ERR_BAD_ARG, "a Frobenius map is 0 .. 11, got %u", m);
  if (!below_p(in, 12)) return fail(SBN_ERR_BAD_ARG, "coefficient >= p");
  fq12_frobenius_words(in, m, out);
  return SBN_OK;
}
// f^-1 = fbar / (f fbar), fbar = frob(f, 1) ... frob(f, 11): f fbar is the norm of f, an element of Fq, non-zero unless f is
extern "C" int sbn_fq12_inverse(const uint32_t in[96], uint32_t out[96]) {
  if (!in || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (!below_p(in, 12)) return fail(SBN_ERR_BAD_ARG, "coefficient >= p");
  Fq f[12], fbar[12], t[12];
  field_load<12>(in, f);
  bool zero = true;
  for (int c = 0; c < 12; c++) zero = zero && fzero(f[c]);
  if (zero) return fail(SBN_ERR_BAD_ARG, "zero has no inverse");
  fq12_frobenius_m(f, 1, fbar);
  for (unsigned m = 2; m < 12; m++) { fq12_frobenius_m(f, m, t); field_mul<12>(fbar, t, fbar); }
  field_mul<12>(f, fbar, t);   // the norm: t[0], every other coefficient zero
  const Fq ni = fq_inv_m(t[0]);
  for (int c = 0; c < 12; c++) fbar[c] = mmul(fbar[c], ni);
  field_store<12>(fbar, out);
  return SBN_OK;
}
