// What the five units that turn application inputs into an explicit `ios` list share (chain_instances.hip, msm.hip, scalar_mul.hip,
// powers.hip, msm_batch.hip): the search for the first offending instance on the host pool, the refusals of a curve list, the
// field tables' square-and-multiply, the pad rule, the table's own walk of an explicit curve list, the reader of the per-unit
// public inputs behind the *_check calls, and what the two program units (program.hip, curve_program.hip) share: the link words,
// the schedule of a levelled program and the link checks.  Host code only.  (The word counts of a table: PiLayout, host_common.hpp.)
#pragma once
#include "curve_host.hpp"
#include <vector>

namespace sbn {
namespace curve_host {

// the smallest index in [0, K) for which bad(k) holds, on the host pool; K when there is none
template <typename F> size_t first_bad(size_t K, F bad) {
  std::atomic<size_t> at(K);
  host_parallel_for(K, [&](size_t k) {
    if (k > at.load() || !bad(k)) return;
    size_t cur = at.load(); while (k < cur && !at.compare_exchange_weak(cur, k)) {}
  });
  return at.load();
}

// The refusals of a curve list: `start` (named `start_name` in the message) and the K points at pts + stride * k have coordinates
// below p and lie on the table's curve; the first offending instance is named.
template <int E> int check_curve_points(const uint32_t* pts, size_t stride, size_t K, const uint32_t* start, const char* start_name) {
  if (!below_p(start, 2 * E)) return fail(SBN_ERR_BAD_ARG, "coordinate >= p (%s)", start_name);
  for (size_t k = 0; k < K; k++) if (!below_p(pts + stride * k, 2 * E)) return fail(SBN_ERR_BAD_ARG, "coordinate >= p (instance %zu)", k);
  const Co<E> b = curve_b<E>();
  const Jac<E> s = ld_point<E>(start);
  if (!on_curve<E>(s.X, s.Y, b)) return fail(SBN_ERR_BAD_ARG, "%s is not a point of the curve", start_name);
  const size_t bad = first_bad(K, [&](size_t k) { const Jac<E> p = ld_point<E>(pts + stride * k); return !on_curve<E>(p.X, p.Y, b); });
  if (bad < K) return fail(SBN_ERR_BAD_ARG, "x of instance %zu is not a point of the curve", bad);
  return SBN_OK;
}

// N Montgomery coefficients of a field element: 1 in Fq, 12 in Fq12 (the flat basis of the field tables); out may be a or b
template <int N> void field_load(const uint32_t* w, Fq* out) { for (int c = 0; c < N; c++) { u64 t[4]; ld_u32(w + 8 * c, t); out[c] = to_m(t); } }
template <int N> void field_store(const Fq* v, uint32_t* w) { for (int c = 0; c < N; c++) st_u32(v[c], w + 8 * c); }
template <int N> void field_mul(const Fq* a, const Fq* b, Fq* out) {
  if (N == 1) { out[0] = mmul(a[0], b[0]); return; }
  Fq prod[12]; fq12_mul_m(a, b, prod); memcpy(out, prod, N * sizeof(Fq));
}
// x^e by the table's walk (a = x, b = 1; bit t set: b = a b; a = a a), `bits` exponent bits, least significant first
template <int N> void field_power(const Fq* x, const uint32_t* e, int bits, Fq* out) {
  Fq a[N], b[N];
  for (int c = 0; c < N; c++) { a[c] = x[c]; b[c] = Fq{{0, 0, 0, 0}}; }
  b[0] = fq_one();
  for (int t = 0; t < bits; t++) { if ((e[t >> 5] >> (t & 31)) & 1) field_mul<N>(a, b, b); field_mul<N>(a, a, a); }
  memcpy(out, b, sizeof b);
}

// The Frobenius maps of Fq12 in the flat basis (include/sbn.h, "Mapped links and the final exponentiation"): out = in^(p^m), m < 12.
// Coefficient k of w^k is a_k = c[k] + c[k+6] i; it becomes conj^m(a_k) * G[m][k], G[m][k] = (9 + i)^(k (p^m - 1) / 6) the table of
// tools/gen_fq12_frobenius.py.  Montgomery form in and out; out may be in.
inline void fq12_frobenius_m(const Fq* in, unsigned m, Fq* out) {
  static const u64 G[12][6][2][4] = {
#include "fq12_frobenius_consts.hpp"
  };
  for (int k = 0; k < 6; k++) {
    const Fq re = in[k], im = (m & 1) ? fsub(Fq{{0, 0, 0, 0}}, in[k + 6]) : in[k + 6];
    const Fq g0 = to_m(G[m][k][0]), g1 = to_m(G[m][k][1]);
    out[k] = fsub(mmul(re, g0), mmul(im, g1));
    out[k + 6] = fadd(mmul(re, g1), mmul(im, g0));
  }
}
// the same on the u32 words of an element (every coefficient < p)
inline void fq12_frobenius_words(const uint32_t* in, unsigned m, uint32_t* out) {
  Fq v[12];
  field_load<12>(in, v);
  fq12_frobenius_m(v, m, v);
  field_store<12>(v, out);
}

// rows [M, total) <- row M - 1: the reference's resize rule (src/curves/g1/circuit.rs:273-277), a pad row is the last row again
inline void pad_rows(uint32_t* ios, size_t IOW, size_t M, size_t total) {
  for (size_t g = M; g < total; g++) memcpy(ios + IOW * g, ios + IOW * (M - 1), IOW * sizeof(uint32_t));
}

inline bool same(const uint64_t* a, const uint64_t* b, size_t n) { return memcmp(a, b, n * sizeof(uint64_t)) == 0; }

// The table's own walk (g1/exp.rs:165-230) of the K instances of an explicit curve list, B[t] = +-A[t] at an addition refuses it.
// first_unwalkable: one instance at a time, the first one the table cannot walk (K: none).  walk_curve_list: with the chains the
// witness generators use (tracegen_host_chains), 512 instances per pass to bound the chain storage (49 KB E per instance); WALKS
// when the table walks them all, the first instance it cannot walk, or UNNAMED when a pass fails and no instance of it does.
static constexpr size_t WALKS = (size_t)-1, UNNAMED = (size_t)-2;
template <int E> size_t first_unwalkable(const uint32_t* ios, size_t K) {
  return first_bad(K, [&](size_t k) {
    std::vector<u64> ja(257 * 12 * E), jb(257 * 12 * E);
    return exp_chains<E>(ios + curve_layout(E).IOW() * k, 0, ja.data(), jb.data()) != 0;
  });
}
template <int E> size_t walk_curve_list(const uint32_t* ios, size_t K) {
  const size_t CH = 512, IOW = curve_layout(E).IOW();
  std::vector<u64> chains(2 * 257 * 12 * E * (K < CH ? K : CH));
  for (size_t at = 0; at < K; at += CH) {
    const size_t k = K - at < CH ? K - at : CH, cw = 257 * 12 * E * k;
    if (!tracegen_host_chains(E, ios + IOW * at, k, chains.data(), chains.data() + cw)) continue;
    const size_t bad = first_unwalkable<E>(ios + IOW * at, k);
    return bad == k ? UNNAMED : at + bad;
  }
  return WALKS;
}
// The per-instance form of that walk (the complete sums need every failing segment of a pass, not the first instance): bad[k] = 1
// where the table cannot walk instance k, 0 elsewhere; false when a pass fails and no instance of it does (walk_curve_list's UNNAMED).
template <int E> bool walk_status(const uint32_t* ios, size_t K, uint8_t* bad) {
  const size_t CH = 512, IOW = curve_layout(E).IOW();
  std::vector<u64> chains(2 * 257 * 12 * E * (K < CH ? K : CH));
  memset(bad, 0, K);
  for (size_t at = 0; at < K; at += CH) {
    const size_t k = K - at < CH ? K - at : CH, cw = 257 * 12 * E * k;
    if (!tracegen_host_chains(E, ios + IOW * at, k, chains.data(), chains.data() + cw)) continue;
    std::atomic<size_t> found(0);
    host_parallel_for(k, [&](size_t i) {
      std::vector<u64> ja(257 * 12 * E), jb(257 * 12 * E);
      if (exp_chains<E>(ios + IOW * (at + i), 0, ja.data(), jb.data()) != 0) { bad[at + i] = 1; found++; }
    });
    if (!found.load()) return false;
  }
  return true;
}
static constexpr const char* UNNAMED_WALK_TEXT = "degenerate affine operation (x1 == x2 or y == 0)";

// The public inputs of the unit proofs of one list, as the link checks read them: instance g is row g % num_io of unit g / num_io.
struct UnitInputs {
  const PiLayout L;
  const size_t num_io, units, oX, oOff, oExp, oOut;   // the four values of an instance start at these public inputs
  const uint64_t* const* const pi;
  UnitInputs(int kind, size_t num_io, const uint64_t* const* public_inputs, size_t units)
      : L(pi_layout(kind)), num_io(num_io), units(units), oX(0), oOff(L.W), oExp(2 * L.W), oOut(2 * L.W + L.EW), pi(public_inputs) {}
  size_t rows() const { return units * num_io; }
  int null_unit() const {
    for (size_t u = 0; u < units; u++) if (!pi[u]) return fail(SBN_ERR_BAD_ARG, "null public inputs (unit %zu)", u);
    return SBN_OK;
  }
  const uint64_t* inst(size_t g) const { return pi[g / num_io] + L.per() * (g % num_io); }
  // a pad instance g is instance `last` again
  int pad(size_t g, size_t last) const {
    static const char* const field[4] = {"x", "offset", "exponent", "output"};
    const size_t at[4] = {oX, oOff, oExp, oOut}, len[4] = {L.W, L.W, L.EW, L.W};
    for (int f = 0; f < 4; f++)
      if (!same(inst(g) + at[f], inst(last) + at[f], len[f])) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (pad): %s differs from instance %zu", g, field[f], last);
    return SBN_OK;
  }
  // the value at oX / oOff, and the exponent, of instance g are the caller's u32 words
  bool value_is(size_t g, size_t at, const uint32_t* w) const { std::vector<uint64_t> want(L.W); value_to_pi(L, w, want.data()); return same(inst(g) + at, want.data(), L.W); }
  bool exp_is(size_t g, const uint32_t* w) const { uint64_t e[8]; exp_to_pi(L, w, e); return same(inst(g) + oExp, e, L.EW); }
  // the output of instance g as the L.xw u32 words of a value; false and *limb = the first limb wider than its slot: no output of the table
  bool output(size_t g, uint32_t* w, size_t* limb) const { return value_from_pi(L, inst(g) + oOut, w, limb); }
};

// ---- programs (program.hip, curve_program.hip, and their device drivers in tracegen_device.hip) ------------------------------------
inline bool linked(uint32_t v) { return (v & SBN_NODE_OUTPUT) != 0; }
inline uint32_t link_of(uint32_t v) { return v & ~SBN_NODE_OUTPUT; }
// mapped programs: maps[g] = the map of x (bits 0..7) | the map of offset << 8 of node g; a null table is all zeros
inline unsigned map_of(const uint32_t* maps, size_t g, int f) { return maps ? (maps[g] >> (8 * f)) & 0xffu : 0u; }
// the unmapped twin of a mapped node table, and its maps
inline void split_nodes(const sbn_program_node_m* nodes, size_t count, std::vector<sbn_program_node>& plain, std::vector<uint32_t>& maps) {
  plain.resize(count); maps.resize(count);
  for (size_t g = 0; g < count; g++) { plain[g] = sbn_program_node{nodes[g].x, nodes[g].offset, nodes[g].exp}; maps[g] = nodes[g].maps; }
}

// The schedule from level[count] (sbn_program_levels): a stable counting sort, so plan.order lists the nodes of level l in node
// order at [level_start[l], level_start[l + 1]).  rows > count: rows [count, rows) are pads, scheduled as further nodes of the level
// of node count - 1 (the device walks a pad of a curve program as one more node).  plan.level is the caller's.
inline void fill_plan(const uint32_t* level, size_t count, size_t rows, ProgramPlan& plan) {
  const auto at = [&](size_t g) { return level[g < count ? g : count - 1]; };
  uint32_t depth = 0;
  for (size_t g = 0; g < count; g++) if (level[g] + 1 > depth) depth = level[g] + 1;
  plan.level_start.assign((size_t)depth + 1, 0);
  for (size_t g = 0; g < rows; g++) plan.level_start[at(g) + 1]++;
  for (size_t l = 0; l < depth; l++) plan.level_start[l + 1] += plan.level_start[l];
  plan.order.resize(rows);
  std::vector<uint32_t> next(plan.level_start.begin(), plan.level_start.end() - 1);
  for (size_t g = 0; g < rows; g++) plan.order[next[at(g)]++] = (uint32_t)g;
}

// The link checks behind sbn_program_check and sbn_curve_program_check, in instance order: a pad is instance count - 1 again; x and
// offset equal the output of the node they link to, or the words of their literal in `literals`, or what sentinel(op, what) returns
// for an operand that is neither (one, the start; null: op is a literal index), `what` the tail of its refusal; the exponent is the
// caller's; judge_output(g) has the last word on the output of instance g.  maps (optional, field programs on Fq12): a linked
// operand with map m equals frob(output of node j, m), computed here from the OUTPUT public inputs of node j (instance order:
// judge_output(j) has accepted them).
template <typename Sentinel, typename Judge>
int check_program_links(const UnitInputs& U, const sbn_program_node* nodes, size_t count, const uint32_t* literals, const uint32_t* exps, Sentinel sentinel,
                        Judge judge_output, const uint32_t* maps = nullptr) {
  const PiLayout& L = U.L;
  std::vector<uint32_t> mapped(maps ? L.xw : 0);
  for (size_t g = 0; g < U.rows(); g++) {
    if (g >= count) { if (int rc = U.pad(g, count - 1)) return rc; continue; }
    const uint32_t op[2] = {nodes[g].x, nodes[g].offset};
    const size_t at[2] = {U.oX, U.oOff};
    static const char* const field[2] = {"x", "offset"};
    for (int f = 0; f < 2; f++) {
      const char* what = nullptr;
      if (const unsigned m = linked(op[f]) ? map_of(maps, g, f) : 0u) {
        size_t limb;
        if (!U.output(link_of(op[f]), mapped.data(), &limb))
          return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: %s is frob_%u of the output of node %u, whose limb %zu is out of range", g, field[f], m, link_of(op[f]), limb);
        fq12_frobenius_words(mapped.data(), m, mapped.data());
        if (!U.value_is(g, at[f], mapped.data()))
          return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: %s differs from frob_%u of the output of node %u", g, field[f], m, link_of(op[f]));
      } else if (linked(op[f])) {
        if (!same(U.inst(g) + at[f], U.inst(link_of(op[f])) + U.oOut, L.W))
          return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: %s differs from the output of node %u", g, field[f], link_of(op[f]));
      } else if (const uint32_t* w = sentinel(op[f], &what)) {
        if (!U.value_is(g, at[f], w)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: %s %s", g, field[f], what);
      } else if (!U.value_is(g, at[f], literals + L.xw * op[f]))
        return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: %s differs from the caller's literal %u", g, field[f], op[f]);
    }
    if (!U.exp_is(g, exps + L.ew * nodes[g].exp)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: exponent differs from the caller's", g);
    if (int rc = judge_output(g)) return rc;
  }
  return SBN_OK;
}

}  // namespace curve_host
}  // namespace sbn
