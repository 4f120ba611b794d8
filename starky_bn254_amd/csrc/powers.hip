// Field powers and power towers (include/sbn.h, "Field powers"): the application call shape of the three field Exp tables
// FqExpStark, Fq12ExpStark and Fq12ExpU64Stark.  A field table needs no trick with its offset (one is always legal), so an
// independent power x^e is an instance with offset = 1; what no list of independent or offset-chained instances can say is a TOWER,
// where the x of level l is the OUTPUT of level l - 1: f^x, f^(x^2), f^(x^3) for the BN parameter x, the three powers the hard part
// of the final exponentiation starts from (the reason Fq12ExpU64Stark exists: src/fields/fq12_u64/exp_u64.rs).  Here
//  * sbn_power_instances builds the explicit, padded, unit-cut list and the powers on the host pool: towers side by side, the
//    levels of a tower one after the other, the square-and-multiply of the table itself (a = x, b = 1; bit t set: b = a b; a = a a);
//  * sbn_power_check reads the public inputs of the unit proofs and states the links a circuit would `connect`: offsets are one,
//    exponents are the caller's, level 0 starts from the caller's base, level l from the output of level l - 1 (across unit
//    boundaries), pads repeat the last instance, outputs are field elements.  It verifies no proof.
// Host code only: no kernel is launched from this unit (tracegen_device.hip holds the device form of the tower).
#include "curve_host.hpp"
#include <cstring>

using namespace sbn;

namespace {
using namespace bnw;
using namespace sbn::curve_host;

// x^e by the table's walk, N Montgomery coefficients (1: Fq, 12: Fq12 in the flat basis), `bits` exponent bits, least significant first
template <int N> void power_m(const Fq* x, const uint32_t* e, int bits, Fq* out) {
  Fq a[N], b[N], prod[N];
  for (int c = 0; c < N; c++) { a[c] = x[c]; b[c] = Fq{{0, 0, 0, 0}}; }
  b[0] = fq_one();
  for (int t = 0; t < bits; t++) {
    const bool bit = (e[t >> 5] >> (t & 31)) & 1;
    if (N == 1) { if (bit) b[0] = mmul(a[0], b[0]); a[0] = mmul(a[0], a[0]); continue; }
    if (bit) { fq12_mul_m(a, b, prod); memcpy(b, prod, sizeof b); }
    fq12_mul_m(a, a, prod); memcpy(a, prod, sizeof a);
  }
  memcpy(out, b, sizeof b);
}

// the `count` towers of `depth` levels: rows [0, count * depth) of ios (optional) and powers (optional, [count][depth][8N])
template <int N>
void towers(const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count, size_t depth, size_t ew, uint32_t* ios, uint32_t* powers) {
  const size_t W = 8 * N, IOW = 2 * W + ew;
  host_parallel_for(count, [&](size_t k) {
    const uint32_t* e = exps + (exp_count == 1 ? 0 : ew * k);
    Fq x[N], out[N];
    for (int c = 0; c < N; c++) { u64 t4[4]; ld_u32(bases + W * k + 8 * c, t4); x[c] = to_m(t4); }
    for (size_t l = 0; l < depth; l++) {
      const size_t g = k * depth + l;
      if (ios) {
        uint32_t* io = ios + IOW * g;
        for (int c = 0; c < N; c++) st_u32(x[c], io + 8 * c);
        memset(io + W, 0, W * sizeof(uint32_t)); io[W] = 1;
        memcpy(io + 2 * W, e, ew * sizeof(uint32_t));
      }
      power_m<N>(x, e, (int)(32 * ew), out);
      if (powers) for (int c = 0; c < N; c++) st_u32(out[c], powers + W * g + 8 * c);
      memcpy(x, out, sizeof x);
    }
  });
}

// (the public inputs of one instance: PiLayout, host_common.hpp)
bool same(const uint64_t* a, const uint64_t* b, size_t n) { return memcmp(a, b, n * sizeof(uint64_t)) == 0; }

// kind, then the arguments every entry point shares, in the order of the header's refusals
int check_args(int32_t kind, const void* bases, const void* exps, size_t exp_count, size_t count, size_t depth, size_t num_io) {
  if (!power_elem_words((int)kind)) return fail(SBN_ERR_UNSUPPORTED, "field powers cover the field tables FQ_EXP, FQ12_EXP and FQ12_EXP_U64 (a curve table takes sbn_scalar_mul_instances)");
  if (!bases || !exps || count == 0 || depth == 0 || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no tower, depth = 0 or num_io = 0");
  if (exp_count != 1 && exp_count != count) return fail(SBN_ERR_BAD_ARG, "exp_count must be 1 (one shared exponent) or count = %zu, got %zu", count, exp_count);
  if (depth > (size_t)-1 / 2 / count) return fail(SBN_ERR_BAD_ARG, "count * depth does not fit");
  return SBN_OK;
}
}  // namespace

namespace sbn {
size_t power_elem_words(int kind) { return kind == SBN_AIR_FQ_EXP ? 8 : (kind == SBN_AIR_FQ12_EXP || kind == SBN_AIR_FQ12_EXP_U64 ? 96 : 0); }

int power_check_inputs(int kind, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count) {
  const size_t W = power_elem_words(kind);
  for (size_t k = 0; k < count; k++) {
    if (!below_p(bases + W * k, (int)(W / 8))) return fail(SBN_ERR_BAD_ARG, "%s >= p (tower %zu)", W == 8 ? "value" : "coefficient", k);
    if (kind == SBN_AIR_FQ12_EXP_U64 && k < exp_count && ((u64)exps[2 * k] | ((u64)exps[2 * k + 1] << 32)) >= GLP)
      return fail(SBN_ERR_NON_CANONICAL, "exponent of tower %zu is not a canonical field element", k);
  }
  return SBN_OK;
}
}  // namespace sbn

extern "C" int sbn_bn_x(uint32_t out[2]) {
  if (!out) return fail(SBN_ERR_BAD_ARG, "null argument");
  out[0] = 0x4A6909F1u; out[1] = 0x44E992B4u;   // 4965661367192848881
  return SBN_OK;
}

extern "C" int sbn_power_instances(int32_t kind, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count, size_t depth, size_t num_io,
                                   uint32_t* ios_out, uint32_t* powers_out) {
  if (int rc = check_args(kind, bases, exps, exp_count, count, depth, num_io)) return rc;
  if (int rc = power_check_inputs((int)kind, bases, exps, exp_count, count)) return rc;
  const size_t ew = kind == SBN_AIR_FQ12_EXP_U64 ? 2 : 8, IOW = exp_io_words((int)kind), M = count * depth;
  if (kind == SBN_AIR_FQ_EXP) towers<1>(bases, exps, exp_count, count, depth, ew, ios_out, powers_out);
  else towers<12>(bases, exps, exp_count, count, depth, ew, ios_out, powers_out);
  // the reference's resize rule (src/curves/g1/circuit.rs:273-277): a pad row is the last row again
  if (ios_out) for (size_t g = M; g < sbn_msm_num_units(M, num_io) * num_io; g++) memcpy(ios_out + IOW * g, ios_out + IOW * (M - 1), IOW * sizeof(uint32_t));
  return SBN_OK;
}

extern "C" int sbn_power_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, size_t depth,
                               const uint32_t* bases, const uint32_t* exps, size_t exp_count, uint32_t* powers_out) {
  if (int rc = check_args(kind, bases, exps, exp_count, count, depth, num_io)) return rc;
  if (!public_inputs) return fail(SBN_ERR_BAD_ARG, "null argument");
  const PiLayout L = pi_layout((int)kind);
  const size_t W = power_elem_words((int)kind), ew = L.EW == 1 ? 2 : 8, M = count * depth, per = L.per();
  if (units != sbn_msm_num_units(M, num_io))
    return fail(SBN_ERR_VERIFY_FAILED, "%zu units given, %zu towers of depth %zu in tables of %zu have %zu units", units, count, depth, num_io, sbn_msm_num_units(M, num_io));
  for (size_t u = 0; u < units; u++) if (!public_inputs[u]) return fail(SBN_ERR_BAD_ARG, "null public inputs (unit %zu)", u);
  auto inst = [&](size_t g) { return public_inputs[g / num_io] + per * (g % num_io); };
  const size_t oX = 0, oOff = L.W, oExp = 2 * L.W, oOut = 2 * L.W + L.EW;
  const uint64_t lim = L.limb16 ? 0xffffULL : 0xffffffffULL;
  const uint64_t* last = inst(M - 1);
  std::vector<uint64_t> want(L.W);
  std::vector<uint32_t> out(W);
  for (size_t g = 0; g < units * num_io; g++) {
    const uint64_t* p = inst(g);
    if (g >= M) {   // a pad instance is instance M - 1 again
      static const char* const field[4] = {"x", "offset", "exponent", "output"};
      const size_t at[4] = {oX, oOff, oExp, oOut}, len[4] = {L.W, L.W, L.EW, L.W};
      for (int f = 0; f < 4; f++)
        if (!same(p + at[f], last + at[f], len[f])) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (pad): %s differs from instance %zu", g, field[f], M - 1);
      continue;
    }
    const size_t k = g / depth, l = g % depth;
    for (size_t i = 0; i < L.W; i++)
      if (p[oOff + i] != (i == 0 ? 1u : 0u)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level %zu): offset is not one", g, k, l);
    const uint32_t* e = exps + (exp_count == 1 ? 0 : ew * k);
    uint64_t ep[8];
    exp_to_pi(L, e, ep);
    if (!same(p + oExp, ep, L.EW)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level %zu): exponent differs from the caller's", g, k, l);
    if (l == 0) {
      value_to_pi(L, bases + W * k, want.data());
      if (!same(p + oX, want.data(), L.W)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level 0): x differs from the caller's base", g, k);
    } else if (!same(p + oX, inst(g - 1) + oOut, L.W))
      return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level %zu): x differs from the output of instance %zu", g, k, l, g - 1);
    // a limb wider than its slot, or a coefficient >= p, is no output of the table
    for (size_t i = 0; i < L.W; i++)
      if (p[oOut + i] > lim) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level %zu): output limb %zu is out of range", g, k, l, i);
    if (!L.limb16) for (size_t i = 0; i < W; i++) out[i] = (uint32_t)p[oOut + i];
    else for (size_t i = 0; i < W; i++) out[i] = (uint32_t)(p[oOut + 2 * i] | (p[oOut + 2 * i + 1] << 16));
    if (!below_p(out.data(), (int)(W / 8))) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level %zu): output has a coefficient >= p", g, k, l);
    if (powers_out) memcpy(powers_out + W * g, out.data(), W * sizeof(uint32_t));
  }
  return SBN_OK;
}
