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
#include "instance_lists.hpp"

using namespace sbn;

namespace {
using namespace bnw;
using namespace sbn::curve_host;

// the `count` towers of `depth` levels: rows [0, count * depth) of ios (optional) and powers (optional, [count][depth][8N])
template <int N>
void towers(const PiLayout& t, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count, size_t depth, uint32_t* ios, uint32_t* powers) {
  const size_t W = t.xw, ew = t.ew, IOW = t.IOW();
  host_parallel_for(count, [&](size_t k) {
    const uint32_t* e = exps + (exp_count == 1 ? 0 : ew * k);
    Fq x[N];
    field_load<N>(bases + W * k, x);
    for (size_t l = 0; l < depth; l++) {
      const size_t g = k * depth + l;
      if (ios) {
        uint32_t* io = ios + IOW * g;
        field_store<N>(x, io);
        memset(io + W, 0, W * sizeof(uint32_t)); io[W] = 1;
        memcpy(io + 2 * W, e, ew * sizeof(uint32_t));
      }
      field_power<N>(x, e, (int)(32 * ew), x);
      if (powers) field_store<N>(x, powers + W * g);
    }
  });
}

// kind, then the arguments every entry point shares, in the order of the header's refusals
int check_args(int32_t kind, const void* bases, const void* exps, size_t exp_count, size_t count, size_t depth, size_t num_io) {
  if (!pi_layout((int)kind).field()) return fail(SBN_ERR_UNSUPPORTED, "field powers cover the field tables FQ_EXP, FQ12_EXP and FQ12_EXP_U64 (a curve table takes sbn_scalar_mul_instances)");
  if (!bases || !exps || count == 0 || depth == 0 || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no tower, depth = 0 or num_io = 0");
  if (exp_count != 1 && exp_count != count) return fail(SBN_ERR_BAD_ARG, "exp_count must be 1 (one shared exponent) or count = %zu, got %zu", count, exp_count);
  if (depth > (size_t)-1 / 2 / count) return fail(SBN_ERR_BAD_ARG, "count * depth does not fit");
  return SBN_OK;
}
}  // namespace

namespace sbn {
int power_check_inputs(int kind, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count) {
  const PiLayout t = pi_layout(kind);
  const size_t W = t.xw;
  for (size_t k = 0; k < count; k++) {
    if (!below_p(bases + W * k, t.values())) return fail(SBN_ERR_BAD_ARG, "%s >= p (tower %zu)", W == 8 ? "value" : "coefficient", k);
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
  const PiLayout t = pi_layout((int)kind);
  const size_t M = count * depth;
  if (t.values() == 1) towers<1>(t, bases, exps, exp_count, count, depth, ios_out, powers_out);
  else towers<12>(t, bases, exps, exp_count, count, depth, ios_out, powers_out);
  if (ios_out) pad_rows(ios_out, t.IOW(), M, sbn_msm_num_units(M, num_io) * num_io);
  return SBN_OK;
}

extern "C" int sbn_power_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, size_t depth,
                               const uint32_t* bases, const uint32_t* exps, size_t exp_count, uint32_t* powers_out) {
  if (int rc = check_args(kind, bases, exps, exp_count, count, depth, num_io)) return rc;
  if (!public_inputs) return fail(SBN_ERR_BAD_ARG, "null argument");
  const size_t M = count * depth;
  if (units != sbn_msm_num_units(M, num_io))
    return fail(SBN_ERR_VERIFY_FAILED, "%zu units given, %zu towers of depth %zu in tables of %zu have %zu units", units, count, depth, num_io, sbn_msm_num_units(M, num_io));
  const UnitInputs U((int)kind, num_io, public_inputs, units);
  if (int rc = U.null_unit()) return rc;
  const PiLayout& L = U.L;
  const uint32_t one[96] = {1};
  std::vector<uint32_t> out(L.xw);
  for (size_t g = 0; g < U.rows(); g++) {
    if (g >= M) { if (int rc = U.pad(g, M - 1)) return rc; continue; }
    const size_t k = g / depth, l = g % depth;
    if (!U.value_is(g, U.oOff, one)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level %zu): offset is not one", g, k, l);
    if (!U.exp_is(g, exps + (exp_count == 1 ? 0 : L.ew * k))) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level %zu): exponent differs from the caller's", g, k, l);
    if (l == 0) {
      if (!U.value_is(g, U.oX, bases + L.xw * k)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level 0): x differs from the caller's base", g, k);
    } else if (!same(U.inst(g) + U.oX, U.inst(g - 1) + U.oOut, L.W))
      return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level %zu): x differs from the output of instance %zu", g, k, l, g - 1);
    // a limb wider than its slot, or a coefficient >= p, is no output of the table
    size_t limb;
    if (!U.output(g, out.data(), &limb)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level %zu): output limb %zu is out of range", g, k, l, limb);
    if (!below_p(out.data(), L.values())) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (tower %zu, level %zu): output has a coefficient >= p", g, k, l);
    if (powers_out) memcpy(powers_out + L.xw * g, out.data(), L.xw * sizeof(uint32_t));
  }
  return SBN_OK;
}
