// Independent batches of scalar multiplications (include/sbn.h, "Scalar multiplications"): every instance of a G1ExpStark /
// G2ExpStark list carries the SAME offset and the caller wants e_k x_k itself, the call shape of the reference's
// g2_mul_by_cofactor_circuit (src/curves/g2/circuit.rs:335-367: x = point, offset = the G2 generator, exp_val = 2p - r, result =
// output + (-generator)) and of its G1ExpOutputGenerator / G2ExpOutputGenerator on independent inputs (src/curves/g1/circuit.rs:111-123).
// The offset exists only because the table cannot hold the point at infinity; here
//  * sbn_scalar_mul_instances builds the explicit, padded, unit-cut list and the products e_k x_k on the host pool (Jacobian, the
//    COMPLETE addition of bn254w.cuh, one shared inversion), then checks the table's own walk of that list and names the first
//    instance it cannot walk;
//  * sbn_scalar_mul_check reads the public inputs of the unit proofs and states what the reference states inside its circuit: the
//    x, exponents and offset are the caller's, the pads repeat the last instance, and product = output + (-offset) by the complete
//    addition (output = offset gives the point at infinity: not an error).  It verifies no proof.
// Host code only: no kernel is launched from this unit (tracegen_device.hip holds the device form of the list and the un-offset).
#include "instance_lists.hpp"

using namespace sbn;

namespace {
using namespace bnw;
using namespace sbn::curve_host;

// (1, 2) on G1; ark_bn254's G2Affine::generator() on the twist: x.c0 x.c1 y.c0 y.c1, eight little-endian u32 limbs each
const uint32_t G1_GEN[16] = {1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0};
const uint32_t G2_GEN[32] = {
    0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu,
    0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u,
    0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u,
    0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u};
// 2p - r: the twist's group has order r (2p - r)
const uint32_t G2_COFACTOR[8] = {0xc0f9fa8du, 0x345f2299u, 0x572a2489u, 0x06ceecdau, 0x8181585eu, 0xb85045b6u, 0xe131a029u, 0x30644e72u};

// the first of K instances the table cannot walk, as the scalar-multiplication calls word it
int degenerate_at(size_t k) {
  return fail(SBN_ERR_WITNESS, "instance %zu: degenerate affine operation in the table's walk (B[t] = +-2^t x at a set bit, or an output at infinity): pick another offset", k);
}

template <int E>
int instances(const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t count, size_t num_io, const uint32_t* offset,
              uint32_t* ios_out, uint32_t* products_out, uint8_t* infinity_out) {
  const PiLayout t = curve_layout(E);
  const size_t total = sbn_msm_num_units(count, num_io) * num_io;
  if (int rc = check_curve_points<E>(points, t.xw, count, offset, "offset")) return rc;
  std::vector<uint32_t> own;
  uint32_t* ios = ios_out;
  if (!ios) { own.resize(t.IOW() * total); ios = own.data(); }
  scalar_mul_explicit_list(E, points, scalars, scalar_count, count, total, offset, ios);
  if (products_out || infinity_out) {
    std::vector<Jac<E>> term(count);
    host_parallel_for(count, [&](size_t k) { term[k] = scalar_mul_jac<E>(ld_point<E>(points + t.xw * k), scalars + (scalar_count == 1 ? 0 : t.ew * k)); });
    affine_or_infinity<E>(term, products_out, infinity_out);
  }
  const size_t bad = walk_curve_list<E>(ios, count);   // the real instances: the pads repeat the last one
  if (bad == WALKS) return SBN_OK;
  return bad == UNNAMED ? fail(SBN_ERR_WITNESS, UNNAMED_WALK_TEXT) : degenerate_at(bad);
}

template <int E>
int check(size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, const uint32_t* points, const uint32_t* scalars,
          size_t scalar_count, const uint32_t* offset, uint32_t* products_out, uint8_t* infinity_out) {
  if (units != sbn_msm_num_units(count, num_io))
    return fail(SBN_ERR_VERIFY_FAILED, "%zu units given, a list of %zu instances in tables of %zu has %zu units", units, count, num_io, sbn_msm_num_units(count, num_io));
  const UnitInputs U(E == 1 ? SBN_AIR_G1_EXP : SBN_AIR_G2_EXP, num_io, public_inputs, units);
  if (int rc = U.null_unit()) return rc;
  const size_t W = U.L.xw;
  const Co<E> b = curve_b<E>();
  std::vector<uint32_t> outs(W * count);
  for (size_t g = 0; g < U.rows(); g++) {
    if (g >= count) { if (int rc = U.pad(g, count - 1)) return rc; continue; }
    if (!U.value_is(g, U.oX, points + W * g)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: x differs from the caller's point", g);
    if (!U.exp_is(g, scalars + (scalar_count == 1 ? 0 : U.L.ew * g))) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: exponent differs from the caller's scalar", g);
    if (!U.value_is(g, U.oOff, offset)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: offset differs from the offset of the call", g);
    uint32_t* o = outs.data() + W * g;
    size_t limb;
    if (!U.output(g, o, &limb)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output limb %zu is out of range", g, limb);
    if (!below_p(o, 2 * E)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output has a coordinate >= p", g);
    const Jac<E> q = ld_point<E>(o);
    if (!on_curve<E>(q.X, q.Y, b)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output is not a point of the curve", g);
  }
  if (products_out || infinity_out) scalar_mul_unoffset_host(E, outs.data(), offset, count, products_out, infinity_out);
  return SBN_OK;
}

// kind, then the arguments every entry point shares, in the order of the header's refusals
int check_args(int32_t kind, const void* points, const void* scalars, size_t scalar_count, size_t count, size_t num_io) {
  if (!pi_layout((int)kind).E) return fail(SBN_ERR_UNSUPPORTED, "scalar multiplications cover the curve tables G1_EXP and G2_EXP (a field table takes offset = 1 as it is)");
  if (!points || !scalars || count == 0 || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no instance or num_io = 0");
  if (scalar_count != 1 && scalar_count != count) return fail(SBN_ERR_BAD_ARG, "scalar_count must be 1 (one shared scalar) or count = %zu, got %zu", count, scalar_count);
  return SBN_OK;
}
}  // namespace

namespace sbn {
const uint32_t* curve_generator_words(int E) { return E == 1 ? G1_GEN : G2_GEN; }
const uint32_t* g2_cofactor_words() { return G2_COFACTOR; }

int scalar_mul_check_points(int E, const uint32_t* points, size_t count, const uint32_t* offset) {
  const size_t W = curve_layout(E).xw;
  return E == 1 ? check_curve_points<1>(points, W, count, offset, "offset") : check_curve_points<2>(points, W, count, offset, "offset");
}

void scalar_mul_explicit_list(int E, const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t count, size_t total,
                              const uint32_t* offset, uint32_t* ios) {
  const PiLayout t = curve_layout(E);
  const size_t W = t.xw, IOW = t.IOW();
  for (size_t g = 0; g < count; g++) {
    memcpy(ios + IOW * g, points + W * g, W * sizeof(uint32_t));
    memcpy(ios + IOW * g + W, offset, W * sizeof(uint32_t));
    memcpy(ios + IOW * g + 2 * W, scalars + (scalar_count == 1 ? 0 : t.ew * g), t.ew * sizeof(uint32_t));
  }
  pad_rows(ios, IOW, count, total);
}

int scalar_mul_name_degenerate(int E, const uint32_t* ios, size_t K) {
  const size_t bad = E == 1 ? first_unwalkable<1>(ios, K) : first_unwalkable<2>(ios, K);
  return bad == K ? SBN_OK : degenerate_at(bad);
}

template <int E> static void unoffset(const uint32_t* outputs, const uint32_t* offset, size_t K, uint32_t* products, uint8_t* infinity) {
  const Jac<E> noff = neg_point<E>(ld_point<E>(offset));
  const size_t W = curve_layout(E).xw;
  std::vector<Jac<E>> prod(K);
  for (size_t k = 0; k < K; k++) prod[k] = jac_add_complete<E>(ld_point<E>(outputs + W * k), noff);
  affine_or_infinity<E>(prod, products, infinity);
}
void scalar_mul_unoffset_host(int E, const uint32_t* outputs, const uint32_t* offset, size_t K, uint32_t* products, uint8_t* infinity) {
  if (E == 1) unoffset<1>(outputs, offset, K, products, infinity); else unoffset<2>(outputs, offset, K, products, infinity);
}
}  // namespace sbn

extern "C" int sbn_curve_generator(int32_t kind, uint32_t* out) {
  const int E = pi_layout((int)kind).E;
  if (!E) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not a curve table", (int)kind);
  if (!out) return fail(SBN_ERR_BAD_ARG, "null argument");
  memcpy(out, curve_generator_words(E), curve_layout(E).xw * sizeof(uint32_t));
  return SBN_OK;
}

extern "C" int sbn_g2_cofactor(uint32_t out[8]) {
  if (!out) return fail(SBN_ERR_BAD_ARG, "null argument");
  memcpy(out, G2_COFACTOR, sizeof G2_COFACTOR);
  return SBN_OK;
}

extern "C" int sbn_scalar_mul_instances(int32_t kind, const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t count, size_t num_io,
                                        const uint32_t* offset, uint32_t* ios_out, uint32_t* products_out, uint8_t* infinity_out) {
  if (int rc = check_args(kind, points, scalars, scalar_count, count, num_io)) return rc;
  const int E = pi_layout((int)kind).E;
  if (!offset) offset = curve_generator_words(E);
  return E == 1 ? instances<1>(points, scalars, scalar_count, count, num_io, offset, ios_out, products_out, infinity_out)
                : instances<2>(points, scalars, scalar_count, count, num_io, offset, ios_out, products_out, infinity_out);
}

extern "C" int sbn_scalar_mul_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, const uint32_t* points,
                                    const uint32_t* scalars, size_t scalar_count, const uint32_t* offset, uint32_t* products_out, uint8_t* infinity_out) {
  if (int rc = check_args(kind, points, scalars, scalar_count, count, num_io)) return rc;
  if (!public_inputs) return fail(SBN_ERR_BAD_ARG, "null argument");
  const int E = pi_layout((int)kind).E;
  if (!offset) offset = curve_generator_words(E);
  if (!below_p(offset, 2 * E)) return fail(SBN_ERR_BAD_ARG, "coordinate >= p (offset)");
  return E == 1 ? check<1>(num_io, public_inputs, units, count, points, scalars, scalar_count, offset, products_out, infinity_out)
                : check<2>(num_io, public_inputs, units, count, points, scalars, scalar_count, offset, products_out, infinity_out);
}

extern "C" int sbn_mul_by_cofactor_check(size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, const uint32_t* points,
                                         uint32_t* cleared_out, uint8_t* infinity_out) {
  return sbn_scalar_mul_check(SBN_AIR_G2_EXP, num_io, public_inputs, units, count, points, G2_COFACTOR, 1, nullptr, cleared_out, infinity_out);
}
