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
// The start candidates of the complete sums (include/sbn.h, "Complete sums"): fixed points with no chosen relation to the generator.
// G1: x = 2, 3, 4, ... kept where x^3 + 3 is a non-zero square, y the smaller root as an integer, the first eight (x = 2, 3, 5, 6, 7,
// 8, 9, 11).  Twist: x = k + i for k = 0, 1, 2, ... kept where x^3 + 3 / (9 + i) is a non-zero square in Fq2, y the root whose (c1, c0)
// pair is smaller, the first eight (k = 0, 2, 3, 4, 5, 6, 8, 11); they need not lie in the order-r subgroup.
const uint32_t G1_STARTS[SBN_START_CANDIDATES][16] = {
    {0x00000002u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x8dac7f34u, 0xc4ef4e70u, 0xf61fcb49u, 0x517130cfu, 0xbe095d60u, 0x6451ec04u, 0xb8625180u, 0x0ce2c194u},
    {0x00000003u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x790bf1d8u, 0x3f5722eau, 0x733cbefbu, 0xb34856a8u, 0xde6c4e5du, 0xcb2a2c72u, 0xc6aa8196u, 0x0dd9a1d6u},
    {0x00000005u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x8c3822f9u, 0x3bb0834du, 0x060d96d8u, 0x8064aa6bu, 0x4225fad9u, 0x0f34b3dau, 0x1c3443f8u, 0x15d246fdu},
    {0x00000006u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0xc068fd16u, 0x7a654e27u, 0xaff154acu, 0x37a3ab23u, 0x66b6646au, 0xddebc44eu, 0xfa785fc1u, 0x0d400b11u},
    {0x00000007u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x1789524cu, 0xa937d3c6u, 0x81f132e7u, 0x425669a1u, 0x10bde5bdu, 0x3515c724u, 0xdf2adcc3u, 0x157d4cebu},
    {0x00000008u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x42ab6e6au, 0xb0f62f2cu, 0xd1d5fec4u, 0xf4ac9fa8u, 0x0c6fd767u, 0x302e1de4u, 0x6a501a90u, 0x171538bdu},
    {0x00000009u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x14dbd3c5u, 0xccee22f3u, 0x13875d5fu, 0x9f6c1006u, 0x20fcf9f0u, 0x1d46b25fu, 0x02b8107du, 0x0769fc14u},
    {0x0000000bu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x7cd1f866u, 0xa48f47e4u, 0x0c8dafe6u, 0xcb98c83bu, 0x71f3f495u, 0xd5f1f745u, 0x9bd1db89u, 0x094263b9u},
};
const uint32_t G2_STARTS[SBN_START_CANDIDATES][32] = {
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x7f596ea8u, 0x60573e3au, 0x6e6321eeu, 0xc299b621u, 0x3201e68du, 0x092f24ecu, 0x49a2cb8au, 0x0cf32d3cu,
     0x3566c0e2u, 0x0b839c7fu, 0x2d4ab9ebu, 0xf9163695u, 0xcbffe3deu, 0xee60335au, 0x753ef8cbu, 0x07bca656u},
    {0x00000002u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0xd23bfb79u, 0x4bc97597u, 0x969ba779u, 0x5f621d6au, 0x53b27798u, 0x67b65916u, 0x9f9e9770u, 0x2044dbfau,
     0x57ed9d69u, 0xe307d561u, 0x71ca132fu, 0x2001ee7du, 0x2d175803u, 0x22129931u, 0x8795e6ffu, 0x04ed8cf9u},
    {0x00000003u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x43fa5543u, 0x512dc357u, 0x0c1600e4u, 0xb87f54f5u, 0x8e89515cu, 0x0b87aca7u, 0xa822ced6u, 0x18317863u,
     0x9ab5ab0cu, 0xd7132ea3u, 0x5fd5bf84u, 0x1e41899eu, 0xb391072cu, 0x4eb9190bu, 0xff7c6a39u, 0x16f36623u},
    {0x00000004u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x8979c2dbu, 0x068fb190u, 0x8569107eu, 0xe65faf58u, 0x83f9e3edu, 0x21689e16u, 0x28f073a9u, 0x09ca3404u,
     0x2a1a0e09u, 0x78b25b54u, 0x452da729u, 0x7e66ede6u, 0x9179b40bu, 0x3194dd31u, 0xa3a5c56bu, 0x0591853au},
    {0x00000005u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x7204b807u, 0xa6b869e4u, 0x82494357u, 0x7e0b18d7u, 0x9524877bu, 0x4e506ccbu, 0x6522aae6u, 0x2d4739e1u,
     0x383b1edcu, 0x0a0ba772u, 0x35e9ffafu, 0xe9488183u, 0x4f7529e1u, 0x15fb5184u, 0x24643defu, 0x0cec0985u},
    {0x00000006u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0xf94b0abfu, 0x7e877024u, 0xddf64b7cu, 0x58099451u, 0xce53e57eu, 0x492532b8u, 0x143955d5u, 0x278e4cf2u,
     0x998695c7u, 0x71a5dbd2u, 0xcf1535fau, 0xafcd72b2u, 0xad040da0u, 0xc91a719du, 0x46ef250eu, 0x07601faau},
    {0x00000008u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x9a2bdf1eu, 0x7457c685u, 0x327ddfb8u, 0x62e8be9eu, 0x7d654c9cu, 0x44c15b0du, 0xbf6571d7u, 0x19cfafe8u,
     0xafa9fd9fu, 0x46b9f17bu, 0x5e9dba86u, 0xea6c011du, 0xb3a52736u, 0x3c8363ddu, 0x231c8a6du, 0x17b061e0u},
    {0x0000000bu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x4115fad0u, 0xc6da3c65u, 0x6ec2b1e9u, 0x587adf8fu, 0x981a17aau, 0xd0d7ceb2u, 0x68b7d3f1u, 0x14b2cba6u,
     0xdb08d178u, 0xcc76b38fu, 0x86e2ec38u, 0x40034dc6u, 0xea6fbf85u, 0x5cd6a4f2u, 0xb378ffecu, 0x0fed929du},
};
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
const uint32_t* curve_start_candidate_words(int E, unsigned j) { return E == 1 ? G1_STARTS[j] : G2_STARTS[j]; }
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

extern "C" int sbn_start_candidate(int32_t kind, uint32_t j, uint32_t* out) {
  const int E = pi_layout((int)kind).E;
  if (!E) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not a curve table", (int)kind);
  if (!out) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (j >= SBN_START_CANDIDATES) return fail(SBN_ERR_BAD_ARG, "start candidate %u: there are %d (0 .. %d)", j, SBN_START_CANDIDATES, SBN_START_CANDIDATES - 1);
  memcpy(out, curve_start_candidate_words(E, j), curve_layout(E).xw * sizeof(uint32_t));
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
