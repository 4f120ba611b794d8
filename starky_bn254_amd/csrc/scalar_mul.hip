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
#include "curve_host.hpp"
#include <cstring>

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

inline int curve_e(int kind) { return kind == SBN_AIR_G1_EXP ? 1 : (kind == SBN_AIR_G2_EXP ? 2 : 0); }

// the table's own walk (g1/exp.rs:165-230) of the K instances of an explicit list, one at a time: the first one it cannot walk
template <int E> int name_degenerate(const uint32_t* ios, size_t K, size_t base = 0) {
  const size_t IOW = 32 * E + 8;
  std::atomic<size_t> bad(K);
  host_parallel_for(K, [&](size_t k) {
    if (k > bad.load()) return;
    std::vector<u64> ja(257 * 12 * E), jb(257 * 12 * E);
    if (exp_chains<E>(ios + IOW * k, 0, ja.data(), jb.data())) { size_t cur = bad.load(); while (k < cur && !bad.compare_exchange_weak(cur, k)) {} }
  });
  if (bad.load() == K) return SBN_OK;
  return fail(SBN_ERR_WITNESS, "instance %zu: degenerate affine operation in the table's walk (B[t] = +-2^t x at a set bit, or an output at infinity): pick another offset",
              base + bad.load());
}

template <int E>
int instances(const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t count, size_t num_io, const uint32_t* offset,
              uint32_t* ios_out, uint32_t* products_out, uint8_t* infinity_out) {
  const size_t IOW = 32 * E + 8, total = sbn_msm_num_units(count, num_io) * num_io;
  if (int rc = check_curve_points<E>(points, 16 * E, count, offset, "offset")) return rc;
  std::vector<uint32_t> own;
  uint32_t* ios = ios_out;
  if (!ios) { own.resize(IOW * total); ios = own.data(); }
  scalar_mul_explicit_list(E, points, scalars, scalar_count, count, total, offset, ios);
  if (products_out || infinity_out) {
    std::vector<Jac<E>> term(count);
    host_parallel_for(count, [&](size_t k) { term[k] = scalar_mul_jac<E>(ld_point<E>(points + 16 * E * k), scalars + (scalar_count == 1 ? 0 : 8 * k)); });
    affine_or_infinity<E>(term, products_out, infinity_out);
  }
  // the table's own walk of the real instances (the pads repeat the last one), 512 instances at a time to bound the chain storage
  const size_t CH = 512;
  std::vector<u64> chains(2 * 257 * 12 * E * (count < CH ? count : CH));
  for (size_t at = 0; at < count; at += CH) {
    const size_t k = count - at < CH ? count - at : CH, cw = 257 * 12 * E * k;
    if (!tracegen_host_chains(E, ios + IOW * at, k, chains.data(), chains.data() + cw)) continue;
    if (int rc = name_degenerate<E>(ios + IOW * at, k, at)) return rc;
    return fail(SBN_ERR_WITNESS, "degenerate affine operation (x1 == x2 or y == 0)");
  }
  return SBN_OK;
}

template <int E>
int check(size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, const uint32_t* points, const uint32_t* scalars,
          size_t scalar_count, const uint32_t* offset, uint32_t* products_out, uint8_t* infinity_out) {
  const size_t W = 16 * E, per = 3 * W + 8, oX = 0, oOff = W, oExp = 2 * W, oOut = 2 * W + 8;
  if (units != sbn_msm_num_units(count, num_io))
    return fail(SBN_ERR_VERIFY_FAILED, "%zu units given, a list of %zu instances in tables of %zu has %zu units", units, count, num_io, sbn_msm_num_units(count, num_io));
  for (size_t u = 0; u < units; u++) if (!public_inputs[u]) return fail(SBN_ERR_BAD_ARG, "null public inputs (unit %zu)", u);
  auto inst = [&](size_t g) { return public_inputs[g / num_io] + per * (g % num_io); };
  auto same = [](const uint64_t* p, const uint32_t* w, size_t n) { for (size_t i = 0; i < n; i++) if (p[i] != w[i]) return false; return true; };
  const uint64_t* last = inst(count - 1);
  const Co<E> b = curve_b<E>();
  std::vector<uint32_t> outs(W * count);
  for (size_t g = 0; g < units * num_io; g++) {
    const uint64_t* p = inst(g);
    if (g >= count) {   // a pad instance is instance count - 1 again
      static const char* const field[4] = {"x", "offset", "exponent", "output"};
      const size_t at[4] = {oX, oOff, oExp, oOut}, len[4] = {W, W, 8, W};
      for (int f = 0; f < 4; f++)
        if (memcmp(p + at[f], last + at[f], len[f] * sizeof(uint64_t)))
          return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (pad): %s differs from instance %zu", g, field[f], count - 1);
      continue;
    }
    if (!same(p + oX, points + W * g, W)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: x differs from the caller's point", g);
    if (!same(p + oExp, scalars + (scalar_count == 1 ? 0 : 8 * g), 8)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: exponent differs from the caller's scalar", g);
    if (!same(p + oOff, offset, W)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: offset differs from the offset of the call", g);
    for (size_t i = 0; i < W; i++) {
      if (p[oOut + i] > 0xffffffffULL) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output limb %zu is out of range", g, i);
      outs[W * g + i] = (uint32_t)p[oOut + i];
    }
    const uint32_t* o = outs.data() + W * g;
    if (!below_p(o, 2 * E)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output has a coordinate >= p", g);
    const Jac<E> q = ld_point<E>(o);
    if (!on_curve<E>(q.X, q.Y, b)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output is not a point of the curve", g);
  }
  if (products_out || infinity_out) scalar_mul_unoffset_host(E, outs.data(), offset, count, products_out, infinity_out);
  return SBN_OK;
}

// kind, then the arguments every entry point shares, in the order of the header's refusals
int check_args(int32_t kind, const void* points, const void* scalars, size_t scalar_count, size_t count, size_t num_io) {
  if (!curve_e((int)kind)) return fail(SBN_ERR_UNSUPPORTED, "scalar multiplications cover the curve tables G1_EXP and G2_EXP (a field table takes offset = 1 as it is)");
  if (!points || !scalars || count == 0 || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no instance or num_io = 0");
  if (scalar_count != 1 && scalar_count != count) return fail(SBN_ERR_BAD_ARG, "scalar_count must be 1 (one shared scalar) or count = %zu, got %zu", count, scalar_count);
  return SBN_OK;
}
}  // namespace

namespace sbn {
const uint32_t* curve_generator_words(int E) { return E == 1 ? G1_GEN : G2_GEN; }
const uint32_t* g2_cofactor_words() { return G2_COFACTOR; }

int scalar_mul_check_points(int E, const uint32_t* points, size_t count, const uint32_t* offset) {
  return E == 1 ? check_curve_points<1>(points, 16, count, offset, "offset") : check_curve_points<2>(points, 32, count, offset, "offset");
}

void scalar_mul_explicit_list(int E, const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t count, size_t total,
                              const uint32_t* offset, uint32_t* ios) {
  const size_t W = 16 * (size_t)E, IOW = 2 * W + 8;
  for (size_t g = 0; g < total; g++) {
    const size_t k = g < count ? g : count - 1;   // the reference's resize rule: a pad row is the last row again
    memcpy(ios + IOW * g, points + W * k, W * sizeof(uint32_t));
    memcpy(ios + IOW * g + W, offset, W * sizeof(uint32_t));
    memcpy(ios + IOW * g + 2 * W, scalars + (scalar_count == 1 ? 0 : 8 * k), 8 * sizeof(uint32_t));
  }
}

int scalar_mul_name_degenerate(int E, const uint32_t* ios, size_t K) { return E == 1 ? name_degenerate<1>(ios, K) : name_degenerate<2>(ios, K); }

template <int E> static void unoffset(const uint32_t* outputs, const uint32_t* offset, size_t K, uint32_t* products, uint8_t* infinity) {
  const Jac<E> noff = neg_point<E>(ld_point<E>(offset));
  std::vector<Jac<E>> prod(K);
  for (size_t k = 0; k < K; k++) prod[k] = jac_add_complete<E>(ld_point<E>(outputs + 16 * E * k), noff);
  affine_or_infinity<E>(prod, products, infinity);
}
void scalar_mul_unoffset_host(int E, const uint32_t* outputs, const uint32_t* offset, size_t K, uint32_t* products, uint8_t* infinity) {
  if (E == 1) unoffset<1>(outputs, offset, K, products, infinity); else unoffset<2>(outputs, offset, K, products, infinity);
}
}  // namespace sbn

extern "C" int sbn_curve_generator(int32_t kind, uint32_t* out) {
  const int E = curve_e((int)kind);
  if (!E) return fail(SBN_ERR_UNSUPPORTED, "kind %d is not a curve table", (int)kind);
  if (!out) return fail(SBN_ERR_BAD_ARG, "null argument");
  memcpy(out, curve_generator_words(E), 16 * E * sizeof(uint32_t));
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
  const int E = curve_e((int)kind);
  if (!offset) offset = curve_generator_words(E);
  return E == 1 ? instances<1>(points, scalars, scalar_count, count, num_io, offset, ios_out, products_out, infinity_out)
                : instances<2>(points, scalars, scalar_count, count, num_io, offset, ios_out, products_out, infinity_out);
}

extern "C" int sbn_scalar_mul_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, const uint32_t* points,
                                    const uint32_t* scalars, size_t scalar_count, const uint32_t* offset, uint32_t* products_out, uint8_t* infinity_out) {
  if (int rc = check_args(kind, points, scalars, scalar_count, count, num_io)) return rc;
  if (!public_inputs) return fail(SBN_ERR_BAD_ARG, "null argument");
  const int E = curve_e((int)kind);
  if (!offset) offset = curve_generator_words(E);
  if (!below_p(offset, 2 * E)) return fail(SBN_ERR_BAD_ARG, "coordinate >= p (offset)");
  return E == 1 ? check<1>(num_io, public_inputs, units, count, points, scalars, scalar_count, offset, products_out, infinity_out)
                : check<2>(num_io, public_inputs, units, count, points, scalars, scalar_count, offset, products_out, infinity_out);
}

extern "C" int sbn_mul_by_cofactor_check(size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, const uint32_t* points,
                                         uint32_t* cleared_out, uint8_t* infinity_out) {
  return sbn_scalar_mul_check(SBN_AIR_G2_EXP, num_io, public_inputs, units, count, points, G2_COFACTOR, 1, nullptr, cleared_out, infinity_out);
}
