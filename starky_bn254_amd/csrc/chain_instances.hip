// Chained instance lists on the host (sbn_chain_instances): the call shape of the reference's *_msm tests
// (src/curves/g1/circuit.rs:459-509 and its G2 / Fq12 / Fq12U64 twins), where offset[0] is a fixed start value and offset[k+1] is
// the output of instance k, so that the last output is start + sum e_k x_k on the curves and start * prod x_k^e_k in the fields.
// The reference derives every offset with arkworks per instance (G1ExpOutputGenerator::run_once, circuit.rs:111-123); here
//  * the terms e_k x_k (x_k^e_k) are independent and run on the host pool, in Jacobian coordinates with the COMPLETE addition of
//    bn254w.cuh (a term may be the identity, and the double-and-add inside a term meets equal operands when e has a leading 1
//    only): a collision in this derivation says nothing about the table's own walk and is not an error;
//  * the running sum is K complete additions, then ONE inversion turns all K + 1 points into affine coordinates;
//  * the table's own walk of the resulting explicit list is then checked with the chains the witness generators use
//    (tracegen_host_chains): only that, or an offset at infinity, refuses a list.
// tracegen_device.hip runs the same derivation on the device and falls back to this one where the chains are host work anyway.
#include "curve_host.hpp"
#include <cstring>

using namespace sbn;

namespace {
using namespace bnw;
using namespace sbn::curve_host;

template <int E> int check_curve_terms(const uint32_t* terms, size_t K, const uint32_t* start) {
  return check_curve_points<E>(terms, 16 * E + 8, K, start, "start");
}

template <int E> int chain_curve(const uint32_t* terms, size_t K, const uint32_t* start, uint32_t* ios, uint32_t* final_out) {
  const size_t T = 16 * E + 8, IOW = 32 * E + 8;
  if (int rc = check_curve_terms<E>(terms, K, start)) return rc;
  std::vector<Jac<E>> sum(K + 1);          // sum[k] = offset[k], sum[K] = the last output
  std::vector<Jac<E>> term(K);
  host_parallel_for(K, [&](size_t k) {     // e_k x_k, most significant bit first
    term[k] = scalar_mul_jac<E>(ld_point<E>(terms + T * k), terms + T * k + 16 * E);
  });
  sum[0] = ld_point<E>(start);
  for (size_t k = 0; k < K; k++) sum[k + 1] = jac_add_complete<E>(sum[k], term[k]);
  // one inversion for all Z (through the norms on the twist)
  std::vector<Fq> nrm(K + 1), pre(K + 1);
  Fq acc = fq_one();
  for (size_t k = 0; k <= K; k++) {
    if (czero<E>(sum[k].Z)) {
      if (k == K) return fail(SBN_ERR_WITNESS, "the output of instance %zu is the point at infinity", K - 1);
      return fail(SBN_ERR_WITNESS, "the offset of instance %zu is the point at infinity", k);
    }
    nrm[k] = norm_of(sum[k].Z); pre[k] = acc; acc = mmul(acc, nrm[k]);
  }
  Fq inv = fq_inv_m(acc);
  for (size_t k = K + 1; k-- > 0;) { const Fq ni = mmul(inv, pre[k]); inv = mmul(inv, nrm[k]); nrm[k] = ni; }
  auto affine = [&](size_t k, uint32_t* out) {   // x.c0 [x.c1] y.c0 [y.c1], 8 u32 words each
    const Co<E> zi = inv_from_norm(sum[k].Z, nrm[k]), zi2 = cmul(zi, zi);
    const Co<E> x = cmul(sum[k].X, zi2), y = cmul(sum[k].Y, cmul(zi2, zi));
    for (int q = 0; q < E; q++) { st_u32(x.c[q], out + 8 * q); st_u32(y.c[q], out + 8 * (E + q)); }
  };
  for (size_t k = 0; k < K; k++) {
    memcpy(ios + IOW * k, terms + T * k, 16 * E * sizeof(uint32_t));
    affine(k, ios + IOW * k + 16 * E);
    memcpy(ios + IOW * k + 32 * E, terms + T * k + 16 * E, 8 * sizeof(uint32_t));
  }
  if (final_out) affine(K, final_out);
  // the table's own walk of the explicit list (g1/exp.rs:165-230): B[t] = +-A[t] at an addition refuses it
  const size_t cw = 257 * 12 * E * K;
  std::vector<u64> chains(2 * cw);
  if (tracegen_host_chains(E, ios, K, chains.data(), chains.data() + cw)) return fail(SBN_ERR_WITNESS, "degenerate affine operation (x1 == x2 or y == 0)");
  return SBN_OK;
}

// FqExpStark: offset[k+1] = offset[k] x_k^e_k
int chain_fq(const uint32_t* terms, size_t K, const uint32_t* start, uint32_t* ios, uint32_t* final_out) {
  if (!below_p(start, 1)) return fail(SBN_ERR_BAD_ARG, "value >= p (start)");
  for (size_t k = 0; k < K; k++) if (!below_p(terms + 16 * k, 1)) return fail(SBN_ERR_BAD_ARG, "value >= p (instance %zu)", k);
  std::vector<Fq> term(K);
  host_parallel_for((K + 7) / 8, [&](size_t g) {
    for (size_t k = 8 * g; k < K && k < 8 * g + 8; k++) {
      u64 t4[4]; ld_u32(terms + 16 * k, t4);
      Fq a = to_m(t4), b = fq_one();
      const uint32_t* e = terms + 16 * k + 8;
      for (int t = 0; t < 256; t++) { if ((e[t >> 5] >> (t & 31)) & 1) b = mmul(a, b); a = mmul(a, a); }
      term[k] = b;
    }
  });
  u64 t4[4]; ld_u32(start, t4);
  Fq off = to_m(t4);
  for (size_t k = 0; k < K; k++) {
    memcpy(ios + 24 * k, terms + 16 * k, 8 * sizeof(uint32_t));
    st_u32(off, ios + 24 * k + 8);
    memcpy(ios + 24 * k + 16, terms + 16 * k + 8, 8 * sizeof(uint32_t));
    off = mmul(off, term[k]);
  }
  if (final_out) st_u32(off, final_out);
  return SBN_OK;
}

// Fq12ExpStark (ew = 8) / Fq12ExpU64Stark (ew = 2)
int chain_fq12(const uint32_t* terms, size_t K, const uint32_t* start, uint32_t* ios, uint32_t* final_out, size_t ew) {
  const size_t T = 96 + ew, IOW = 192 + ew;
  if (!below_p(start, 12)) return fail(SBN_ERR_BAD_ARG, "coefficient >= p (start)");
  for (size_t k = 0; k < K; k++) {
    if (!below_p(terms + T * k, 12)) return fail(SBN_ERR_BAD_ARG, "coefficient >= p (instance %zu)", k);
    if (ew == 2 && ((u64)terms[T * k + 96] | ((u64)terms[T * k + 97] << 32)) >= GLP)
      return fail(SBN_ERR_NON_CANONICAL, "exponent of instance %zu is not a canonical field element", k);
  }
  std::vector<Fq> term(12 * K);
  host_parallel_for(K, [&](size_t k) {
    Fq a[12], b[12], prod[12];
    for (int c = 0; c < 12; c++) { u64 t4[4]; ld_u32(terms + T * k + 8 * c, t4); a[c] = to_m(t4); b[c] = Fq{{0, 0, 0, 0}}; }
    b[0] = fq_one();
    const uint32_t* e = terms + T * k + 96;
    for (int t = 0; t < (int)(32 * ew); t++) {
      if ((e[t >> 5] >> (t & 31)) & 1) { fq12_mul_m(a, b, prod); memcpy(b, prod, sizeof b); }
      fq12_mul_m(a, a, prod); memcpy(a, prod, sizeof a);
    }
    memcpy(&term[12 * k], b, sizeof b);
  });
  Fq off[12], prod[12];
  for (int c = 0; c < 12; c++) { u64 t4[4]; ld_u32(start + 8 * c, t4); off[c] = to_m(t4); }
  for (size_t k = 0; k < K; k++) {
    memcpy(ios + IOW * k, terms + T * k, 96 * sizeof(uint32_t));
    for (int c = 0; c < 12; c++) st_u32(off[c], ios + IOW * k + 96 + 8 * c);
    memcpy(ios + IOW * k + 192, terms + T * k + 96, ew * sizeof(uint32_t));
    fq12_mul_m(off, &term[12 * k], prod); memcpy(off, prod, sizeof off);
  }
  if (final_out) for (int c = 0; c < 12; c++) st_u32(off[c], final_out + 8 * c);
  return SBN_OK;
}
}  // namespace

namespace sbn {
int chain_terms_check_curve(int E, const uint32_t* terms, size_t K, const uint32_t* start) {
  return E == 1 ? check_curve_terms<1>(terms, K, start) : check_curve_terms<2>(terms, K, start);
}
int chain_instances_host(int kind, const uint32_t* terms, size_t K, const uint32_t* start, uint32_t* ios, uint32_t* final_out) {
  switch (kind) {
    case SBN_AIR_G1_EXP: return chain_curve<1>(terms, K, start, ios, final_out);
    case SBN_AIR_G2_EXP: return chain_curve<2>(terms, K, start, ios, final_out);
    case SBN_AIR_FQ_EXP: return chain_fq(terms, K, start, ios, final_out);
    case SBN_AIR_FQ12_EXP: return chain_fq12(terms, K, start, ios, final_out, 8);
    case SBN_AIR_FQ12_EXP_U64: return chain_fq12(terms, K, start, ios, final_out, 2);
    default: return fail(SBN_ERR_BAD_ARG, "kind %d is not an Exp table", kind);
  }
}
}  // namespace sbn

extern "C" int sbn_chain_instances(int32_t kind, const uint32_t* terms, size_t count, const uint32_t* start, uint32_t* ios_out, uint32_t* final_out) {
  if (!terms || !start || !ios_out || count == 0) return fail(SBN_ERR_BAD_ARG, "null argument or no instance");
  return chain_instances_host((int)kind, terms, count, start, ios_out, final_out);
}
