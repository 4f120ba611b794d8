// Host helpers over bn254w.cuh shared by the units that derive instance lists on the host pool (through instance_lists.hpp):
// u32-limb loads and stores, the curve constants, the on-curve test, the norm-based inversion of a Z, and the batched affine form
// of a list of Jacobian points that may hold the point at infinity.
#pragma once
#include "host_common.hpp"
#include "bn254w.cuh"
#include <atomic>
#include <cstring>

namespace sbn {
namespace curve_host {
using namespace bnw;

inline void ld_u32(const uint32_t* w, u64* out) { for (int i = 0; i < 4; i++) out[i] = (u64)w[2 * i] | ((u64)w[2 * i + 1] << 32); }
inline void st_u32(const Fq& m, uint32_t* w) { u64 s[4]; from_m(m, s); for (int i = 0; i < 8; i++) w[i] = (uint32_t)(s[i >> 1] >> (32 * (i & 1))); }
inline Fq fq_small(u64 v) { u64 t[4] = {v, 0, 0, 0}; return to_m(t); }
inline Fq fq_inv_m(const Fq& a) { u64 s[4], si[4]; from_m(a, s); inv_std(s, si); return to_m(si); }

// the curve constant b of y^2 = x^3 + b: 3 on G1, 3 / (9 + i) = (27 - 3i) / 82 on the twist
template <int E> Co<E> curve_b() {
  Co<E> r;
  if (E == 1) { r.c[0] = fq_small(3); return r; }
  const Fq i82 = fq_inv_m(fq_small(82)), z = {{0, 0, 0, 0}};
  r.c[0] = mmul(fq_small(27), i82); r.c[E - 1] = fsub(z, mmul(fq_small(3), i82));
  return r;
}
template <int E> bool on_curve(const Co<E>& x, const Co<E>& y, const Co<E>& b) {
  return czero<E>(csub(cmul(y, y), cadd(cmul(cmul(x, x), x), b)));
}
inline Fq norm_of(const Co<1>& a) { return a.c[0]; }
inline Fq norm_of(const Co<2>& a) { return fadd(mmul(a.c[0], a.c[0]), mmul(a.c[1], a.c[1])); }
inline Co<1> inv_from_norm(const Co<1>&, const Fq& ni) { Co<1> r; r.c[0] = ni; return r; }
inline Co<2> inv_from_norm(const Co<2>& a, const Fq& ni) { Co<2> r; r.c[0] = mmul(a.c[0], ni); r.c[1] = fsub(Fq{{0, 0, 0, 0}}, mmul(a.c[1], ni)); return r; }

// `values` Fq elements of 8 u32 words each are below p
inline bool below_p(const uint32_t* w, int values) {
  for (int v = 0; v < values; v++) { u64 t[4]; ld_u32(w + 8 * v, t); if (geq_p(t)) return false; }
  return true;
}

// x.c0 [x.c1] y.c0 [y.c1], 8 u32 words each -> the affine point, Z = 1
template <int E> Jac<E> ld_point(const uint32_t* w) {
  Jac<E> p; u64 t[4];
  for (int q = 0; q < E; q++) { ld_u32(w + 8 * q, t); p.X.c[q] = to_m(t); ld_u32(w + 8 * (E + q), t); p.Y.c[q] = to_m(t); }
  p.Z = cone<E>();
  return p;
}

// e x for a 256-bit e (eight u32 limbs, not reduced), most significant bit first, with the complete addition
template <int E> Jac<E> scalar_mul_jac(const Jac<E>& x, const uint32_t* e) {
  Jac<E> acc = jac_infinity<E>();
  for (int t = 255; t >= 0; t--) {
    acc = jac_double<E>(acc);
    if ((e[t >> 5] >> (t & 31)) & 1) acc = jac_add_complete<E>(acc, x);
  }
  return acc;
}

template <int E> Jac<E> neg_point(const Jac<E>& p) { Jac<E> r = p; r.Y = csub(csub(p.Y, p.Y), p.Y); return r; }

// K Jacobian points -> affine u32 words ([K][16E]) and flags ([K], 1 = the point at infinity, its words zero): one inversion for
// every non-zero Z (through the norms on the twist); either output may be null
template <int E> void affine_or_infinity(const std::vector<Jac<E>>& pts, uint32_t* words, uint8_t* inf) {
  const size_t K = pts.size();
  std::vector<Fq> nrm(K), pre(K);
  Fq acc = fq_one();
  for (size_t k = 0; k < K; k++) {
    const bool z = czero<E>(pts[k].Z);
    if (inf) inf[k] = z ? 1 : 0;
    nrm[k] = z ? fq_one() : norm_of(pts[k].Z);
    pre[k] = acc; acc = mmul(acc, nrm[k]);
  }
  if (!words) return;
  Fq inv = fq_inv_m(acc);
  for (size_t k = K; k-- > 0;) { const Fq ni = mmul(inv, pre[k]); inv = mmul(inv, nrm[k]); nrm[k] = ni; }
  for (size_t k = 0; k < K; k++) {
    uint32_t* out = words + 16 * E * k;
    if (czero<E>(pts[k].Z)) { memset(out, 0, 16 * E * sizeof(uint32_t)); continue; }
    const Co<E> zi = inv_from_norm(pts[k].Z, nrm[k]), zi2 = cmul(zi, zi);
    const Co<E> x = cmul(pts[k].X, zi2), y = cmul(pts[k].Y, cmul(zi2, zi));
    for (int q = 0; q < E; q++) { st_u32(x.c[q], out + 8 * q); st_u32(y.c[q], out + 8 * (E + q)); }
  }
}
}  // namespace curve_host
}  // namespace sbn
