// Device witness generation for G1ExpStark and G2ExpStark (E = 1, 2): replaces generate_trace / generate_public_inputs
// (src/curves/g1/exp.rs:255-327, src/curves/g2/exp.rs:271-342) with kernels that fill the column-major trace directly in HBM, so the 0.9 GB
// trace never crosses PCIe.  The host generator (tracegen.hip) is the bit-exact counterpart; both share bn254w.cuh.
//
// The reference's per-instance loop is sequential in two ways: a = 2^t x is a chain of doublings and
// b += a is a chain of additions, and every affine step needs a field inversion.  Here
//   * both chains of an instance are walked in Jacobian coordinates (no inversion): bn254w.cuh g1_chains, run on host
//     threads by default (512 strictly sequential point operations per instance are 0.1% of the arithmetic and
//     latency-bound on a lane) or by chain_kernel, one lane per instance;
//   * affine_lambda_kernel then inverts all Z's and all slope denominators at once (the inversions of different
//     rows are independent once the chain is known, and the denominators have closed forms in Jacobian coordinates): a lane owns
//     the eight values of two rows and inverts their product (Montgomery's trick; Fermat, a^(p-2), for the one inversion left);
//   * gadget_witness_kernel computes the limb columns and the modular-gadget witnesses, one lane per (row, gadget);
//   * flags / pulse columns are closed forms of the row index;
//   * range_check_kernel: one workgroup per range-checked column, histogram and prefix counts in LDS, and the
//     reference's sorted-merge with its LIFO pool of unused table values (src/utils/lookup.rs:60-111) restated as
//     independent searches over the prefix counts.
#pragma once
#include "bn254w.cuh"

namespace tg {
using namespace bnw;


// a^(p-2) with 4-bit fixed windows (252 squarings + <= 64 + 14 products).  The inversion helpers below are host-device only so that
// sbn_bn254_fq_batch (tracegen_device.hip) can run the host build of them as well; the kernels use the device build.
__host__ __device__ __noinline__ Fq finv_fermat(const Fq& a) {
  constexpr u64 PL[4] = BNW_PL;
  const u64 e[4] = {PL[0] - 2, PL[1], PL[2], PL[3]};
  Fq tab[16];
  tab[0] = fq_one(); tab[1] = a;
  for (int i = 2; i < 16; i++) tab[i] = mmul(tab[i - 1], a);
  Fq r = tab[(e[3] >> 60) & 15];
  for (int w = 62; w >= 0; w--) {
    r = mmul(r, r); r = mmul(r, r); r = mmul(r, r); r = mmul(r, r);
    const unsigned nib = (unsigned)(e[w >> 4] >> (4 * (w & 15))) & 15;
    if (nib) r = mmul(r, tab[nib]);
  }
  return r;
}


// Inversions are BATCHED inside a lane (Montgomery's trick): a lane multiplies up the TG_INV_BATCH values it owns, inverts the
// product with one Fermat chain (~330 multiplies) and walks back with two multiplies per value, so an inversion costs ~45
// multiplies instead of ~330.  A coordinate in Fq2 is inverted through its norm a^2 + b^2 (an Fq value): 1/(a + bi) = (a - bi) / norm.
static constexpr int TG_INV_BATCH = 8;
GL_HD Fq cnorm(const Co<1>& a) { return a.c[0]; }
GL_HD Fq cnorm(const Co<2>& a) { return fadd(mmul(a.c[0], a.c[0]), mmul(a.c[1], a.c[1])); }
GL_HD Co<1> cinv_from_norm(const Co<1>&, const Fq& ni) { Co<1> r; r.c[0] = ni; return r; }
GL_HD Co<2> cinv_from_norm(const Co<2>& a, const Fq& ni) {
  Co<2> r; r.c[0] = mmul(a.c[0], ni); r.c[1] = fsub(Fq{{0, 0, 0, 0}}, mmul(a.c[1], ni));
  return r;
}
// nrm[j] (all non-zero) -> nrm[j]^-1, j < TG_INV_BATCH
GL_HD void batch_inverse(Fq (&nrm)[TG_INV_BATCH]) {
  Fq pre[TG_INV_BATCH];
  pre[0] = nrm[0];
#pragma unroll
  for (int j = 1; j < TG_INV_BATCH; j++) pre[j] = mmul(pre[j - 1], nrm[j]);
  Fq inv = finv_fermat(pre[TG_INV_BATCH - 1]);
#pragma unroll
  for (int j = TG_INV_BATCH - 1; j > 0; j--) {
    const Fq ni = mmul(inv, pre[j - 1]);
    inv = mmul(inv, nrm[j]);
    nrm[j] = ni;
  }
  nrm[0] = inv;
}

// One lane per instance: exp_chains (bn254w.cuh).  512 strictly sequential point operations per lane: the host
// threads do this faster (prover.hip picks), the kernel keeps the path host-free when asked (SBN_TRACEGEN_DEVICE_CHAIN=1).
template <int E>
__global__ void chain_kernel(const uint32_t* __restrict__ ios, size_t K, u64* __restrict__ ja, u64* __restrict__ jb, int* __restrict__ err) {
  const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int bad = exp_chains<E>(ios + 8 * (4 * E + 1) * k, k, ja, jb);
  if (bad) atomicOr(err, bad);
}

// ---- the curve chains with ONE WAVE per instance (round 3) --------------------------------------------------------------------
// exp_chains is 512 dependent point operations per instance: 13 ms on one lane, 2.2 ms on the host pool.  But a Jacobian doubling
// and an addition are ~25 Fq (4 x that: Fq2) products of which up to 8 (32) are independent, and the doubling of a and the addition
// b += a of one step do not depend on each other.  The host lays one step out as LEVELS of independent micro-operations over Fq
// slots (ChainProgram in tracegen_device.hip: every product, sum, difference of jac_double / jac_add, Fq2 products expanded into their four
// Fq products; level = longest dependency path), and a wave executes a level with one micro-operation per lane, operands and
// results in LDS.  Field arithmetic is exact, so the stored Jacobian coordinates are word for word those of exp_chains.
// Micro-operation word: kind | dst << 8 | a << 16 | b << 24 (slot numbers < 256).
enum { CP_NOP = 0, CP_MUL = 1, CP_ADD = 2, CP_SUB = 3, CP_COPY = 4, CP_CHK1 = 5, CP_CHK2 = 6, CP_LANES = 64, CP_MAX_SLOTS = 256 };
struct ChainProgDev {
  const uint32_t* ops[2];     // [bit]: [levels][CP_LANES] micro-operations
  int levels[2];
  unsigned char in_slot[8];   // slots of x.x x.y offset.x offset.y (E each, component-major as in the io words)
  unsigned char one_slot[2];  // first components of a.Z and b.Z (set to 1; the other components to 0)
  unsigned char zero_slot[2]; // second components of a.Z and b.Z (E = 2; 255 = none)
  unsigned char coord[12];    // slots of a.X a.Y a.Z b.X b.Y b.Z, E each
};
template <int E>
__global__ void __launch_bounds__(CP_LANES) chain_coop_kernel(const uint32_t* __restrict__ ios, size_t K, u64* __restrict__ ja, u64* __restrict__ jb,
                                                              int* __restrict__ err, ChainProgDev cp) {
  __shared__ Fq V[CP_MAX_SLOTS];
  __shared__ uint32_t prog[2][24 * CP_LANES];     // both programs (<= 24 levels each), read 256 times: kept in LDS
  const size_t k = blockIdx.x;
  const int lane = threadIdx.x;
  for (int b = 0; b < 2; b++) for (int lv = 0; lv < cp.levels[b]; lv++) prog[b][lv * CP_LANES + lane] = cp.ops[b][lv * CP_LANES + lane];
  const uint32_t* io = ios + 8 * (4 * E + 1) * k;
  if (lane < 4 * E) { u64 t4[4]; u32x8_to_u64x4(io + 8 * lane, t4); V[cp.in_slot[lane]] = to_m(t4); }
  if (lane >= 32 && lane < 34) V[cp.one_slot[lane - 32]] = fq_one();
  if (E == 2 && lane >= 40 && lane < 42) V[cp.zero_slot[lane - 40]] = Fq{{0, 0, 0, 0}};
  __syncthreads();
  const uint32_t* e = io + 32 * E;
  for (int t = 0;; t++) {
    if (lane < 6 * E) {                       // the Jacobian coordinates of step t, Montgomery form (affine_lambda_kernel reads them)
      const int which = lane / (3 * E), cc = (lane % (3 * E)) / E, q = lane % E;
      const Fq v = V[cp.coord[lane]];
      u64* dst = (which ? jb : ja) + jac_at<E>(k, t, cc) + 4 * q;
      for (int i = 0; i < 4; i++) dst[i] = v.l[i];
    }
    if (t == 256) break;
    const int bit = (e[t >> 5] >> (t & 31)) & 1;
    const uint32_t* ops = prog[bit];
    const int nl = cp.levels[bit];
    for (int lv = 0; lv < nl; lv++) {
      const uint32_t op = ops[lv * CP_LANES + lane];
      const int kind = op & 255, d = (op >> 8) & 255, a = (op >> 16) & 255, b = op >> 24;
      if (kind == CP_MUL) V[d] = mmul(V[a], V[b]);
      else if (kind == CP_ADD) V[d] = fadd(V[a], V[b]);
      else if (kind == CP_SUB) V[d] = fsub(V[a], V[b]);
      else if (kind == CP_COPY) V[d] = V[a];
      else if (kind == CP_CHK1) { if (fzero(V[a])) atomicOr(err, TG_ERR_DEGENERATE); }
      else if (kind == CP_CHK2) { if (fzero(V[a]) && fzero(V[b])) atomicOr(err, TG_ERR_DEGENERATE); }
      __syncthreads();
    }
  }
}

// Row r of instance k: a = A[r>>1]; even rows: b = B[r>>1], add if bit; odd rows: b = B[(r>>1)+1], double.
template <int E>
struct LambdaRow {
  size_t k; int t, tb, op; bool dbl;
  __device__ __forceinline__ LambdaRow(const uint32_t* __restrict__ ios, size_t row) {
    k = row >> 9; const int r = (int)(row & 511); t = r >> 1; dbl = r & 1;
    const bool bit = (ios[8 * (4 * E + 1) * k + 32 * E + (t >> 5)] >> (t & 31)) & 1;
    op = dbl ? 2 : (bit ? 1 : 0);
    tb = dbl ? t + 1 : t;
  }
};
// One lane per TG_ROWS rows (row = L + j NL), straight from the JACOBIAN chains: the standard-form values ax ay bx by lam nx ny of
// the row (sv[((v*E + q)*4 + limb) * n + row]) and its operation (0 none, 1 add, 2 double); also the instance output B[256] (u32
// limbs) for the public inputs.  Rounds 2-3 ran two kernels, each waiting for one Fermat chain (~350 dependent products, 0.44 +
// 0.49 ms): affine_kernel inverted every Z, lambda_kernel then the slope denominators.  The denominators have closed forms in
// Jacobian coordinates -- x2 - x1 = (X2 Z1^2 - X1 Z2^2) / (Z1^2 Z2^2), 2 y1 = 2 Y1 / Z1^3 -- so ONE batch per lane inverts Z1, Z2,
// Z_next and D = X2 Z1^2 - X1 Z2^2 (or 2 Y1) of its rows together (Montgomery's trick, one Fermat chain), and
// lambda = (y2 - y1) Z1^2 Z2^2 / D  (or 3 x1^2 Z1^3 / (2 Y1)).  Field elements are exact, so every word written equals the two-kernel
// path's.  D = 0 iff the affine denominator is 0 (the Z's are non-zero): the same instances are refused.
static constexpr int TG_ROWS = TG_INV_BATCH / 4;
template <int E>
__global__ void affine_lambda_kernel(const uint32_t* __restrict__ ios, size_t K, const u64* __restrict__ ja, const u64* __restrict__ jb, size_t n,
                                     u64* __restrict__ sv, unsigned char* __restrict__ row_op, u64* __restrict__ pi_out, int* __restrict__ err) {
  const size_t L = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t NL = (n + TG_ROWS - 1) / TG_ROWS;
  if (L >= NL) return;
  Fq nrm[TG_INV_BATCH];
  for (int j = 0; j < TG_ROWS; j++) {
    const size_t row = L + (size_t)j * NL;
    for (int i = 0; i < 4; i++) nrm[4 * j + i] = fq_one();
    if (row >= n) continue;
    const LambdaRow<E> R(ios, row);
    const Co<E> Z1 = ldc<E>(ja + jac_at<E>(R.k, R.t, 2)), Z2 = ldc<E>(jb + jac_at<E>(R.k, R.tb, 2));
    if (czero<E>(Z1) || czero<E>(Z2)) { atomicOr(err, TG_ERR_DEGENERATE); continue; }   // (a zero would poison the batch; the proof is refused anyway)
    nrm[4 * j] = cnorm(Z1); nrm[4 * j + 1] = cnorm(Z2);
    if (!R.op) continue;
    const Co<E> Zn = ldc<E>((R.dbl ? ja : jb) + jac_at<E>(R.k, R.t + 1, 2));
    Co<E> D;
    if (R.dbl) { const Co<E> Y1 = ldc<E>(ja + jac_at<E>(R.k, R.t, 1)); D = cadd(Y1, Y1); }
    else D = csub(cmul(ldc<E>(jb + jac_at<E>(R.k, R.tb, 0)), cmul(Z1, Z1)), cmul(ldc<E>(ja + jac_at<E>(R.k, R.t, 0)), cmul(Z2, Z2)));
    if (czero<E>(Zn) || czero<E>(D)) { atomicOr(err, TG_ERR_DEGENERATE); continue; }
    nrm[4 * j + 2] = cnorm(Zn); nrm[4 * j + 3] = cnorm(D);
  }
  batch_inverse(nrm);
  for (int j = 0; j < TG_ROWS; j++) {
    const size_t row = L + (size_t)j * NL;
    if (row >= n) continue;
    const LambdaRow<E> R(ios, row);
    const size_t k = R.k; const int t = R.t, op = R.op; const bool dbl = R.dbl;
    const Co<E> X1 = ldc<E>(ja + jac_at<E>(k, t, 0)), Y1 = ldc<E>(ja + jac_at<E>(k, t, 1)), Z1 = ldc<E>(ja + jac_at<E>(k, t, 2));
    const Co<E> X2 = ldc<E>(jb + jac_at<E>(k, R.tb, 0)), Y2 = ldc<E>(jb + jac_at<E>(k, R.tb, 1)), Z2 = ldc<E>(jb + jac_at<E>(k, R.tb, 2));
    Co<E> v[7];
    const Co<E> zi1 = cinv_from_norm(Z1, nrm[4 * j]), zi1s = cmul(zi1, zi1);
    const Co<E> zi2 = cinv_from_norm(Z2, nrm[4 * j + 1]), zi2s = cmul(zi2, zi2);
    v[0] = cmul(X1, zi1s); v[1] = cmul(Y1, cmul(zi1s, zi1));
    v[2] = cmul(X2, zi2s); v[3] = cmul(Y2, cmul(zi2s, zi2));
    if (op) {
      const Co<E> Z1s = cmul(Z1, Z1);
      Co<E> D, num, scale;
      if (dbl) { D = cadd(Y1, Y1); const Co<E> x2 = cmul(v[0], v[0]); num = cadd(cadd(x2, x2), x2); scale = cmul(Z1s, Z1); }
      else { const Co<E> Z2s = cmul(Z2, Z2); D = csub(cmul(X2, Z1s), cmul(X1, Z2s)); num = csub(v[3], v[1]); scale = cmul(Z1s, Z2s); }
      v[4] = cmul(cmul(num, scale), cinv_from_norm(D, nrm[4 * j + 3]));
      const u64* nsrc = dbl ? ja : jb;
      const Co<E> Xn = ldc<E>(nsrc + jac_at<E>(k, t + 1, 0)), Yn = ldc<E>(nsrc + jac_at<E>(k, t + 1, 1)), Zn = ldc<E>(nsrc + jac_at<E>(k, t + 1, 2));
      const Co<E> zin = cinv_from_norm(Zn, nrm[4 * j + 2]), zins = cmul(zin, zin);
      v[5] = cmul(Xn, zins); v[6] = cmul(Yn, cmul(zins, zin));
    }
    for (int w = 0; w < (op ? 7 : 4); w++)
      for (int q = 0; q < E; q++) {
        u64 s[4]; from_m(v[w].c[q], s);
        for (int i = 0; i < 4; i++) sv[(size_t)((w * E + q) * 4 + i) * n + row] = s[i];
      }
    row_op[row] = (unsigned char)op;
    if ((row & 511) == 511) {  // b at the last row is the output (g1/exp.rs:124-135, g2/exp.rs:139-156)
      for (int c = 0; c < 2; c++)
        for (int q = 0; q < E; q++) {
          u64 s[4]; from_m(v[2 + c].c[q], s);
          for (int i = 0; i < 8; i++) pi_out[16 * E * k + 8 * (c * E + q) + i] = (s[i >> 1] >> (32 * (i & 1))) & 0xffffffffULL;
        }
    }
  }
}

// One lane per (row, modular gadget): lane (row, g), g = blk * E + q, computes gadget blk (0: the zero polynomial of the
// slope, 1: new_x, 2: new_y; generate_g1_add / _double muladd.rs:124-177, 409-460 and their G2 twins) for the Fq2 component
// q -- its limb convolutions (component q of an Fq2 product is two 16 x 16 convolutions), its modular witness -- and writes
// that gadget's columns; the blk 0 lanes also write the limb columns of lambda / new_x / new_y, the blk 1 / 2 lanes those of
// a / b.  Lanes of a wave share g (lane index = g * n + row), so they neither diverge nor scatter their stores.
// Round 1 had one lane per ROW with all three (six) gadgets: 7.4 KB (13.5 KB) of scratch arrays per lane, 3,458 spilled
// registers, 1.98 GB of traffic for a 0.88 GB trace.
template <int E>
__device__ __forceinline__ void prod_comp(const int64_t (*X)[16], const int64_t (*Y)[16], int q, int64_t* out) {
  if (E == 1) { conv16(X[0], Y[0], out); return; }
  int64_t t[31];   // Fq2 limb product (src/fields/fq2.rs:41-58): c0 = x0*y0 - x1*y1, c1 = x0*y1 + x1*y0
  if (q == 0) { conv16(X[0], Y[0], out); conv16(X[E - 1], Y[E - 1], t); for (int k = 0; k < 31; k++) out[k] -= t[k]; }
  else { conv16(X[0], Y[E - 1], out); conv16(X[E - 1], Y[0], t); for (int k = 0; k < 31; k++) out[k] += t[k]; }
}
template <int E>
__global__ void __launch_bounds__(256) gadget_witness_kernel(const u64* __restrict__ sv, const unsigned char* __restrict__ row_op, size_t n, int gadget_col,
                                                             u64* __restrict__ trace, int* __restrict__ err) {
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (tid >= 3 * E * n) return;
  const size_t row = tid % n;
  const int g = (int)(tid / n), blk = g / E, q = g % E;
  const int op = row_op[row];
  // sv (affine_lambda_kernel): value w in {ax ay bx by lam nx ny}, component c, 64-bit word i at ((w * E + c) * 4 + i) * n + row
  auto ld = [&](int w, int c, u64* out4) { for (int i = 0; i < 4; i++) out4[i] = sv[(size_t)((w * E + c) * 4 + i) * n + row]; };
  auto ldl = [&](int w, int c, int64_t* out16) { u64 t4[4]; ld(w, c, t4); limbs16(t4, out16); };
  u64* gc = trace + (size_t)gadget_col * n + row;
  auto putc = [&](int c, u64 v) { gc[(size_t)c * n] = v; };
  if (blk >= 1)   // limb columns of a (blk 1: ax, ay) / b (blk 2: bx, by), component q: trace columns 16 (w E + q) ..
    for (int c = 0; c < 2; c++) {
      const int w = 2 * (blk - 1) + c;
      u64 s4[4]; ld(w, q, s4);
      for (int i = 0; i < 16; i++) trace[(size_t)(16 * (w * E + q) + i) * n + row] = (s4[i >> 2] >> (16 * (i & 3))) & 0xffff;
    }
  // G1Output / G2Output columns (muladd.rs:79-94, g2/muladd.rs:56-80): limbs of lambda, new_x, new_y (48 E), the zero gadgets
  // (79 each), the x and y gadgets (95 each), 3 E quotient signs
  const int base = blk == 0 ? 48 * E + 79 * q : (blk == 1 ? 127 * E + 95 * q : 222 * E + 95 * q), sgn = 317 * E + blk * E + q;
  if (!op) {   // G1Output / G2Output::default: zeros, quotient signs = 1
    if (blk == 0) for (int i = 0; i < 16; i++) { putc(16 * q + i, 0); putc(16 * E + 16 * q + i, 0); putc(32 * E + 16 * q + i, 0); }
    for (int c = 0; c < (blk ? 95 : 79); c++) putc(base + c, 0);
    putc(sgn, 1);
    return;
  }
  const bool dbl = op == 2;
  int64_t l[E][16], X[E][16], Y[E][16], pol[31], v16[16];
  u64 outv[4] = {0, 0, 0, 0};
  for (int c = 0; c < E; c++) ldl(4, c, l[c]);
  if (blk == 0) {
    for (int i = 0; i < 16; i++) putc(16 * q + i, (u64)l[q][i]);
    ldl(5, q, v16); for (int i = 0; i < 16; i++) putc(16 * E + 16 * q + i, (u64)v16[i]);
    ldl(6, q, v16); for (int i = 0; i < 16; i++) putc(32 * E + 16 * q + i, (u64)v16[i]);
    if (dbl) {   // 2 lambda y - 3 x^2
      int64_t t2[31];
      for (int c = 0; c < E; c++) { ldl(1, c, Y[c]); ldl(0, c, X[c]); }
      prod_comp<E>(l, Y, q, pol); prod_comp<E>(X, X, q, t2);
      for (int k = 0; k < 31; k++) pol[k] = 2 * pol[k] - 3 * t2[k];
    } else {     // lambda (x2 - x1) - (y2 - y1)
      for (int c = 0; c < E; c++) { ldl(2, c, X[c]); ldl(0, c, Y[c]); for (int i = 0; i < 16; i++) X[c][i] -= Y[c][i]; }
      prod_comp<E>(l, X, q, pol);
      ldl(3, q, v16); for (int i = 0; i < 16; i++) pol[i] -= v16[i];
      ldl(1, q, v16); for (int i = 0; i < 16; i++) pol[i] += v16[i];
    }
  } else if (blk == 1) {   // lambda^2 - x1 - x2
    prod_comp<E>(l, l, q, pol);
    ldl(0, q, v16); for (int i = 0; i < 16; i++) pol[i] -= v16[i];
    ldl(dbl ? 0 : 2, q, v16); for (int i = 0; i < 16; i++) pol[i] -= v16[i];
    ld(5, q, outv);
  } else {                 // lambda (x1 - new_x) - y1
    for (int c = 0; c < E; c++) { ldl(0, c, X[c]); ldl(5, c, Y[c]); for (int i = 0; i < 16; i++) X[c][i] -= Y[c][i]; }
    prod_comp<E>(l, X, q, pol);
    ldl(1, q, v16); for (int i = 0; i < 16; i++) pol[i] -= v16[i];
    ld(6, q, outv);
  }
  ModW w;
  if (!mod_witness(pol, outv, blk > 0, w)) { atomicOr(err, TG_ERR_WITNESS); return; }
  int cur = base;
  if (blk) for (int i = 0; i < 16; i++) putc(cur++, (u64)w.out_aux_red[i]);
  for (int i = 0; i < 17; i++) putc(cur++, (u64)w.quot_abs[i]);
  for (int i = 0; i < 31; i++) putc(cur++, (u64)w.aux_lo[i]);
  for (int i = 0; i < 31; i++) putc(cur++, (u64)w.aux_hi[i]);
  putc(sgn, w.sign > 0 ? (u64)1 : GLP - 1);
}

// flags columns (flags.rs:46-134) in closed form: within the 64-row block q of an instance the u32 limb e[q] is
// consumed one bit per two rows; the limb window rotates after row 62 of the block.  iow = u32 words per instance,
// the scalar sits in its last 8.
__global__ void flags_kernel(const uint32_t* __restrict__ ios, size_t iow, size_t n, int sf, u64* __restrict__ trace) {
  const size_t row = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (row >= n) return;
  const size_t k = row >> 9; const int r = (int)(row & 511), q = r >> 6, s = r & 63, t = s >> 1;
  const uint32_t* e = ios + iow * k + (iow - 8);
  auto limb = [&](int i) -> u64 { return i < 8 ? (u64)e[i] : 0; };
  const u64 a = r & 1, b = 1 - a, bit = (limb(q) >> t) & 1;
  auto col = [&](int c) -> u64& { return trace[(size_t)(sf + c) * n + row]; };
  col(0) = r == 511; col(1) = s == 62; col(2) = a; col(3) = b; col(4) = bit * b; col(5) = bit;
  const int sh = s == 63 ? 1 : 0;
  col(6) = s == 63 ? limb(q + 1) : (limb(q) >> (t + 1));
  for (int i = 1; i < 8; i++) col(6 + i) = limb(q + i + sh);
}

// flags of the u64 table (fq12_u64/flags_u64.rs:34-94) in closed form: bit t of e is consumed on rows 2t, 2t+1 of the
// 128-row instance.  Columns is_final, a, b, filtered_bit, bit, val.
__global__ void flags_u64_kernel(const uint32_t* __restrict__ ios, size_t iow, size_t n, int sf, u64* __restrict__ trace) {
  const size_t row = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (row >= n) return;
  const size_t k = row >> 7; const unsigned r = (unsigned)(row & 127), t = r >> 1;
  const u64 e = (u64)ios[iow * k + iow - 2] | ((u64)ios[iow * k + iow - 1] << 32);
  const u64 a = r & 1, b = 1 - a, bit = (e >> t) & 1, val = t == 63 ? 0 : e >> (t + 1);
  auto col = [&](int c) -> u64& { return trace[(size_t)(sf + c) * n + row]; };
  col(0) = r == 127; col(1) = a; col(2) = b; col(3) = bit * b; col(4) = bit; col(5) = val;
}

// inv[i] = 1/i in Goldilocks for i = 1..n-1 (inv[0] = 0).
__global__ void small_inverse_kernel(u64* __restrict__ inv, size_t n) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  inv[i] = i == 0 ? 0 : f_inv(F(i)).v;
}

// periodic pulse (pulse.rs:100-144) + io-pulse counter, and the lookup table column (range_check.rs:20-47).
__global__ void periodic_kernel(const u64* __restrict__ inv, size_t n, int start_periodic, int start_io_pulses, int start_lookups, u64 table_max, u64* __restrict__ trace) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 c = (i + 1) & 63;
  if (start_periodic >= 0) {  // the u64 table has no rotation pulse
    trace[(size_t)start_periodic * n + i] = c;
    trace[(size_t)(start_periodic + 1) * n + i] = c == 63 ? 0 : (-F(inv[63 - c])).v;
  }
  trace[(size_t)start_io_pulses * n + i] = i;
  trace[(size_t)start_lookups * n + i] = i < table_max ? i : table_max;  // 0..table_max then table_max repeated
}
// io pulses (pulse.rs:20-43): pulse q sits at row pos(q) = rpb*(q/2) + (q odd ? rpb-1 : 0); witness = 1/(i - pos).
__global__ void io_pulse_kernel(const u64* __restrict__ inv, size_t n, size_t rpb, int first_col, u64* __restrict__ trace) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int q = blockIdx.y;
  const size_t pos = (size_t)(q >> 1) * rpb + ((q & 1) ? rpb - 1 : 0);
  u64* w = trace + (size_t)(first_col + 2 * q) * n;  // witness_col(q); pulse_col(q) = witness_col(q) + 1
  w[i] = i > pos ? inv[i - pos] : (i < pos ? (-F(inv[pos - i])).v : 0);
  w[n + i] = i == pos;
}
// Reads back what the two kernels above write: `block` = the gridDim.y columns [periodic counter, periodic witness (has_periodic
// only)], io counter, (witness, pulse) of every io pulse, table column, n rows each; *mismatch becomes 1 unless every word is the
// generators' word.  A valid witness may differ (a pulse witness at its own pulse row is unconstrained; the generators write 0),
// so this is a comparison of words, not a constraint check.  No inverse table: a canonical w is 1/d exactly when w * d = 1.
__global__ void fixed_columns_check_kernel(const u64* __restrict__ block, size_t n, int has_periodic, size_t rpb, u64 table_max, unsigned long long* __restrict__ mismatch) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  int j = blockIdx.y;
  const u64 w = block[(size_t)j * n + i];
  auto inverse_of = [&](F d) { return w < GLP && (F(w) * d).v == 1; };   // d != 0
  const u64 c = (i + 1) & 63;
  bool ok;
  if (j + 1 == (int)gridDim.y) ok = w == (i < table_max ? i : table_max);
  else if (has_periodic && j == 0) ok = w == c;
  else if (has_periodic && j == 1) ok = c == 63 ? w == 0 : inverse_of(-F(63 - c));
  else {
    j -= has_periodic ? 3 : 1;   // -1: the io counter; then witness_col(q) = 2 q, pulse_col(q) = 2 q + 1
    if (j < 0) ok = w == i;
    else {
      const size_t q = (size_t)(j >> 1), pos = (q >> 1) * rpb + ((q & 1) ? rpb - 1 : 0);   // (io_pulse_kernel)
      if (j & 1) ok = w == (i == pos ? 1u : 0u);
      else ok = i == pos ? w == 0 : inverse_of(i > pos ? F(i - pos) : -F(pos - i));
    }
  }
  if (!ok) *mismatch = 1;
}

// ---- Fq12ExpStark rows (src/fields/fq12/exp.rs:229-319) -----------------------------------------------------------------
// One lane per row.  ca / cb: the square-and-multiply chains of every instance in standard form, [K][257][12][4]
// (A[t] = x^(2^t), B[t]); row r of instance k: a = A[r>>1]; even rows: b = B[r>>1], multiply when the bit is set
// (product B[(r>>1)+1]); odd rows: b = B[(r>>1)+1], square (product A[(r>>1)+1]).  Writes the 384 limb columns of
// a and b and the 1344 Fq12Output columns (mul.rs:217-231) straight into the column-major trace.
// Fq12ExpU64Stark (fq12_u64/exp_u64.rs) is the same with 128 rows per instance: log_rpb = 7, iow = 194, 65 chain entries.
__global__ void __launch_bounds__(64) fq12_row_kernel(const uint32_t* __restrict__ ios, size_t iow, int log_rpb, const u64* __restrict__ ca, const u64* __restrict__ cb,
                                                      size_t n, u64* __restrict__ trace, int* __restrict__ err) {
  const size_t row = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (row >= n) return;
  const size_t k = row >> log_rpb, cl = ((size_t)1 << (log_rpb - 1)) + 1;  // chain entries per instance
  const int r = (int)(row & (((size_t)1 << log_rpb) - 1)), t = r >> 1; const bool sq = r & 1;
  const bool bit = (ios[iow * k + 192 + (t >> 5)] >> (t & 31)) & 1;
  const int op = sq ? 1 : (bit ? 2 : 0);  // 1 square, 2 multiply
  const u64 (*a)[4] = reinterpret_cast<const u64 (*)[4]>(ca + ((k * cl + t) * 12) * 4);
  const u64 (*b)[4] = reinterpret_cast<const u64 (*)[4]>(cb + ((k * cl + t + (sq ? 1 : 0)) * 12) * 4);
  for (int c = 0; c < 12; c++)
    for (int i = 0; i < 16; i++) {
      trace[(size_t)(16 * c + i) * n + row] = (a[c][i >> 2] >> (16 * (i & 3))) & 0xffff;
      trace[(size_t)(192 + 16 * c + i) * n + row] = (b[c][i >> 2] >> (16 * (i & 3))) & 0xffff;
    }
  u64* g = trace + (size_t)384 * n + row;
  if (op) {
    const u64 (*prod)[4] = reinterpret_cast<const u64 (*)[4]>((op == 1 ? ca : cb) + ((k * cl + t + 1) * 12) * 4);
    if (!fq12_output_row(a, op == 1 ? a : b, prod, [&](int i, u64 v) { g[(size_t)i * n] = v; })) atomicOr(err, TG_ERR_WITNESS);
  } else {  // Fq12Output::default (mul.rs:179-187)
    for (int i = 0; i < 1332; i++) g[(size_t)i * n] = 0;
    for (int i = 1332; i < 1344; i++) g[(size_t)i * n] = 1;
  }
}

// ---- the square-and-multiply chains of Fq12ExpStark on the device (round 3) ------------------------------------------------------
// A[t] = x^(2^t), B[0] = offset, B[t+1] = bit_t ? A[t] B[t] : B[t] (fq12/exp.rs:165-221): 2 x 256 DEPENDENT Fq12 products per
// instance.  A lane would take ~0.2 s for them and the host pool 1 ms per instance and core (32 ms for 512 instances on a 16-CPU
// share); but one Fq12 product is 144 independent Fq products, so ONE WORKGROUP walks the chain of one instance: lanes 0..143 form
// a_i a_j, lanes 144..287 a_i b_j (Montgomery, eight 32-bit limbs), the products meet in LDS, and 24 lanes fold them into the 12 + 12
// new coefficients (flat basis, w^6 = 9 + i, exactly fq12_mul_m's sums: field arithmetic is exact, so the standard forms written
// to ca / cb are the host's words).  512 instances = 512 workgroups side by side.
__device__ __forceinline__ Fq fq12_fold_coeff(const Fq* P, int c) {   // coefficient c of the product from P[i * 12 + j] = x_i y_j
  const int m = c < 6 ? c : c - 6;
  const bool re = c < 6;
  const Fq z = {{0, 0, 0, 0}};
  Fq lo = z, hd = z, hs = z;     // d[m] (or s[m]),  d[m+6],  s[m+6]
  for (int i = 0; i < 6; i++) {
    const int jl = m - i, jh = m + 6 - i;
    if (jl >= 0) {
      if (re) lo = fadd(lo, fsub(P[i * 12 + jl], P[(i + 6) * 12 + jl + 6]));
      else lo = fadd(lo, fadd(P[i * 12 + jl + 6], P[(i + 6) * 12 + jl]));
    }
    if (jh >= 0 && jh <= 5) {
      hd = fadd(hd, fsub(P[i * 12 + jh], P[(i + 6) * 12 + jh + 6]));
      hs = fadd(hs, fadd(P[i * 12 + jh + 6], P[(i + 6) * 12 + jh]));
    }
  }
  if (m == 5) return lo;
  const Fq& nine = re ? hd : hs;
  Fq t = fadd(nine, nine); t = fadd(t, t); t = fadd(t, t); t = fadd(t, nine);     // 9 x
  return re ? fsub(fadd(lo, t), hs) : fadd(fadd(lo, hd), t);
}
__global__ void __launch_bounds__(320) fq12_chain_kernel(const uint32_t* __restrict__ ios, size_t iow, int steps, u64* __restrict__ ca, u64* __restrict__ cb,
                                                         u64* __restrict__ outs) {   // outs: [K][12][4], B[steps] again, compact (the public inputs' outputs)
  __shared__ Fq A[12], B[12], PA[144], PB[144];
  const size_t k = blockIdx.x;
  const uint32_t* io = ios + iow * k;
  const int tid = threadIdx.x, c = tid % 12;
  const bool is_a = tid < 12, is_b = tid >= 12 && tid < 24;
  if (is_a || is_b) {
    u64 t4[4]; u32x8_to_u64x4(io + (is_a ? 0 : 96) + 8 * c, t4);
    (is_a ? A : B)[c] = to_m(t4);
  }
  __syncthreads();
  for (int t = 0;; t++) {
    if (is_a || is_b) from_m((is_a ? A : B)[c], (is_a ? ca : cb) + ((k * (size_t)(steps + 1) + t) * 12 + c) * 4);
    if (t == steps) { if (is_b) from_m(B[c], outs + (k * 12 + c) * 4); break; }
    const bool bit = (io[192 + (t >> 5)] >> (t & 31)) & 1;          // uniform over the workgroup
    if (tid < 144) PA[tid] = mmul(A[tid / 12], A[tid % 12]);
    else if (tid < 288 && bit) PB[tid - 144] = mmul(A[(tid - 144) / 12], B[(tid - 144) % 12]);
    __syncthreads();
    Fq nv;
    if (is_a) nv = fq12_fold_coeff(PA, c);
    else if (is_b && bit) nv = fq12_fold_coeff(PB, c);
    __syncthreads();                                                   // every product has been read, A / B may change
    if (is_a) A[c] = nv; else if (is_b && bit) B[c] = nv;
    __syncthreads();
  }
}

// The same rows with one lane per (row, output coefficient) -- round 3.  fq12_row_kernel keeps 22 limb polynomials of 31 signed
// 64-bit coefficients per lane (d[11], s[11] of fq12_output_row: 5.4 KB) next to the operand limbs: 9.8 KB of scratch per lane and
// 420 VGPRs, every limb product a round trip through scratch memory (44 ms for the 2^18 rows of Fq12ExpStark(512)).  Coefficient c
// of x*y needs only  d[m] + 9 d[m+6] - s[m+6]  (c < 6, m = c)  or  s[m] + d[m+6] + 9 s[m+6]  (c >= 6, m = c - 6)  with
// d[q] = sum_{i+j=q} x_i y_j - x_{i+6} y_{j+6},  s[q] = sum_{i+j=q} x_i y_{j+6} + x_{i+6} y_j  (mul.rs:24-87, w^6 = 9 + i): a lane
// accumulates those (at most 22) weighted limb products straight into ONE polynomial of 31 coefficients held in registers, runs
// mod_witness on it and writes the 16 + 95 + 1 columns of its coefficient plus the limb columns of a[c] and b[c].  1.4 x the limb
// products of the shared form (d[m+6], s[m+6] are formed by two lanes), 12 x the lanes, no scratch arrays for the products.  Lanes
// of a wave share c (lane index = c * n + row): no divergence, coalesced stores.
__device__ __forceinline__ void conv16_acc(const u64* __restrict__ x4, const u64* __restrict__ y4, int w, int64_t* t) {
  int xl[16], yl[16];
#pragma unroll
  for (int i = 0; i < 16; i++) { xl[i] = (int)((x4[i >> 2] >> (16 * (i & 3))) & 0xffff); yl[i] = w * (int)((y4[i >> 2] >> (16 * (i & 3))) & 0xffff); }
#pragma unroll
  for (int i = 0; i < 16; i++)
#pragma unroll
    for (int j = 0; j < 16; j++) t[i + j] += (int64_t)xl[i] * (int64_t)yl[j];
}
__global__ void __launch_bounds__(256) fq12_gadget_kernel(const uint32_t* __restrict__ ios, size_t iow, int log_rpb, const u64* __restrict__ ca,
                                                          const u64* __restrict__ cb, size_t n, u64* __restrict__ trace, int* __restrict__ err) {
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (tid >= 12 * n) return;
  const size_t row = tid % n;
  const int c = (int)(tid / n);
  const size_t k = row >> log_rpb, cl = ((size_t)1 << (log_rpb - 1)) + 1;  // chain entries per instance
  const int r = (int)(row & (((size_t)1 << log_rpb) - 1)), t = r >> 1; const bool sq = r & 1;
  const bool bit = (ios[iow * k + 192 + (t >> 5)] >> (t & 31)) & 1;
  const int op = sq ? 1 : (bit ? 2 : 0);  // 1 square, 2 multiply
  const u64* a = ca + ((k * cl + t) * 12) * 4;                       // [12][4]
  const u64* b = cb + ((k * cl + t + (sq ? 1 : 0)) * 12) * 4;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    trace[(size_t)(16 * c + i) * n + row] = (a[4 * c + (i >> 2)] >> (16 * (i & 3))) & 0xffff;
    trace[(size_t)(192 + 16 * c + i) * n + row] = (b[4 * c + (i >> 2)] >> (16 * (i & 3))) & 0xffff;
  }
  u64* g = trace + (size_t)384 * n + row;
  auto put = [&](int i, u64 v) { g[(size_t)i * n] = v; };
  if (!op) {  // Fq12Output::default (mul.rs:179-187): zeros, quotient signs 1
    for (int i = 0; i < 16; i++) put(16 * c + i, 0);
    for (int i = 0; i < 95; i++) put(192 + 95 * c + i, 0);
    put(1332 + c, 1);
    return;
  }
  const u64* x = a;
  const u64* y = op == 1 ? a : b;
  const u64* out = (op == 1 ? ca : cb) + ((k * cl + t + 1) * 12 + c) * 4;
  const int m = c < 6 ? c : c - 6;
  const bool re = c < 6;
  int64_t pol[31];
#pragma unroll
  for (int q = 0; q < 31; q++) pol[q] = 0;
#pragma unroll 1
  for (int i = 0; i < 6; i++) {
    const int jl = m - i, jh = m + 6 - i;          // i + j = m (weights of d[m] / s[m]) and i + j = m + 6 (of d[m+6], s[m+6])
    if (jl >= 0) {
      if (re) { conv16_acc(x + 4 * i, y + 4 * jl, 1, pol); conv16_acc(x + 4 * (i + 6), y + 4 * (jl + 6), -1, pol); }
      else { conv16_acc(x + 4 * i, y + 4 * (jl + 6), 1, pol); conv16_acc(x + 4 * (i + 6), y + 4 * jl, 1, pol); }
    }
    if (jh >= 0 && jh <= 5) {
      const int wd = re ? 9 : 1, ws = re ? -1 : 9;
      conv16_acc(x + 4 * i, y + 4 * jh, wd, pol); conv16_acc(x + 4 * (i + 6), y + 4 * (jh + 6), -wd, pol);
      conv16_acc(x + 4 * i, y + 4 * (jh + 6), ws, pol); conv16_acc(x + 4 * (i + 6), y + 4 * jh, ws, pol);
    }
  }
  ModW w;
  if (!mod_witness(pol, out, true, w)) { atomicOr(err, TG_ERR_WITNESS); return; }
#pragma unroll
  for (int i = 0; i < 16; i++) put(16 * c + i, (out[i >> 2] >> (16 * (i & 3))) & 0xffff);
  int cur = 192 + 95 * c;
  for (int i = 0; i < 16; i++) put(cur++, (u64)w.out_aux_red[i]);
  for (int i = 0; i < 17; i++) put(cur++, (u64)w.quot_abs[i]);
  for (int i = 0; i < 31; i++) put(cur++, (u64)w.aux_lo[i]);
  for (int i = 0; i < 31; i++) put(cur++, (u64)w.aux_hi[i]);
  put(1332 + c, w.sign > 0 ? (u64)1 : GLP - 1);
}

// ---- FqExpStark rows (src/fields/fq/exp.rs:128-176): as fq12_row_kernel with one coefficient; ca / cb: [K][257][4] ---------
__global__ void __launch_bounds__(128) fq_row_kernel(const uint32_t* __restrict__ ios, const u64* __restrict__ ca, const u64* __restrict__ cb, size_t n,
                                                     u64* __restrict__ trace, int* __restrict__ err) {
  const size_t row = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (row >= n) return;
  const size_t k = row >> 9; const int r = (int)(row & 511), t = r >> 1; const bool sq = r & 1;
  const bool bit = (ios[24 * k + 16 + (t >> 5)] >> (t & 31)) & 1;
  const int op = sq ? 1 : (bit ? 2 : 0);  // 1 square, 2 multiply
  u64 a[4], b[4], prod[4];
  for (int i = 0; i < 4; i++) { a[i] = ca[(k * 257 + t) * 4 + i]; b[i] = cb[(k * 257 + t + (sq ? 1 : 0)) * 4 + i]; }
  for (int i = 0; i < 16; i++) {
    trace[(size_t)i * n + row] = (a[i >> 2] >> (16 * (i & 3))) & 0xffff;
    trace[(size_t)(16 + i) * n + row] = (b[i >> 2] >> (16 * (i & 3))) & 0xffff;
  }
  u64* g = trace + (size_t)32 * n + row;
  if (op) {
    for (int i = 0; i < 4; i++) prod[i] = (op == 1 ? ca : cb)[(k * 257 + t + 1) * 4 + i];
    u64 lv[112];
    if (!fq_output_row(a, op == 1 ? a : b, prod, lv)) { atomicOr(err, TG_ERR_WITNESS); return; }
    for (int c = 0; c < 112; c++) g[(size_t)c * n] = lv[c];
  } else {  // FqOutput::default (mul.rs:24-32)
    for (int c = 0; c < 111; c++) g[(size_t)c * n] = 0;
    g[(size_t)111 * n] = 1;
  }
}

// ---- split range check (range_check.rs:116-160): table 0..255 then 255 repeated; per target column the low and the high
// byte, each with its sorted column and permuted table (lookup.rs:60-111).  One workgroup of 256 lanes per target.
// With 256 distinct values the reference's merge is simulated value by value by one lane (push a missing value; the
// first occurrence of a present value takes its table entry, repeats pop the pool or are deferred; repeats of 255 keep
// matching the table's tail of 255s), then every sorted slot is classified independently from the per-value records.
__global__ void __launch_bounds__(256) split_range_check_kernel(u64* __restrict__ trace, size_t n, int first_target, int table_col, int* __restrict__ err) {
  __shared__ unsigned hist[2][256], tincl[256], npop[256], pbase[256], defbase[256];
  __shared__ unsigned char pool[256], poplist[256];
  __shared__ unsigned misc[8];
  const int tid = threadIdx.x, kcol = blockIdx.x;
  const u64* col = trace + (size_t)(first_target + kcol) * n;
  u64* base = trace + (size_t)(table_col + 1 + 6 * kcol) * n;  // lo, sorted lo, perm lo, hi, sorted hi, perm hi
  hist[0][tid] = 0; hist[1][tid] = 0;
  __syncthreads();
  bool bad = false;
  for (size_t i = tid; i < n; i += 256) {
    const u64 v = col[i];
    if (v >= 65536) { bad = true; continue; }
    const unsigned lo = (unsigned)v & 255, hi = (unsigned)v >> 8;
    base[i] = lo; base[3 * n + i] = hi;
    atomicAdd(&hist[0][lo], 1u); atomicAdd(&hist[1][hi], 1u);
  }
  if (bad) atomicOr(err, TG_ERR_RANGE);
  __syncthreads();
  for (int h = 0; h < 2; h++) {
    u64* sorted_out = base + (size_t)(3 * h + 1) * n;
    u64* perm_out = sorted_out + n;
    // inclusive prefix counts
    unsigned incl = hist[h][tid];
    for (int o = 1; o < 64; o <<= 1) { unsigned t = __shfl_up(incl, o, 64); if ((tid & 63) >= o) incl += t; }
    if ((tid & 63) == 63) misc[tid >> 6] = incl;
    __syncthreads();
    for (int w = 0; w < (tid >> 6); w++) incl += misc[w];
    tincl[tid] = incl;
    __syncthreads();
    if (tid == 0) {
      unsigned sp = 0, npl = 0, ndef = 0;
      for (int v = 0; v < 255; v++) {
        const unsigned c = hist[h][v];
        npop[v] = 0; pbase[v] = npl; defbase[v] = ndef;
        if (c == 0) { pool[sp++] = (unsigned char)v; continue; }
        const unsigned k = c - 1 < sp ? c - 1 : sp;
        for (unsigned j = 0; j < k; j++) poplist[npl++] = pool[--sp];
        npop[v] = k; ndef += c - 1 - k;
      }
      const unsigned c255 = hist[h][255];
      const size_t tail = n - 255;             // table entries equal to 255
      npop[255] = 0; pbase[255] = npl; defbase[255] = ndef;
      if (c255 > tail) ndef += (unsigned)(c255 - tail);
      misc[4] = sp; misc[5] = ndef;
    }
    __syncthreads();
    const unsigned sp = misc[4];
    const size_t tail = n - 255;
    for (size_t i = tid; i < n; i += 256) {
      // value of sorted slot i: first v with tincl[v] > i
      int lo = 0, hi = 255;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (tincl[mid] > i) hi = mid; else lo = mid + 1; }
      const int v = lo;
      const size_t d = i - (tincl[v] - hist[h][v]);
      unsigned out;
      if (v < 255) {
        if (d == 0) out = v;
        else if (d <= npop[v]) out = poplist[pbase[v] + d - 1];
        else { const unsigned rank = defbase[v] + (unsigned)(d - 1 - npop[v]); out = rank < sp ? pool[rank] : 255u; }
      } else {
        if (d < tail) out = 255u;
        else { const unsigned rank = defbase[255] + (unsigned)(d - tail); out = rank < sp ? pool[rank] : 255u; }
      }
      sorted_out[i] = (u64)v; perm_out[i] = (u64)out;
    }
    __syncthreads();
  }
}

// ---- u16 range check (range_check.rs:20-47, lookup.rs:60-111), n == 65536 ------------------------------------------
// One workgroup per range-checked column; everything after the histogram stays in LDS.
//
// The reference merges the sorted column against the table 0..65535 (lookup.rs:60-111): a table value missing from
// the column goes on a LIFO pool; the first occurrence of a present value takes its own table entry; every further
// occurrence pops the pool or, when the pool is empty, is deferred; deferred slots finally take the remaining pool
// bottom-up (the repeats of 65535 are always deferred: the loop has run off the table by then).  Replaying that
// serially costs a lane ~400 cycles per value, so it is restated as independent searches:
//   c[v] = multiplicity, T[v] = #entries <= v (LDS, u16; 65536 is implied for v >= max value),
//   S[v] = v + 1 - T[v]  = (#pushes - #pops) after value v, unclamped, for v <= 65534,
//   a pushed value u is popped by the first x > u with S[x] < S[u], into sorted slot x - S[u] + 1;
//   if there is no such x it is still pooled at the end, at height h = S[u] - min(0, min S), and fills the deferred
//   slot of rank h-1, which is slot v + h where v is the first value with S[v] < -(h-1) (or a repeat of 65535).
// Every lane owns 64 consecutive values; "first x >= from with S[x] < target" walks a two-level min tree (32 / 1024).
// tools/microbench/range_check_phases.hip defines SBN_RC_PROFILE: workgroup 0 then stamps the constant 100 MHz clock at the phase
// boundaries of range_check_kernel (a barrier in front of each stamp); the library never defines it.
#ifdef SBN_RC_PROFILE
__device__ unsigned long long g_rc_prof[16];
#define RC_MARK(k) do { __syncthreads(); if (blockIdx.x == 0 && threadIdx.x == 0) g_rc_prof[k] = wall_clock64(); } while (0)
#else
#define RC_MARK(k) do { } while (0)
#endif
static constexpr int RC_THREADS = 1024;
// heavy[]: values with more than HEAVY occurrences are expanded by the whole block.  HEAVY = 64, 256 for BIG (n <= 2^18) and
// n / RC_HEAVY_MAX for TALL.  INVARIANT: a column of n rows has at most floor(n / (HEAVY + 1)) values with more than HEAVY occurrences;
// that is 1,008 at n = 2^16, 1,020 at n = 2^18 and, with HEAVY = n / 1,024, at most 1,023 at any n: the list cannot overflow whatever
// the histogram is.  (A fixed cut of 256 would meet up to 2,040 such values at 2^19 rows.)
static constexpr int RC_HEAVY_MAX = 1024;
static constexpr size_t RC_LDS_BYTES = 65536 * 2 + 2 * 2048 * 4 + 64 * 4 + 64 * 4 + RC_HEAVY_MAX * 8;
// TALL (n > 2^18): the values at which T crosses a multiple of 2^16 no longer fit misc[40..42] (7 crossings at 2^19 rows, 63 at 2^22):
// thr[k - 1], k = 1..63, behind heavy[]; thr[63] stays 65536, the end mark of a walk along the thresholds
static constexpr int RC_THR_MAX = 64;
static constexpr size_t RC_TALL_LDS_BYTES = RC_LDS_BYTES + RC_THR_MAX * 4;

// Tables with MORE than 2^16 rows (G1ExpStark(256) ... : the reference pads to any power of two >= 128 instances,
// src/curves/g1/circuit.rs:273-277): multiplicities no longer fit the u16 LDS counters, so range_count_kernel builds
// the histogram of every target column in HBM (u32, one atomic per row) and the BIG variant of range_check_kernel reads
// it.  The prefix counts T[v] <= n stay in LDS as T mod 2^16 (u16) plus the <= 3 values at which T crosses a multiple
// of 2^16 (T is monotone, so the high part is the number of those thresholds <= v).
// Tables with more than 2^18 rows (G1ExpStark(1024) ...) take the TALL variant of the BIG form: up to 63 thresholds, sorted in LDS
// (thr[k - 1] = the first value at which T >= k 2^16; several k may share one value when its count carries T over more than one
// multiple), the high part of T(v) = 2^16 x the number of thresholds <= v: a binary search for a lone T(v), a cursor along the
// thresholds where consecutive values are read; and the cut of heavy[] grows with n (RC_HEAVY_MAX above).  The forms of
// 2^16 .. 2^18 rows are the instantiations <false> and <true> as before: everything TALL adds sits behind that compile-time constant.
__global__ void range_count_kernel(const u64* __restrict__ trace, size_t n, int first_col, unsigned int* __restrict__ cnt, int* __restrict__ err) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 v = trace[(size_t)(first_col + blockIdx.y) * n + i];
  if (v >= 65536) { atomicOr(err, TG_ERR_RANGE); return; }
  atomicAdd(&cnt[(size_t)blockIdx.y * 65536 + v], 1u);
}

// The table column is 0..65534 once each, then 65535 K = n - 65535 times (range_check.rs:20-47: min(i, 65535)); the merge
// gives the first min(c, K) occurrences of 65535 their own table entry (Ordering::Equal), further occurrences run off
// the table and are deferred, and table copies left over when the inputs end are appended to the pool (lookup.rs:100-101).
template <bool BIG, bool TALL = false>
__global__ void __launch_bounds__(RC_THREADS) __attribute__((amdgpu_waves_per_eu(5, 5))) range_check_kernel(u64* __restrict__ trace, size_t n, int first_col, int start_lookups, int* __restrict__ err,
                                                                 const unsigned int* __restrict__ cnt, int old_form) {
  extern __shared__ unsigned int lds[];
  unsigned int* t32 = lds;                                                  // 32768 words = 65536 u16 counters, then T (mod 2^16)
  const unsigned short* t16 = reinterpret_cast<const unsigned short*>(lds);
  int* L1 = reinterpret_cast<int*>(lds + 32768);                            // min S over 32 values
  int* SM1 = L1 + 2048;                                                     // suffix minima of L1
  int* L2 = SM1 + 2048;                                                     // min over 32 L1 entries
  unsigned int* misc = reinterpret_cast<unsigned int*>(L2 + 64);            // [0..15] wave sums, [32] differs, [33] vmax, [34] heavy count, [40..42] thresholds
  uint2* heavy = reinterpret_cast<uint2*>(misc + 64);                       // (value, start) of values with many occurrences
  [[maybe_unused]] unsigned int* thr = reinterpret_cast<unsigned int*>(heavy + RC_HEAVY_MAX);   // TALL only (RC_TALL_LDS_BYTES)
  static_assert(BIG || !TALL, "the tall form reads the HBM histogram");
  const int tid = threadIdx.x, kcol = blockIdx.x;
  const u64* col = trace + (size_t)(first_col + kcol) * n;
  u64* sorted_out = trace + (size_t)(start_lookups + 1 + 2 * kcol) * n;
  u64* perm_out = sorted_out + n;
  constexpr int INF = 0x3fffffff;
  const int N = (int)n, KT = N - 65535;             // rows; copies of 65535 in the table
  const int HEAVY = TALL ? N / RC_HEAVY_MAX : (BIG ? 256 : 64);   // (a constant unless TALL)

  RC_MARK(0);
  for (int i = tid; i < 32768; i += RC_THREADS) t32[i] = 0;
  if (tid < 64) misc[tid] = tid >= 40 && tid < 44 ? 65536u : 0u;
  if constexpr (TALL) { if (tid < RC_THR_MAX) thr[tid] = 65536u; }
  __syncthreads();
  RC_MARK(1);
  if constexpr (!BIG) {
    const u64 v0 = col[0];
    bool differs = false, bad = false; unsigned vm = 0;
    for (size_t i0 = tid; i0 < n; i0 += 8 * RC_THREADS) {   // eight loads in flight, then their eight LDS atomics
      u64 vv[8];
#pragma unroll
      for (int k = 0; k < 8; k++) { const size_t i = i0 + (size_t)k * RC_THREADS; vv[k] = i < n ? col[i] : v0; }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const u64 v = vv[k];
        if (i0 + (size_t)k * RC_THREADS >= n) continue;
        if (v >= 65536) { bad = true; continue; }
        differs |= v != v0; vm = vm > (unsigned)v ? vm : (unsigned)v;
        atomicAdd(&t32[v >> 1], 1u << (16 * (v & 1)));
      }
    }
    if (bad) atomicOr(err, TG_ERR_RANGE);
    if (differs) misc[32] = 1;
    atomicMax(&misc[33], vm);
    __syncthreads();
    // a constant column wrapped its single u16 counter (65536 occurrences): clear it, T is implied by vmax alone
    if (misc[32] == 0 && tid == 0) t32[v0 >> 1] = 0;
    __syncthreads();
  }

  RC_MARK(2);
  // counts -> inclusive prefix counts T (mod 2^16), in place
  if constexpr (!BIG) {
    uint4* p = reinterpret_cast<uint4*>(t32 + 32 * tid);
    unsigned cw[32];
    for (int j = 0; j < 8; j++) { uint4 q = p[j]; cw[4 * j] = q.x; cw[4 * j + 1] = q.y; cw[4 * j + 2] = q.z; cw[4 * j + 3] = q.w; }
    unsigned tot = 0;
    for (int j = 0; j < 32; j++) tot += (cw[j] & 0xffff) + (cw[j] >> 16);
    unsigned incl = tot;
    for (int o = 1; o < 64; o <<= 1) { unsigned t = __shfl_up(incl, o, 64); if ((tid & 63) >= o) incl += t; }
    if ((tid & 63) == 63) misc[tid >> 6] = incl;
    __syncthreads();
    unsigned run = incl - tot;
    for (int w = 0; w < (tid >> 6); w++) run += misc[w];
    for (int j = 0; j < 32; j++) { unsigned lo = run + (cw[j] & 0xffff), hi = lo + (cw[j] >> 16); run = hi; cw[j] = (lo & 0xffff) | (hi << 16); }
    for (int j = 0; j < 8; j++) p[j] = make_uint4(cw[4 * j], cw[4 * j + 1], cw[4 * j + 2], cw[4 * j + 3]);
  } else {
    // this lane's 64 values: counts from the HBM histogram (twice: total first, then the running prefix)
    const unsigned int* cg = cnt + (size_t)kcol * 65536 + 64 * tid;
    unsigned tot = 0, vm = 0;
    for (int j = 0; j < 64; j++) { const unsigned c = cg[j]; tot += c; if (c) vm = (unsigned)(64 * tid + j); }
    atomicMax(&misc[33], vm);
    unsigned incl = tot;
    for (int o = 1; o < 64; o <<= 1) { unsigned t = __shfl_up(incl, o, 64); if ((tid & 63) >= o) incl += t; }
    if ((tid & 63) == 63) misc[tid >> 6] = incl;
    __syncthreads();
    unsigned run = incl - tot;
    for (int w = 0; w < (tid >> 6); w++) run += misc[w];
    for (int j = 0; j < 32; j++) {
      const unsigned before = run;
      const unsigned lo = run + cg[2 * j], hi = lo + cg[2 * j + 1];
      run = hi;
      t32[32 * tid + j] = (lo & 0xffff) | (hi << 16);
      // thresholds: the first value at which T reaches k * 2^16 (k = 1..3)
      if constexpr (!TALL) {
        for (unsigned k = (before >> 16) + 1; k <= (lo >> 16) && k < 4; k++) atomicMin(&misc[39 + k], (unsigned)(64 * tid + 2 * j));
        for (unsigned k = (lo >> 16) + 1; k <= (hi >> 16) && k < 4; k++) atomicMin(&misc[39 + k], (unsigned)(64 * tid + 2 * j + 1));
      } else {   // k = 1..63: every k is reached at exactly one value, so one lane stores it (T = n = 64 x 2^16 only at vmax, where T is n by rule)
        for (unsigned k = (before >> 16) + 1; k <= (lo >> 16) && k < RC_THR_MAX; k++) thr[k - 1] = (unsigned)(64 * tid + 2 * j);
        for (unsigned k = (lo >> 16) + 1; k <= (hi >> 16) && k < RC_THR_MAX; k++) thr[k - 1] = (unsigned)(64 * tid + 2 * j + 1);
      }
    }
  }
  __syncthreads();
  RC_MARK(3);
  const int vmax = (int)misc[33];
  const int thr1 = (int)misc[40], thr2 = (int)misc[41], thr3 = (int)misc[42];
  auto Thi = [&](int v) __attribute__((always_inline)) -> int {
    if constexpr (TALL) {   // the number of thresholds <= v: thr[0..62] ascend, never-reached ones are 65536 > v
      int c = 0;
      for (int s = RC_THR_MAX / 2; s; s >>= 1) if ((int)thr[c + s - 1] <= v) c += s;
      return c << 16;
    } else return BIG ? ((v >= thr1) + (v >= thr2) + (v >= thr3)) << 16 : 0;
  };
  // TALL, consecutive values: `hic` thresholds are <= the last value asked for, `nx` is the next one (thr[63] = 65536 ends the walk)
  auto Thi_next = [&](int v, int& hic, int& nx) __attribute__((always_inline)) -> int {
    while (nx <= v) { hic++; nx = (int)thr[hic]; }
    return hic << 16;
  };
  auto T = [&](int v) __attribute__((always_inline)) -> int { return v < 0 ? 0 : (v >= vmax ? N : (int)t16[v] + Thi(v)); };
  auto S = [&](int v) __attribute__((always_inline)) -> int { return v >= 65535 ? INF : v + 1 - T(v); };
  unsigned long long pool = 0;   // two-pass form: the unused table values of this lane's segment that nothing inside the segment took
  int s_end = 0;                 // pool height after the segment's last value below 65535
  if (old_form) {
    for (int b = 0; b < 2; b++) {
      int m = INF;
      for (int j = 0; j < 32; j++) { int s = S(tid * 64 + b * 32 + j); m = s < m ? s : m; }
      L1[2 * tid + b] = m;
    }
  } else {
    // Lane l owns the values 64 l .. 64 l + 63: their 64 prefix counts come out of LDS once (eight 128-bit reads) and serve both the
    // two minima of the search tree and the LIFO pool INSIDE the segment, which is a bit mask: an absent value sets its bit (push), the
    // k-th repeat of a present value takes the highest set bit (pop: slot tprev + k, the same slot the search x - S(u) + 1 of the
    // one-pass form finds, since S(u) = S(x - 1) - k + 1 for the k-th pop at x).  What is still set at the end goes through the
    // search tree below; the one-pass form searched for EVERY absent value, a wave waiting for the longest of its 64 searches in
    // every iteration (2.2e8 wave-instructions per launch, as many as a sponge launch: profiles/r3_v10_pmc_summary.json).
    const uint4* p = reinterpret_cast<const uint4*>(t32 + 32 * tid);
    unsigned cw[32];
#pragma unroll
    for (int j = 0; j < 8; j++) { const uint4 q = p[j]; cw[4 * j] = q.x; cw[4 * j + 1] = q.y; cw[4 * j + 2] = q.z; cw[4 * j + 3] = q.w; }
    int tprev = T(tid * 64 - 1), m0 = INF, m1 = INF;
    [[maybe_unused]] int hic = 0, nx = 0;
    if constexpr (TALL) { hic = Thi(tid * 64 - 1) >> 16; nx = (int)thr[hic]; }
#pragma unroll
    for (int j = 0; j < 64; j++) {
      const int v = tid * 64 + j;
      const int tv = v >= vmax ? N : (int)((cw[j >> 1] >> (16 * (j & 1))) & 0xffff) + (TALL ? Thi_next(v, hic, nx) : Thi(v));
      if (v < 65535) {
        const int sv = v + 1 - tv;
        if (j < 32) m0 = sv < m0 ? sv : m0; else m1 = sv < m1 ? sv : m1;
        s_end = sv;
        const int c = tv - tprev;
        if (c == 0) pool |= 1ull << j;
        else
          for (int k = 1; k < c && pool; k++) {
            const int u = 63 - __builtin_clzll(pool);
            pool &= ~(1ull << u);
            perm_out[tprev + k] = (u64)(tid * 64 + u);
          }
      }
      tprev = tv;
    }
    L1[2 * tid] = m0; L1[2 * tid + 1] = m1;
  }
  __syncthreads();
  if (tid < 64) { int m = INF; for (int j = 0; j < 32; j++) { int s = L1[tid * 32 + j]; m = s < m ? s : m; } L2[tid] = m; }
  __syncthreads();
  int mfin = 0;
  for (int j = 0; j < 64; j++) { int s = L2[j]; mfin = s < mfin ? s : mfin; }

  // suffix minima of L1: SM1[b] = min L1[b..2047] (lets a push that is never popped stop after its own 32-block)
  if (tid < 64) {
    int m = INF;
    for (int g = tid + 1; g < 64; g++) { int s = L2[g]; m = s < m ? s : m; }
    for (int j = 31; j >= 0; j--) { int s = L1[tid * 32 + j]; m = s < m ? s : m; SM1[tid * 32 + j] = m; }
  }
  __syncthreads();

  RC_MARK(4);
  // first x in [from, from | 31] with S(x) < target, or -1 (8 prefix counts per LDS read)
  auto scan32 = [&](int from, int target) __attribute__((always_inline)) -> int {
    const int hi = from | 31;
    [[maybe_unused]] int hic = 0, nx = 0;
    if constexpr (TALL) { hic = Thi((from & ~7) - 1) >> 16; nx = (int)thr[hic]; }
    for (int a = from & ~7; a <= hi; a += 8) {
      const uint4 q = *reinterpret_cast<const uint4*>(t16 + a);
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
      for (int e = 0; e < 8; e++) {
        const int x = a + e;
        const int tv = x >= vmax ? N : (int)((w[e >> 1] >> (16 * (e & 1))) & 0xffff) + (TALL ? Thi_next(x, hic, nx) : Thi(x));
        const int sx = x >= 65535 ? INF : x + 1 - tv;
        if (x >= from && sx < target) return x;
      }
    }
    return -1;
  };
  // first index in [from, hi] with arr[index] < target, or -1 (arr 16-byte aligned, hi + 1 a multiple of 4)
  auto scan_min = [&](const int* arr, int from, int hi, int target) __attribute__((always_inline)) -> int {
    for (int a = from & ~3; a <= hi; a += 4) {
      const int4 q = *reinterpret_cast<const int4*>(arr + a);
      if (a >= from && q.x < target) return a;
      if (a + 1 >= from && q.y < target) return a + 1;
      if (a + 2 >= from && q.z < target) return a + 2;
      if (a + 3 >= from && q.w < target) return a + 3;
    }
    return -1;
  };
  // first x in [from, 65534] with S(x) < target, or -1.  (Measured and dropped, round 4: issuing every level's LDS reads together
  // and scanning registers -- 0.48 -> 0.65 ms per launch in tools/microbench/range_check_phases.hip: with 16 waves per CU the walk
  // is bound by the instructions of its longest searches, not by LDS latency.)
  auto firstbelow = [&](int from, int target) __attribute__((always_inline)) -> int {
    if (from > 65534) return -1;
    const int x = scan32(from, target);
    if (x >= 0) return x;
    const int b = (from >> 5) + 1;
    if (b >= 2048 || SM1[b] >= target) return -1;
    int fb = scan_min(L1, b, b | 31, target);
    if (fb < 0) { const int fg = scan_min(L2, (b >> 5) + 1, 63, target); fb = scan_min(L1, fg * 32, fg * 32 + 31, target); }
    return scan32(fb * 32, target);
  };
  const int t_last = T(65534);  // = start of the 65535 run
  // deferred slot of rank `rank`: the first -mfin of them are repeats met with an empty pool below 65535, the rest are the
  // occurrences of 65535 beyond the table's KT copies (slots t_last + KT ...)
  auto assign_deferred = [&](int rank, int val) __attribute__((always_inline)) {
    int slot;
    if (rank < -mfin) { const int v = firstbelow(0, -rank); slot = v + rank + 1; }
    else slot = t_last + KT + (rank + mfin);
    perm_out[slot] = (u64)val;
  };

  if (old_form) {   // round 3 (SBN_RANGE_CHECK=1, A/B): one pass, lane l owns the values 64 l .. 64 l + 63, every unused table value searches its slot
    int tprev = T(tid * 64 - 1);
    for (int j = 0; j < 64; j++) {
      const int v = tid * 64 + j;
      if (v == 65535) break;                           // handled by the whole block below
      const int tv = T(v), c = tv - tprev;
      if (c > 0) {
        perm_out[tprev] = (u64)v;  // first occurrence takes its own table entry
        if (c <= HEAVY) { for (int d = 0; d < c; d++) sorted_out[tprev + d] = (u64)v; }
        else { const unsigned h = atomicAdd(&misc[34], 1u); heavy[h] = make_uint2((unsigned)v, (unsigned)tprev); }
      } else {
        const int s = v + 1 - tv;
        const int x = firstbelow(v + 1, s);
        if (x >= 0) perm_out[x - s + 1] = (u64)v;
        else assign_deferred(s - mfin - 1, v);
      }
      tprev = tv;
    }
  } else {
    // The pushes left in the segment's pool, top first: their levels are s_end, s_end - 1, ... (nothing after a left-over push
    // drops below it inside the segment), so ONE forward walk serves them all -- the search for level s - 1 continues at the
    // value that popped level s -- and it starts at the next segment.  Once a level is never undercut, neither are the lower ones:
    // those pushes stay in the pool to the end and fill the deferred slots.
    {
      int from = tid * 64 + 64, s = s_end;
      while (pool) {
        const int u = 63 - __builtin_clzll(pool);
        const int x = firstbelow(from, s);
        if (x < 0) break;
        pool &= ~(1ull << u);
        perm_out[x - s + 1] = (u64)(tid * 64 + u);
        from = x; s--;
      }
      // never popped: BOTTOM first -- ranks ascend, so the value at which the pool first runs `rank + 1` short (the deferred slot of
      // that rank sits right behind it) moves forward too, and this walk also continues where the last one ended
      if (pool) {
        int lvl = s - __builtin_popcountll(pool) + 1, dfrom = 0;
        while (pool) {
          const int u = __builtin_ctzll(pool);
          pool &= pool - 1;
          const int rank = lvl - mfin - 1;
          int slot;
          if (rank < -mfin) { const int vv = firstbelow(dfrom, -rank); slot = vv + rank + 1; dfrom = vv; }
          else slot = t_last + KT + (rank + mfin);
          perm_out[slot] = (u64)(tid * 64 + u);
          lvl++;
        }
      }
    }
    RC_MARK(5);
    // Lane l <-> values l, l + 1024, ...: neighbouring lanes write neighbouring slots (the one-pass form stored with a stride of
    // ~512 bytes between lanes: 3.2 x the algorithmic write traffic).  The sorted copy and the table entry of every first occurrence.
    for (int j = 0; j < 64; j++) {
      const int v = j * RC_THREADS + tid;
      if (v == 65535) break;                           // handled by the whole block below
      const int tp = T(v - 1), c = T(v) - tp;
      if (c > 0) {
        perm_out[tp] = (u64)v;
        if (c <= HEAVY) { for (int d = 0; d < c; d++) sorted_out[tp + d] = (u64)v; }
        else { const unsigned h = atomicAdd(&misc[34], 1u); heavy[h] = make_uint2((unsigned)v, (unsigned)tp); }
      }
    }
    RC_MARK(6);
  }
  __syncthreads();
  RC_MARK(7);
  const unsigned nheavy = misc[34];
  for (unsigned h = 0; h < nheavy; h++) {
    const int v = (int)heavy[h].x, st = (int)heavy[h].y, c = T(v) - st;
    for (int d = tid; d < c; d += RC_THREADS) sorted_out[st + d] = (u64)v;
  }
  // the run of 65535: c65 occurrences against KT table copies
  {
    const int c65 = N - t_last, eq = c65 < KT ? c65 : KT;
    for (int d = tid; d < c65; d += RC_THREADS) sorted_out[t_last + d] = 65535;
    for (int d = tid; d < eq; d += RC_THREADS) perm_out[t_last + d] = 65535;
    const int pooled = S(65534) - mfin;              // pool height after the values below 65535 = rank of the first left-over 65535
    for (int r = tid; r < KT - c65; r += RC_THREADS) assign_deferred(pooled + r, 65535);
  }
  RC_MARK(8);
}

// ---- chained instance lists (sbn_prover_generate_trace_chained): offset[0] = start, offset[k+1] = output[k] ------------------------
// The offsets of the reference's *_msm call shape (src/curves/g1/circuit.rs:459-509) built on the device.  The A chain of an
// instance (2^t x, or x^(2^t)) does not depend on its offset, so the existing chain kernel runs once on a list whose offsets are all
// `start` (curves) or one (Fq12) and leaves, per instance, the 256 Jacobian points 2^t x in ja (its B chain and its degenerate
// flags mean nothing there and are dropped), or x^e in the kernel's compact outputs.  Then
//   chain_prefix_kernel  I[t] = the sum of the A[s], s <= t, whose bit is set: one workgroup per instance, a Hillis-Steele scan of its
//                        256 steps in LDS (48 KB for G2); I[255] = e_k x_k;
//   chain_scan_kernel    ONE workgroup: Hillis-Steele prefix sums of (start, e_0 x_0, e_1 x_1, ...) over K <= 512 lanes, ping-pong
//                        in global scratch (a Jacobian G2 point is 192 bytes: two copies of 512 do not fit the default LDS), then one
//                        batch of TG_INV_BATCH Z's per lane for the affine form, written as u32 limbs into the offset words of ios;
//   fq12_offset_scan_kernel  the same running product in Fq12: K - 1 DEPENDENT products, each spread over 144 lanes as in
//                        fq12_chain_kernel (a product per lane would be 144 sequential Fq products per level); fq12_rebase_kernel
//                        then turns the chain of the preliminary list into the chain of the true one, so Fq12 walks its chain once.
//   chain_rebase_kernel  the B chain of the true list without a second walk: B[t] = offset_k + I[t-1], K x 257 independent additions.
// Every addition is bnw::jac_add_complete: a term may be the identity, two partial sums may be equal or opposite, and none of that
// is a property of the explicit list.  The rebased B chain holds other Jacobian representatives than exp_chains would, but
// affine_lambda_kernel turns every point into its affine form, which is unique, and judges the table's own walk there: a set bit
// with B[t] = +-A[t] is a zero slope denominator, B[t] at infinity a zero Z, both TG_ERR_DEGENERATE as on the explicit list.
// Sums in a group do not depend on the bracketing, so the offsets equal sbn_chain_instances' word for word.
template <int E> __device__ __forceinline__ Jac<E> ld_jac(const u64* p) { Jac<E> r; r.X = ldc<E>(p); r.Y = ldc<E>(p + 4 * E); r.Z = ldc<E>(p + 8 * E); return r; }
template <int E> __device__ __forceinline__ void st_jac(u64* p, const Jac<E>& v) { stc<E>(p, v.X); stc<E>(p + 4 * E, v.Y); stc<E>(p + 8 * E, v.Z); }
// Out of Jacobian and Montgomery form, for every kernel that leaves an affine point in u32 words (the word order of a point in `ios`):
//   affine_or_zero   x, y of p from ni = 1 / norm(Z) (batch_inverse, finv_fermat); the point at infinity has none: zeros, true;
//   st_affine_words  x then y, E coordinates of eight standard-form u32 words each, to dst[0 .. 16E);
//   ld_affine_words  the way back: x, y of the affine point in the 16E u32 words at w, Montgomery form.
template <int E> __device__ __forceinline__ bool affine_or_zero(const Jac<E>& p, const Fq& ni, Co<E> (&v)[2]) {
  if (czero<E>(p.Z)) { v[0] = p.Z; v[1] = p.Z; return true; }
  const Co<E> zi = cinv_from_norm(p.Z, ni), zi2 = cmul(zi, zi);
  v[0] = cmul(p.X, zi2); v[1] = cmul(p.Y, cmul(zi2, zi));
  return false;
}
template <int E> __device__ __forceinline__ void ld_affine_words(const uint32_t* w, Co<E>& X, Co<E>& Y) {
  u64 t4[4];
  for (int q = 0; q < E; q++) { u32x8_to_u64x4(w + 8 * q, t4); X.c[q] = to_m(t4); u32x8_to_u64x4(w + 8 * (E + q), t4); Y.c[q] = to_m(t4); }
}
template <int E> __device__ __forceinline__ void st_affine_words(uint32_t* dst, const Co<E> (&v)[2]) {
  for (int c = 0; c < 2; c++)
    for (int q = 0; q < E; q++) {
      u64 s[4]; from_m(v[c].c[q], s);
      for (int w = 0; w < 8; w++) dst[8 * (c * E + q) + w] = (uint32_t)(s[w >> 1] >> (32 * (w & 1)));
    }
}
static constexpr int CT_LANES = 256;   // one lane per step of an instance
template <int E>
__global__ void __launch_bounds__(CT_LANES) chain_prefix_kernel(const uint32_t* __restrict__ ios, size_t K, const u64* __restrict__ ja, u64* __restrict__ pre, u64* __restrict__ terms) {
  __shared__ Jac<E> buf[CT_LANES];
  const size_t k = blockIdx.x;
  const int t = threadIdx.x;
  const uint32_t* e = ios + 8 * (4 * E + 1) * k + 32 * E;
  Jac<E> cur = ((e[t >> 5] >> (t & 31)) & 1) ? ld_jac<E>(ja + jac_at<E>(k, t, 0)) : jac_infinity<E>();   // (X Y Z of a step are adjacent)
  for (int d = 1; d < CT_LANES; d <<= 1) {   // Hillis-Steele in one LDS buffer: publish, read the partner, and only then the next level's publish
    buf[t] = cur;
    __syncthreads();
    if (t >= d) cur = jac_add_complete<E>(buf[t - d], cur);
    __syncthreads();
  }
  st_jac<E>(pre + 12 * E * (k * CT_LANES + t), cur);
  if (t == CT_LANES - 1) st_jac<E>(terms + 12 * E * k, cur);
}
// B[0] = offset_k, B[t] = offset_k + I[t-1]: one lane per (instance, step), into the B chain the witness kernels read
template <int E>
__global__ void chain_rebase_kernel(const uint32_t* __restrict__ ios, size_t K, const u64* __restrict__ pre, u64* __restrict__ jb) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= K * 257) return;
  const size_t k = i / 257; const int t = (int)(i % 257);
  const uint32_t* io = ios + 8 * (4 * E + 1) * k;
  Jac<E> b;
  ld_affine_words<E>(io + 16 * E, b.X, b.Y);
  b.Z = cone<E>();
  if (t) b = jac_add_complete<E>(b, ld_jac<E>(pre + 12 * E * (k * CT_LANES + (size_t)(t - 1))));
  st_jac<E>(jb + jac_at<E>(k, t, 0), b);
}

// Lanes of one scan workgroup.  Lists of K <= CS_LANES instances (tables up to 2^18 rows) are scanned by ONE workgroup
// (chain_scan_kernel, chain_seg_scan_kernel); longer ones (K <= 8,192: 2^22 rows) in blocks of CS_LANES instances by the three
// chain_block_* kernels behind chain_seg_scan_kernel, ordered by their kernel boundaries.
static constexpr int CS_LANES = 512;
template <int E>
__global__ void __launch_bounds__(CS_LANES) chain_scan_kernel(uint32_t* ios, size_t K, const u64* __restrict__ terms, u64* s0, u64* s1, int* __restrict__ err) {
  const size_t IOW = 8 * (4 * E + 1);
  const size_t k = threadIdx.x;
  Jac<E> cur = jac_infinity<E>();
  if (k < K) {
    if (k == 0) {   // start: the offset every instance of the preliminary list carries
      ld_affine_words<E>(ios + 16 * E, cur.X, cur.Y);
      cur.Z = cone<E>();
    } else cur = ld_jac<E>(terms + 12 * E * (k - 1));
  }
  u64* buf[2] = {s0, s1};
  int par = 0;
  for (size_t d = 1; d < K; d <<= 1, par ^= 1) {
    if (k < K) st_jac<E>(buf[par] + 12 * E * k, cur);
    __syncthreads();                                    // one workgroup: the barrier orders its global stores and loads
    if (k < K && k >= d) cur = jac_add_complete<E>(ld_jac<E>(buf[par] + 12 * E * (k - d)), cur);
  }
  if (k < K) st_jac<E>(buf[par] + 12 * E * k, cur);   // (the other buffer than the last level read)
  __syncthreads();
  const u64* sum = buf[par];
  const size_t NL = (K + TG_INV_BATCH - 1) / TG_INV_BATCH;
  if (k >= NL) return;
  Fq nrm[TG_INV_BATCH];
  for (int j = 0; j < TG_INV_BATCH; j++) {
    const size_t i = k + (size_t)j * NL;
    nrm[j] = fq_one();
    if (i >= K) continue;
    const Co<E> Z = ldc<E>(sum + 12 * E * i + 8 * E);
    if (czero<E>(Z)) { atomicOr(err, TG_ERR_INFINITY); continue; }
    nrm[j] = cnorm(Z);
  }
  batch_inverse(nrm);
  for (int j = 0; j < TG_INV_BATCH; j++) {
    const size_t i = k + (size_t)j * NL;
    if (i >= K) continue;
    const Jac<E> p = ld_jac<E>(sum + 12 * E * i);
    Co<E> v[2];
    affine_or_zero<E>(p, nrm[j], v);   // at infinity: zeros, the call is refused (TG_ERR_INFINITY)
    st_affine_words<E>(ios + IOW * i + 16 * E, v);
  }
}

// ---- independent scalar multiplications (sbn_prover_generate_trace_scalar_muls): every instance carries the same offset --------------
// The call shape of the reference's g2_mul_by_cofactor_circuit (src/curves/g2/circuit.rs:335-367): the caller wants e_k x_k, the table
// proves offset + e_k x_k.  Two kernels of K-lane work around the unchanged witness kernels:
//   scalar_mul_list_kernel      the `ios` rows the chain and witness kernels read, from the compact upload `cin` = points [K][16E],
//                               scalars [SC][8] (SC = K, or 1: one scalar shared by every instance), offset [16E]: one lane per u32
//                               word of the list, broadcasting the offset and the shared scalar;
//   scalar_mul_unoffset_kernel  after affine_lambda_kernel has left the instance outputs in `outs` (one u32 limb per u64 word):
//                               product = output + (-offset) by bnw::jac_add_complete -- output = offset (e = 0, or e a multiple of
//                               the point's order) meets opposite operands and is the point at infinity; e x = -2 offset makes
//                               output = -offset, equal operands, the doubling branch; the table refuses neither --
//                               then one batched inversion of TG_INV_BATCH norms per lane for the affine form, a zero Z skipped and
//                               flagged as in the tail of chain_scan_kernel.  The Jacobian sums wait in `jp` ([K][12E] u64) between
//                               the two passes of a lane, so a lane holds one point at a time.
// out_at / off_at (null in the call above: item i reads instance i): item i reads the output of instance out_at[i] and the offset
// words of instance off_at[i] -- the un-offset of a SEGMENTED list, K = its segments, final_s + (-start_s) from the segment's tail
// and head ("segmented chained lists" below).
// An instance the table cannot walk leaves garbage in `outs`; the arithmetic here is total (no index depends on a value), the call
// is refused through the error word of the witness kernels and the host drops what this kernel wrote.
template <int E>
__global__ void scalar_mul_list_kernel(const uint32_t* __restrict__ cin, size_t K, size_t SC, uint32_t* __restrict__ ios) {
  const size_t W = 16 * E, IOW = 2 * W + 8;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= IOW * K) return;
  const size_t k = i / IOW, w = i % IOW;
  const uint32_t* scal = cin + W * K;
  const uint32_t* off = scal + 8 * SC;
  ios[i] = w < W ? cin[W * k + w] : (w < 2 * W ? off[w - W] : scal[(SC == 1 ? 0 : 8 * k) + (w - 2 * W)]);
}
// What scalar_mul_unoffset_kernel and curve_program_values_kernel ("curve programs" below) share: dst[i] = output of instance
// out_at[i] (null: i) + the subtrahend of item i, which `load(i, m)` leaves in m.X, m.Y already negated (false: there is none, the
// value is the output itself), then the batched inversion and the affine words with their infinity flags.
template <int E, typename Load>
__device__ __forceinline__ void unoffset_store(size_t K, const u64* __restrict__ outs, const uint32_t* __restrict__ out_at, u64* __restrict__ jp,
                                               uint32_t* __restrict__ dst, unsigned char* __restrict__ infinity, Load load) {
  const size_t W = 16 * E;
  const size_t L = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t NL = (K + TG_INV_BATCH - 1) / TG_INV_BATCH;
  if (L >= NL) return;
  Fq nrm[TG_INV_BATCH];
  for (int j = 0; j < TG_INV_BATCH; j++) {
    const size_t i = L + (size_t)j * NL;
    nrm[j] = fq_one();
    if (i >= K) continue;
    Jac<E> o, m; u64 t4[4];
    const size_t io = out_at ? out_at[i] : i;
    for (int c = 0; c < 2; c++)
      for (int q = 0; q < E; q++) {
        const u64* src = outs + W * io + 8 * (c * E + q);
        for (int h = 0; h < 4; h++) t4[h] = (src[2 * h] & 0xffffffffULL) | (src[2 * h + 1] << 32);
        (c ? o.Y : o.X).c[q] = to_m(t4);
      }
    o.Z = cone<E>(); m.Z = o.Z;
    const Jac<E> r = load(i, m) ? jac_add_complete<E>(o, m) : o;
    st_jac<E>(jp + 12 * E * i, r);
    if (!czero<E>(r.Z)) nrm[j] = cnorm(r.Z);
  }
  batch_inverse(nrm);
  for (int j = 0; j < TG_INV_BATCH; j++) {
    const size_t i = L + (size_t)j * NL;
    if (i >= K) continue;
    Co<E> v[2];
    const bool inf = affine_or_zero<E>(ld_jac<E>(jp + 12 * E * i), nrm[j], v);   // the point at infinity: zero words and its flag
    st_affine_words<E>(dst + W * i, v);
    infinity[i] = inf ? 1 : 0;
  }
}
template <int E>
__global__ void scalar_mul_unoffset_kernel(const uint32_t* __restrict__ ios, size_t K, const u64* __restrict__ outs, u64* __restrict__ jp,
                                           uint32_t* __restrict__ products, unsigned char* __restrict__ infinity,
                                           const uint32_t* __restrict__ out_at = nullptr, const uint32_t* __restrict__ off_at = nullptr) {
  unoffset_store<E>(K, outs, out_at, jp, products, infinity, [&](size_t i, Jac<E>& m) {
    const size_t im = off_at ? off_at[i] : i;   // (segmented lists: out_at / off_at = the tail and the head of segment i)
    ld_affine_words<E>(ios + (2 * 16 * E + 8) * im + 16 * E, m.X, m.Y);
    m.Y = csub(csub(m.Y, m.Y), m.Y);   // -offset
    return true;
  });
}

// outs: [K][12][4] = x_k^e_k in standard form (fq12_chain_kernel on offsets of one); start: 12 coefficients of 8 u32 limbs
__global__ void __launch_bounds__(192) fq12_offset_scan_kernel(uint32_t* ios, size_t iow, size_t K, const uint32_t* __restrict__ start, const u64* __restrict__ outs) {
  __shared__ Fq B[12], X[12], PB[144];
  const int tid = threadIdx.x;
  if (tid < 12) { u64 t4[4]; u32x8_to_u64x4(start + 8 * tid, t4); B[tid] = to_m(t4); }
  for (size_t k = 0;; k++) {
    if (tid < 12) {   // lane c owns coefficient c of the running product
      u64 s[4]; from_m(B[tid], s);
      for (int w = 0; w < 8; w++) ios[iow * k + 96 + 8 * tid + w] = (uint32_t)(s[w >> 1] >> (32 * (w & 1)));
      X[tid] = to_m(outs + (k * 12 + tid) * 4);
    }
    if (k + 1 == K) break;
    __syncthreads();
    if (tid < 144) PB[tid] = mmul(B[tid / 12], X[tid % 12]);
    __syncthreads();
    if (tid < 12) B[tid] = fq12_fold_coeff(PB, tid);   // read again by the products only behind the next barrier
  }
}

// The Fq12 chain needs no second walk: products commute, so B[t] = offset_k * B'[t] with B' the chain of the preliminary list
// (offset one) -- steps + 1 INDEPENDENT products per instance, one workgroup each, in place over cb (standard form); the instance
// output B[steps] goes to outs again.
__global__ void __launch_bounds__(192) fq12_rebase_kernel(const uint32_t* __restrict__ ios, size_t iow, int steps, u64* __restrict__ cb, u64* __restrict__ outs) {
  __shared__ Fq O[12], X[12], PB[144];
  const size_t entry = blockIdx.x, k = entry / (size_t)(steps + 1);
  const int tid = threadIdx.x;
  u64* slot = cb + (entry * 12 + (size_t)(tid < 12 ? tid : 0)) * 4;
  if (tid < 12) { u64 t4[4]; u32x8_to_u64x4(ios + iow * k + 96 + 8 * tid, t4); O[tid] = to_m(t4); X[tid] = to_m(slot); }
  __syncthreads();
  if (tid < 144) PB[tid] = mmul(O[tid / 12], X[tid % 12]);
  __syncthreads();
  if (tid < 12) {
    const Fq v = fq12_fold_coeff(PB, tid);
    from_m(v, slot);
    if (entry % (size_t)(steps + 1) == (size_t)steps) from_m(v, outs + (k * 12 + tid) * 4);
  }
}

// ---- segmented chained lists (sbn_prover_generate_trace_msm_batch): many short chains packed into one unit --------------------------
// The list of a unit is cut into segments; instance g is a HEAD (its offset is the start of its segment, which the preliminary list
// carries in its offset words) or continues the chain (offset[g] = output[g - 1]).  Rows [M, K) are pads: copies of row M - 1 in x,
// offset and exponent -- they do not continue the chain.  chain_prefix_kernel, chain_rebase_kernel and fq12_rebase_kernel run
// unchanged on all K rows (the preliminary rows of the pads are row M - 1 already, so their chains and outputs are its too).
//   chain_seg_scan_kernel  the segmented form of chain_scan_kernel, ONE workgroup, lane k = instance k: it starts from the start of
//                          its segment when k is a head (head[k] == k), else from the term e_{k-1} x_{k-1}; the Hillis-Steele level of
//                          stride d adds the partner k - d only while k - d >= head[k], so after that level lane k holds the sum over
//                          [max(head, k - 2d + 1), k] and a segment never reads across its head.  Same ping-pong in global scratch
//                          (the workgroup barrier orders its stores and loads), same batched-inversion tail and TG_ERR_INFINITY;
//                          the tail writes the offset of row i from the sum of lane min(i, M - 1): the pads.
//   fq12_seg_scan_kernel   fq12_offset_scan_kernel with ONE WORKGROUP PER SEGMENT, the same lane roles and LDS layout: each walks
//                          the len - 1 dependent products of its own instances from its own start; the workgroup of the last segment
//                          also writes its last offset into the pad rows.
// Nothing either kernel stores to global memory is read by ANOTHER workgroup inside it: the scan is one workgroup, and an Fq12
// segment writes the offset words of its own rows (and of the pads), which the kernels behind the kernel boundary read.
template <int E>
__global__ void __launch_bounds__(CS_LANES) chain_seg_scan_kernel(uint32_t* ios, size_t K, size_t M, const uint32_t* __restrict__ head, const u64* __restrict__ terms,
                                                                  u64* s0, u64* s1, int* __restrict__ err) {
  const size_t IOW = 8 * (4 * E + 1);
  const size_t k = threadIdx.x;
  Jac<E> cur = jac_infinity<E>();
  size_t hd = 0;
  if (k < M) {
    hd = head[k];
    if (hd == k) {   // a head: the start of its segment, in the offset words of its preliminary row
      ld_affine_words<E>(ios + IOW * k + 16 * E, cur.X, cur.Y);
      cur.Z = cone<E>();
    } else cur = ld_jac<E>(terms + 12 * E * (k - 1));   // (hd < k here, so k >= 1)
  }
  u64* buf[2] = {s0, s1};
  int par = 0;
  for (size_t d = 1; d < M; d <<= 1, par ^= 1) {
    if (k < M) st_jac<E>(buf[par] + 12 * E * k, cur);
    __syncthreads();                                    // one workgroup: the barrier orders its global stores and loads
    if (k < M && k >= hd + d) cur = jac_add_complete<E>(ld_jac<E>(buf[par] + 12 * E * (k - d)), cur);   // the partner is in lane k's segment
  }
  if (k < M) st_jac<E>(buf[par] + 12 * E * k, cur);   // (the other buffer than the last level read)
  __syncthreads();
  const u64* sum = buf[par];
  const size_t NL = (K + TG_INV_BATCH - 1) / TG_INV_BATCH;
  if (k >= NL) return;
  Fq nrm[TG_INV_BATCH];
  for (int j = 0; j < TG_INV_BATCH; j++) {
    const size_t i = k + (size_t)j * NL;
    nrm[j] = fq_one();
    if (i >= K) continue;
    const Co<E> Z = ldc<E>(sum + 12 * E * (i < M ? i : M - 1) + 8 * E);
    if (czero<E>(Z)) { atomicOr(err, TG_ERR_INFINITY); continue; }
    nrm[j] = cnorm(Z);
  }
  batch_inverse(nrm);
  for (int j = 0; j < TG_INV_BATCH; j++) {
    const size_t i = k + (size_t)j * NL;
    if (i >= K) continue;
    const Jac<E> p = ld_jac<E>(sum + 12 * E * (i < M ? i : M - 1));   // a pad row carries the offset of row M - 1
    Co<E> v[2];
    affine_or_zero<E>(p, nrm[j], v);   // at infinity: zeros, the call is refused (TG_ERR_INFINITY)
    st_affine_words<E>(ios + IOW * i + 16 * E, v);
  }
}
// ---- complete sums (sbn_prover_generate_trace_msm_batch_complete): the start of segment s is start candidate choice[s] -----------------
// The scan kernels above and below read the start of a segment from the offset words of its head row, and chain_rebase_kernel
// builds B[t] = offset + I[t-1] with the complete addition, so the B chain is right whether or not the TABLE can walk it.  Two
// small kernels turn that into a per-segment verdict without touching the kernels of the explicit-start calls:
//   chain_seg_start_kernel   one lane per (segment, word): the offset words of the head row of segment s <- candidate choice[s];
//   chain_seg_status_kernel  one lane per (real instance, step t <= 256), behind the rebase: a bad event of the table's walk is
//                            B[t] at infinity (a zero Z: the step behind B[s] = -A[s], or for t = 256 an output, i.e. the next offset
//                            or the final, at infinity) or, at a set bit, B[t] = +-A[t] (X2 Z1^2 = X1 Z2^2) -- the refusals of
//                            affine_lambda_kernel.  A lane that meets one ORs a bit into the status word of its instance's segment
//                            (seg_of[k]); a clean list stores nothing, and no lane reads a status word.
// The host clears the status words, reads them back behind the kernel, moves the failing segments to their next candidate and runs
// start, scan, rebase and status again; the terms e_k x_k and the partial sums I[t] enter no start and are computed once.
template <int E>
__global__ void chain_seg_start_kernel(uint32_t* ios, size_t S, const uint32_t* __restrict__ seg_head, const uint32_t* __restrict__ choice,
                                       const uint32_t* __restrict__ candidates) {
  const size_t W = 16 * E, IOW = 2 * W + 8;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= S * W) return;
  const size_t s = i / W, w = i % W;
  ios[IOW * seg_head[s] + W + w] = candidates[W * choice[s] + w];
}
// the verdict on step t <= 256 of instance k, for this kernel and for curve_program_status_kernel ("curve programs" below)
template <int E>
__device__ __forceinline__ bool walk_bad_event(const uint32_t* __restrict__ ios, const u64* __restrict__ ja, const u64* __restrict__ jb, size_t k, int t) {
  const Co<E> Z2 = ldc<E>(jb + jac_at<E>(k, t, 2));
  if (czero<E>(Z2)) return true;
  if (t == 256 || !((ios[8 * (4 * E + 1) * k + 32 * E + (t >> 5)] >> (t & 31)) & 1)) return false;
  const Co<E> Z1 = ldc<E>(ja + jac_at<E>(k, t, 2));
  const Co<E> D = csub(cmul(ldc<E>(jb + jac_at<E>(k, t, 0)), cmul(Z1, Z1)), cmul(ldc<E>(ja + jac_at<E>(k, t, 0)), cmul(Z2, Z2)));
  return czero<E>(Z1) || czero<E>(D);
}
template <int E>
__global__ void chain_seg_status_kernel(const uint32_t* __restrict__ ios, size_t M, const u64* __restrict__ ja, const u64* __restrict__ jb,
                                        const uint32_t* __restrict__ seg_of, int* __restrict__ status) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= M * 257) return;
  const size_t k = i / 257;
  if (walk_bad_event<E>(ios, ja, jb, k, (int)(i % 257))) atomicOr(status + seg_of[k], 1);
}

// ---- lists of more than CS_LANES instances: the same scan in blocks of CS_LANES, chained and segmented alike --------------------------
// `head` is null for a chained list (one segment: every head is 0, M = K).  Three kernels; what one stores another reads only behind
// the kernel boundary between them, and no workgroup waits for another one.
//   chain_block_scan_kernel   grid = the blocks that hold a real instance: the Hillis-Steele scan of chain_seg_scan_kernel INSIDE
//                             block b, the partner k - d taken only while k - d >= max(head[k], first lane of b).  Lane k ends with
//                             the sum over [max(head[k], first lane of b), k] in `local` (the buffer of the last level, 9 levels
//                             whatever M is: the barrier count is uniform).
//   chain_block_carry_kernel  one lane, at most 15 dependent additions: in[b] = what the lanes of block b whose segment began in an
//                             earlier block still lack = the sum from their head to the last lane of block b - 1.  Those lanes are a
//                             prefix of the block and share one head (a later head closes the segment).  With t = the local sum of
//                             block b - 1's last lane: in[b] = t when that lane's head lies inside block b - 1 (or b = 1), else
//                             in[b - 1] + t.  A head ON the first lane of a block takes no carry (head >= first lane), a head on the
//                             last lane of a block starts the carry anew: no sum ever crosses a segment head.
//   chain_block_tail_kernel   the batched-inversion tail of chain_seg_scan_kernel as a grid: sum(i) = local[j] or in[block of j] +
//                             local[j], j = min(i, M - 1) (the pads), kept in `sum` between the two passes of a lane (its own slots);
//                             TG_ERR_INFINITY and the offset words as there.
template <int E>
__global__ void __launch_bounds__(CS_LANES) chain_block_scan_kernel(const uint32_t* __restrict__ ios, size_t M, const uint32_t* __restrict__ head,
                                                                    const u64* __restrict__ terms, u64* s0, u64* s1) {
  const size_t IOW = 8 * (4 * E + 1);
  const size_t first = (size_t)blockIdx.x * CS_LANES, k = first + threadIdx.x;
  Jac<E> cur = jac_infinity<E>();
  size_t lo = first;   // the lowest partner of this lane
  if (k < M) {
    const size_t hd = head ? head[k] : 0;
    lo = hd > first ? hd : first;
    if (hd == k) {   // a head: the start of its segment, in the offset words of its preliminary row
      ld_affine_words<E>(ios + IOW * k + 16 * E, cur.X, cur.Y);
      cur.Z = cone<E>();
    } else cur = ld_jac<E>(terms + 12 * E * (k - 1));   // (hd < k here, so k >= 1)
  }
  u64* buf[2] = {s0, s1};
  int par = 0;
  for (size_t d = 1; d < (size_t)CS_LANES; d <<= 1, par ^= 1) {
    if (k < M) st_jac<E>(buf[par] + 12 * E * k, cur);
    __syncthreads();                                    // the partner is in this workgroup: the barrier orders its global stores and loads
    if (k < M && k >= lo + d) cur = jac_add_complete<E>(ld_jac<E>(buf[par] + 12 * E * (k - d)), cur);
  }
  if (k < M) st_jac<E>(buf[par] + 12 * E * k, cur);   // nine levels: par = 1, `local` is s1
}
template <int E>
__global__ void chain_block_carry_kernel(size_t M, const uint32_t* __restrict__ head, const u64* __restrict__ local, u64* __restrict__ in) {
  if (blockIdx.x || threadIdx.x) return;
  Jac<E> run = jac_infinity<E>();
  for (size_t b = 1; b * CS_LANES < M; b++) {
    const size_t last = b * CS_LANES - 1;   // the last lane of block b - 1 (< M)
    const Jac<E> t = ld_jac<E>(local + 12 * E * last);
    const bool fresh = b == 1 || (head && head[last] >= (b - 1) * CS_LANES);
    run = fresh ? t : jac_add_complete<E>(run, t);
    st_jac<E>(in + 12 * E * b, run);
  }
}
template <int E>
__global__ void chain_block_tail_kernel(uint32_t* ios, size_t K, size_t M, const uint32_t* __restrict__ head, const u64* __restrict__ local,
                                        const u64* __restrict__ in, u64* __restrict__ sum, int* __restrict__ err) {
  const size_t IOW = 8 * (4 * E + 1);
  const size_t L = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t NL = (K + TG_INV_BATCH - 1) / TG_INV_BATCH;
  if (L >= NL) return;
  Fq nrm[TG_INV_BATCH];
  for (int j = 0; j < TG_INV_BATCH; j++) {
    const size_t i = L + (size_t)j * NL;
    nrm[j] = fq_one();
    if (i >= K) continue;
    const size_t src = i < M ? i : M - 1, b = src / CS_LANES;   // a pad row carries the offset of row M - 1
    Jac<E> p = ld_jac<E>(local + 12 * E * src);
    if (b && (head ? head[src] : 0) < b * CS_LANES) p = jac_add_complete<E>(ld_jac<E>(in + 12 * E * b), p);
    st_jac<E>(sum + 12 * E * i, p);
    if (czero<E>(p.Z)) { atomicOr(err, TG_ERR_INFINITY); continue; }
    nrm[j] = cnorm(p.Z);
  }
  batch_inverse(nrm);
  for (int j = 0; j < TG_INV_BATCH; j++) {
    const size_t i = L + (size_t)j * NL;
    if (i >= K) continue;
    const Jac<E> p = ld_jac<E>(sum + 12 * E * i);
    Co<E> v[2];
    affine_or_zero<E>(p, nrm[j], v);   // at infinity: zeros, the call is refused (TG_ERR_INFINITY)
    st_affine_words<E>(ios + IOW * i + 16 * E, v);
  }
}
// seg_head / seg_len: [segments] (blockIdx.x = segment; the host has checked head + len <= M <= K); starts: [SC][96] u32, SC = 1
// (one start shared by every segment) or the number of segments; outs as fq12_offset_scan_kernel
__global__ void __launch_bounds__(192) fq12_seg_scan_kernel(uint32_t* ios, size_t iow, size_t K, size_t M, const uint32_t* __restrict__ seg_head,
                                                            const uint32_t* __restrict__ seg_len, const uint32_t* __restrict__ starts, size_t SC,
                                                            const u64* __restrict__ outs) {
  __shared__ Fq B[12], X[12], PB[144];
  const int tid = threadIdx.x;
  const size_t s = blockIdx.x, h = seg_head[s], len = seg_len[s];
  const uint32_t* start = starts + (SC == 1 ? 0 : 96 * s);
  if (tid < 12) { u64 t4[4]; u32x8_to_u64x4(start + 8 * tid, t4); B[tid] = to_m(t4); }
  for (size_t j = 0;; j++) {
    const size_t k = h + j;
    if (tid < 12) {   // lane c owns coefficient c of the running product
      u64 sw[4]; from_m(B[tid], sw);
      for (int w = 0; w < 8; w++) ios[iow * k + 96 + 8 * tid + w] = (uint32_t)(sw[w >> 1] >> (32 * (w & 1)));
      X[tid] = to_m(outs + (k * 12 + tid) * 4);
    }
    if (j + 1 == len) break;
    __syncthreads();
    if (tid < 144) PB[tid] = mmul(B[tid / 12], X[tid % 12]);
    __syncthreads();
    if (tid < 12) B[tid] = fq12_fold_coeff(PB, tid);   // read again by the products only behind the next barrier
  }
  if (s + 1 == gridDim.x && tid < 12) {   // the pads: the offset of instance M - 1 again (lane c wrote B[c] itself)
    u64 sw[4]; from_m(B[tid], sw);
    for (size_t g = M; g < K; g++)
      for (int w = 0; w < 8; w++) ios[iow * g + 96 + 8 * tid + w] = (uint32_t)(sw[w >> 1] >> (32 * (w & 1)));
  }
}

// ---- power towers (sbn_prover_generate_trace_powers): x of level l = the output of level l - 1, offset = one everywhere ------------
// `count` towers of `depth` consecutive instances (tower-major: instance g = tower * depth + level).  The levels of a tower are
// sequential by definition, the towers independent, so ONE workgroup walks the levels of its tower with the lane roles, the LDS
// layout and the step of fq12_chain_kernel: at the end of a level the output sits in B in LDS; the twelve coefficient lanes turn
// it into standard form, store it into the x words of the next instance in `ios` (for the kernels that follow: the row kernel, the
// flags and the download read them behind the kernel boundary, which is where those stores become visible to other workgroups) and
// load A from those very registers, as fq12_chain_kernel would from the words.  Nothing this kernel stores to global memory is read
// again inside it, so no fence and no scope question arises; the barrier orders LDS only.  `ios` arrives with the level-0 x, the
// offsets (one) and the exponents of every instance; the x words of the levels above 0 are written here.
//   fq12_tower_pad_kernel  the reference's resize rule on the device: instances [M, K) become instance M - 1 again -- its `ios`
//                          row (whose x may have been derived above), both chains and the compact output -- one workgroup per pad.
__global__ void __launch_bounds__(320) fq12_tower_kernel(uint32_t* ios, size_t iow, int steps, size_t depth, u64* __restrict__ ca, u64* __restrict__ cb,
                                                         u64* __restrict__ outs) {
  __shared__ Fq A[12], B[12], PA[144], PB[144];
  const int tid = threadIdx.x, c = tid % 12;
  const bool is_a = tid < 12, is_b = tid >= 12 && tid < 24;
  for (size_t l = 0; l < depth; l++) {
    const size_t k = blockIdx.x * depth + l;
    uint32_t* io = ios + iow * k;
    Fq nv;
    if (is_a) {
      u64 t4[4];
      if (l == 0) u32x8_to_u64x4(io + 8 * c, t4);
      else {   // the link: output of level l - 1 -> x of level l
        from_m(B[c], t4);
        for (int w = 0; w < 8; w++) io[8 * c + w] = (uint32_t)(t4[w >> 1] >> (32 * (w & 1)));
      }
      nv = to_m(t4);
    } else if (is_b) { u64 t4[4]; u32x8_to_u64x4(io + 96 + 8 * c, t4); nv = to_m(t4); }
    __syncthreads();                                                     // the previous level's B has been read
    if (is_a) A[c] = nv; else if (is_b) B[c] = nv;
    __syncthreads();
    for (int t = 0;; t++) {
      if (is_a || is_b) from_m((is_a ? A : B)[c], (is_a ? ca : cb) + ((k * (size_t)(steps + 1) + t) * 12 + c) * 4);
      if (t == steps) { if (is_b) from_m(B[c], outs + (k * 12 + c) * 4); break; }
      const bool bit = (io[192 + (t >> 5)] >> (t & 31)) & 1;            // uniform over the workgroup
      if (tid < 144) PA[tid] = mmul(A[tid / 12], A[tid % 12]);
      else if (tid < 288 && bit) PB[tid - 144] = mmul(A[(tid - 144) / 12], B[(tid - 144) % 12]);
      __syncthreads();
      Fq fv;
      if (is_a) fv = fq12_fold_coeff(PA, c);
      else if (is_b && bit) fv = fq12_fold_coeff(PB, c);
      __syncthreads();                                                   // every product has been read, A / B may change
      if (is_a) A[c] = fv; else if (is_b && bit) B[c] = fv;
      __syncthreads();
    }
  }
}
// instances [M, K) <- instance M - 1: blockIdx.x = pad index; cw1 = u64 words of one chain of one instance ((steps + 1) * 48)
__global__ void __launch_bounds__(256) fq12_tower_pad_kernel(uint32_t* ios, size_t iow, size_t M, size_t K, size_t cw1, u64* ca, u64* cb, u64* outs) {
  const size_t g = M + blockIdx.x, src = M - 1;
  if (g >= K) return;
  for (size_t i = threadIdx.x; i < iow; i += blockDim.x) ios[iow * g + i] = ios[iow * src + i];
  for (size_t i = threadIdx.x; i < cw1; i += blockDim.x) { ca[cw1 * g + i] = ca[cw1 * src + i]; cb[cw1 * g + i] = cb[cw1 * src + i]; }
  for (size_t i = threadIdx.x; i < 48; i += blockDim.x) outs[48 * g + i] = outs[48 * src + i];
}

// ---- field programs (sbn_prover_generate_trace_program): x and offset of an instance = a literal or the output of an earlier one ----
// The host sorts the nodes by level (level 0: no link; otherwise 1 + the largest level linked to), so the nodes of one level are
// independent and every node they link to lies in an EARLIER level.  ONE LAUNCH PER LEVEL, one workgroup per node of that level,
// with the lane roles, the LDS layout and the step of fq12_chain_kernel (spelled out in each of the three kernels: one shared
// function cost the two one-level kernels two VGPRs and 0.7 % of their time); the new part is the head.  The twelve coefficient lanes of
// A (x) and of B (offset) look their operand up in the node table: a link (bit 31) reads the standard-form output of node j from
// `outs`, which an earlier LAUNCH wrote, stores those words into the x or offset words of the node's own `ios` row (for the row,
// flag and download kernels that follow) and enters the chain from those very registers; a literal, or one, loads from `ios`, where
// the host put it.  Links cross kernel boundaries only: a workgroup writes outs[k] of its own node and reads outs[j] of nodes of
// earlier levels, so nothing a launch stores to global memory is read again inside it -- no flag, no spin, no fence, no scope
// question (the rule of fq12_tower_kernel above); the barriers order LDS only.  The price is one launch boundary per level, beside
// chains of 64 to 256 dependent steps.  fq12_tower_pad_kernel fills the pads behind the last level.
//   nodes: [count][3] = (x, offset, exp) of include/sbn.h's sbn_program_node; order: the node of workgroup blockIdx.x of this launch
//   (every entry < count <= K and every link j < its node: program_plan, program.hip, refuses anything else before a launch)
__global__ void __launch_bounds__(320) fq12_program_level_kernel(uint32_t* ios, size_t iow, int steps, const uint32_t* __restrict__ nodes,
                                                                 const uint32_t* __restrict__ order, u64* __restrict__ ca, u64* __restrict__ cb, u64* outs) {
  __shared__ Fq A[12], B[12], PA[144], PB[144];
  const size_t k = order[blockIdx.x];
  uint32_t* io = ios + iow * k;
  const int tid = threadIdx.x, c = tid % 12;
  const bool is_a = tid < 12, is_b = tid >= 12 && tid < 24;
  if (is_a || is_b) {
    const uint32_t src = nodes[3 * k + (is_a ? 0 : 1)];
    uint32_t* w8 = io + (is_a ? 0 : 96) + 8 * c;
    u64 t4[4];
    if (src & 0x80000000u) {   // the link: output of node j (an earlier launch) -> x / offset of this node
      const u64* o = outs + ((size_t)(src & 0x7fffffffu) * 12 + c) * 4;
      for (int i = 0; i < 4; i++) t4[i] = o[i];
      for (int w = 0; w < 8; w++) w8[w] = (uint32_t)(t4[w >> 1] >> (32 * (w & 1)));
    } else u32x8_to_u64x4(w8, t4);
    (is_a ? A : B)[c] = to_m(t4);
  }
  __syncthreads();
  for (int t = 0;; t++) {
    if (is_a || is_b) from_m((is_a ? A : B)[c], (is_a ? ca : cb) + ((k * (size_t)(steps + 1) + t) * 12 + c) * 4);
    if (t == steps) { if (is_b) from_m(B[c], outs + (k * 12 + c) * 4); break; }
    const bool bit = (io[192 + (t >> 5)] >> (t & 31)) & 1;            // uniform over the workgroup
    if (tid < 144) PA[tid] = mmul(A[tid / 12], A[tid % 12]);
    else if (tid < 288 && bit) PB[tid - 144] = mmul(A[(tid - 144) / 12], B[(tid - 144) % 12]);
    __syncthreads();
    Fq nv;
    if (is_a) nv = fq12_fold_coeff(PA, c);
    else if (is_b && bit) nv = fq12_fold_coeff(PB, c);
    __syncthreads();                                                   // every product has been read, A / B may change
    if (is_a) A[c] = nv; else if (is_b && bit) B[c] = nv;
    __syncthreads();
  }
}

// ---- mapped links (sbn_prover_generate_trace_program_m): x / offset of an instance = frob(output of an earlier one, m) -------------
// A pre-pass in FRONT of the level launch of every level that has a mapped operand; fq12_program_level_kernel above stays as it is.
// One workgroup per (node of the level, mapped operand): the twelve coefficient lanes read the standard-form output of node j from
// `outs`, which the launch of an EARLIER level wrote, apply f -> f^(p^m) in the flat basis -- coefficient k of w^k is the Fq2
// element a_k = c[k] + c[k+6] i and becomes conj^m(a_k) * G[m][k] (include/sbn.h, "Mapped links"): lanes k and k + 6 exchange their
// halves over LDS and each folds its half of the Fq2 product -- and store the mapped words into the x / offset words of the node's
// own `ios` row.  The host has marked that operand as a literal in the device copy of the node table, so the level launch behind
// this one loads it as it loads a literal.  The rule of the level kernel is kept: this launch reads what launches of earlier
// levels stored and stores what only later launches read -- no flag, no spin, no fence; the barrier orders LDS only.
//   tbl: [gridDim.x][4] = (node k, 0: x / 1: offset, node j, map m); k < K, j < k, 1 <= m <= 11 (program_plan refuses the rest)
__device__ const u64 FQ12_FROBENIUS_G[12][6][2][4] = {
#include "fq12_frobenius_consts.hpp"
};
__global__ void __launch_bounds__(64) fq12_program_map_kernel(uint32_t* ios, size_t iow, const uint32_t* __restrict__ tbl, const u64* __restrict__ outs) {
  __shared__ Fq V[12];
  const uint32_t* e = tbl + 4 * (size_t)blockIdx.x;
  const uint32_t m = e[3];
  const int c = threadIdx.x;
  Fq own;
  if (c < 12) {
    u64 t4[4];
    const u64* o = outs + ((size_t)e[2] * 12 + c) * 4;
    for (int i = 0; i < 4; i++) t4[i] = o[i];
    own = to_m(t4);
    if (c >= 6 && (m & 1)) own = fsub(Fq{{0, 0, 0, 0}}, own);   // conj^m: the imaginary half changes sign for an odd m
    V[c] = own;
  }
  __syncthreads();
  if (c < 12) {
    const int k = c % 6;
    const Fq other = V[c < 6 ? c + 6 : c - 6];
    const Fq a = mmul(own, to_m(FQ12_FROBENIUS_G[m][k][0])), b = mmul(other, to_m(FQ12_FROBENIUS_G[m][k][1]));
    u64 s4[4];
    from_m(c < 6 ? fsub(a, b) : fadd(a, b), s4);   // re = re g0 - im g1, im = im g0 + re g1
    uint32_t* w8 = ios + iow * e[0] + 96 * e[1] + 8 * c;
    for (int w = 0; w < 8; w++) w8[w] = (uint32_t)(s4[w >> 1] >> (32 * (w & 1)));
  }
}

// ---- curve programs (sbn_prover_generate_trace_curve_program): x and offset of an instance = a literal point, the start, or the ------
// ---- output of an earlier instance --------------------------------------------------------------------------------------------------
// The field programs above on G1 / G2 (E = 1 / 2).  The host sorts the nodes by level, so the nodes of one level are independent
// and every node they link to lies in an EARLIER level.  Per level TWO launches, ordered by their kernel boundary:
//   curve_program_level_kernel       one LANE per node of the level (placement 1), the chain step of chain_kernel / exp_chains, copied:
//     calling bnw::exp_chains_from instead cost the 16-level G2 program 3 % of its time;
//   curve_program_level_coop_kernel  one WAVE per node of the level (placement 2), the chain step of chain_coop_kernel, copied:
//     shared as one function it cost the explicit G1 list 0.8 % of its time.  The new part of both is the head: an
//     operand whose node word has bit 31 set is the affine output of node j, which an earlier LAUNCH left in `outs` ([K][16E]
//     u32, the word order of a point in `ios`); its words go into the x or offset words of the node's own `ios` row (for the row,
//     flag and download kernels that follow) and enter the chain from those registers.  A literal, or the start, loads from
//     `ios`, where the host put it.  The chain's own degenerate flags go to a word nobody reads: the status kernel finds them.
//   curve_program_status_kernel      one lane per (node of the level, step t <= 256), the verdict of chain_seg_status_kernel (walk_bad_event): a bad
//     event of the table's walk is B[t] at infinity or, at a set bit, B[t] = +-A[t].  A lane that meets one ORs into the ONE status
//     word; a clean level stores nothing there.  The lane of t = 256 also turns B[256] into its affine form (one Fermat chain) and
//     writes outs[k] -- zeros for an output at infinity, which the status word reports.
// Links cross kernel boundaries only: a launch writes ja / jb / the ios row / outs of its OWN nodes and reads outs[j] of nodes of
// earlier levels, and the status kernel reads the chains the launch in front of it stored.  Nothing a launch stores to global
// memory is read again inside it -- no flag, no spin, no fence (the rule of fq12_program_level_kernel).  A node with a bad event
// leaves garbage behind it; the arithmetic is total (no index depends on a value) and the host drops everything when the status
// word is set.  The pads are nodes of the level of node count - 1 (the host repeats its node words), so they need no kernel.
//   nodes: [K][3] = (x, offset, exp) of include/sbn.h's sbn_program_node; order: the node of item i of this launch (every entry
//   < K and every link j < its node: curve_program_plan, curve_program.hip, refuses anything else before a launch)
template <int E>
__device__ __forceinline__ Co<E> program_operand(uint32_t* io8, uint32_t src, const uint32_t* outs, int w) {   // coordinate w (0: x, 1: y) of one operand
  Co<E> r; u64 t4[4];
#pragma unroll   // (r.c[q] under a rolled loop is an indexed stack object: scratch)
  for (int q = 0; q < E; q++) {
    uint32_t* dst = io8 + 8 * (w * E + q);
    if (src & 0x80000000u) {
      const uint32_t* o = outs + 16 * E * (size_t)(src & 0x7fffffffu) + 8 * (w * E + q);
      for (int i = 0; i < 4; i++) {
        const uint32_t lo = o[2 * i], hi = o[2 * i + 1];
        dst[2 * i] = lo; dst[2 * i + 1] = hi;
        t4[i] = (u64)lo | ((u64)hi << 32);
      }
    } else u32x8_to_u64x4(dst, t4);
    r.c[q] = to_m(t4);
  }
  return r;
}
template <int E>
__global__ void __launch_bounds__(64) curve_program_level_kernel(uint32_t* ios, const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ order, size_t count,
                                                                 u64* __restrict__ ja, u64* __restrict__ jb, const uint32_t* outs, int* __restrict__ err) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= count) return;
  const size_t k = order[i];
  uint32_t* io = ios + 8 * (4 * E + 1) * k;
  Jac<E> a, b;
  a.X = program_operand<E>(io, nodes[3 * k], outs, 0); a.Y = program_operand<E>(io, nodes[3 * k], outs, 1);
  b.X = program_operand<E>(io + 16 * E, nodes[3 * k + 1], outs, 0); b.Y = program_operand<E>(io + 16 * E, nodes[3 * k + 1], outs, 1);
  a.Z = cone<E>(); b.Z = cone<E>();
  const uint32_t* e = io + 32 * E;
  int bad = 0;
  for (int t = 0;; t++) {   // exp_chains (bn254w.cuh) from here on
    stc<E>(ja + jac_at<E>(k, t, 0), a.X); stc<E>(ja + jac_at<E>(k, t, 1), a.Y); stc<E>(ja + jac_at<E>(k, t, 2), a.Z);
    stc<E>(jb + jac_at<E>(k, t, 0), b.X); stc<E>(jb + jac_at<E>(k, t, 1), b.Y); stc<E>(jb + jac_at<E>(k, t, 2), b.Z);
    if (t == 256) break;
    const bool bit = (e[t >> 5] >> (t & 31)) & 1;
    if (bit) { bool deg; b = jac_add<E>(b, a, &deg); if (deg) bad |= TG_ERR_DEGENERATE; }
    if (czero<E>(a.Y)) bad |= TG_ERR_DEGENERATE;
    a = jac_double<E>(a);
  }
  if (bad) atomicOr(err, bad);
}
template <int E>
__global__ void __launch_bounds__(CP_LANES) curve_program_level_coop_kernel(uint32_t* ios, const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ order,
                                                                            u64* __restrict__ ja, u64* __restrict__ jb, const uint32_t* outs, int* __restrict__ err,
                                                                            ChainProgDev cp) {
  __shared__ Fq V[CP_MAX_SLOTS];
  __shared__ uint32_t prog[2][24 * CP_LANES];
  const size_t k = order[blockIdx.x];
  const int lane = threadIdx.x;
  for (int b = 0; b < 2; b++) for (int lv = 0; lv < cp.levels[b]; lv++) prog[b][lv * CP_LANES + lane] = cp.ops[b][lv * CP_LANES + lane];
  uint32_t* io = ios + 8 * (4 * E + 1) * k;
  if (lane < 4 * E) {   // lane = (operand, coordinate, component): x.x x.y offset.x offset.y, E each, as in the io words
    const uint32_t src = nodes[3 * k + lane / (2 * E)];
    uint32_t* w8 = io + 8 * lane;
    u64 t4[4];
    if (src & 0x80000000u) {   // the link: affine output of node j (an earlier launch) -> x / offset of this node
      const uint32_t* o = outs + 16 * E * (size_t)(src & 0x7fffffffu) + 8 * (lane % (2 * E));
      uint32_t v[8];
      for (int i = 0; i < 8; i++) v[i] = o[i];
      for (int i = 0; i < 8; i++) w8[i] = v[i];
      for (int i = 0; i < 4; i++) t4[i] = (u64)v[2 * i] | ((u64)v[2 * i + 1] << 32);
    } else u32x8_to_u64x4(w8, t4);
    V[cp.in_slot[lane]] = to_m(t4);
  }
  if (lane >= 32 && lane < 34) V[cp.one_slot[lane - 32]] = fq_one();
  if (E == 2 && lane >= 40 && lane < 42) V[cp.zero_slot[lane - 40]] = Fq{{0, 0, 0, 0}};
  __syncthreads();
  // the exponent words, before the walk: the row is this workgroup's own and only its operand words were written above
  const uint32_t* e = io + 32 * E;
  for (int t = 0;; t++) {   // chain_coop_kernel from here on
    if (lane < 6 * E) {
      const int which = lane / (3 * E), cc = (lane % (3 * E)) / E, q = lane % E;
      const Fq v = V[cp.coord[lane]];
      u64* dst = (which ? jb : ja) + jac_at<E>(k, t, cc) + 4 * q;
      for (int i = 0; i < 4; i++) dst[i] = v.l[i];
    }
    if (t == 256) break;
    const int bit = (e[t >> 5] >> (t & 31)) & 1;
    const uint32_t* ops = prog[bit];
    const int nl = cp.levels[bit];
    for (int lv = 0; lv < nl; lv++) {
      const uint32_t op = ops[lv * CP_LANES + lane];
      const int kind = op & 255, d = (op >> 8) & 255, a = (op >> 16) & 255, b = op >> 24;
      if (kind == CP_MUL) V[d] = mmul(V[a], V[b]);
      else if (kind == CP_ADD) V[d] = fadd(V[a], V[b]);
      else if (kind == CP_SUB) V[d] = fsub(V[a], V[b]);
      else if (kind == CP_COPY) V[d] = V[a];
      else if (kind == CP_CHK1) { if (fzero(V[a])) atomicOr(err, TG_ERR_DEGENERATE); }
      else if (kind == CP_CHK2) { if (fzero(V[a]) && fzero(V[b])) atomicOr(err, TG_ERR_DEGENERATE); }
      __syncthreads();
    }
  }
}
template <int E>
__global__ void __launch_bounds__(256) curve_program_status_kernel(const uint32_t* __restrict__ ios, const uint32_t* __restrict__ order, size_t count,
                                                                   const u64* __restrict__ ja, const u64* __restrict__ jb, uint32_t* __restrict__ outs,
                                                                   int* __restrict__ status) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= count * 257) return;
  const size_t k = order[i / 257]; const int t = (int)(i % 257);
  const bool bad = walk_bad_event<E>(ios, ja, jb, k, t);
  if (bad) atomicOr(status, 1);
  if (t != 256) return;
  const Co<E> Z2 = ldc<E>(jb + jac_at<E>(k, 256, 2));
  Co<E> v[2];
  if (bad) { v[0] = Z2; v[1] = Z2; }   // the point at infinity has no affine form: zeros, and the status word says so
  else {
    const Co<E> zi = cinv_from_norm(Z2, finv_fermat(cnorm(Z2))), zi2 = cmul(zi, zi);
    v[0] = cmul(ldc<E>(jb + jac_at<E>(k, 256, 0)), zi2); v[1] = cmul(ldc<E>(jb + jac_at<E>(k, 256, 1)), cmul(zi2, zi));
  }
  st_affine_words<E>(outs + 16 * E * k, v);
}
// values[i] = out_i + (-T_i), i < K real nodes, behind affine_lambda_kernel: the unoffset_store of scalar_mul_unoffset_kernel with the subtrahend from
// `neg_blinds` ([K][16E] u32 affine words of -T_i, uploaded by the host; blind_inf[i] = 1: T_i is the point at infinity and the
// value is the output itself) instead of the instance's own offset words.  Outputs, `jp`, the batched inversion and the flags as there.
template <int E>
__global__ void curve_program_values_kernel(size_t K, const u64* __restrict__ outs, const uint32_t* __restrict__ neg_blinds, const unsigned char* __restrict__ blind_inf,
                                            u64* __restrict__ jp, uint32_t* __restrict__ values, unsigned char* __restrict__ infinity) {
  unoffset_store<E>(K, outs, nullptr, jp, values, infinity, [&](size_t i, Jac<E>& m) {
    ld_affine_words<E>(neg_blinds + 16 * E * i, m.X, m.Y);
    return !blind_inf[i];
  });
}

// ---- parity hook (sbn_bn254_fq_batch, tracegen_device.hip): the field helpers above on standard-form operands, 4 words per element --------------
enum { FQB_MUL = 0, FQB_ADD = 1, FQB_SUB = 2, FQB_INV = 3, FQB_BATCH_INV = 4, FQB_FQ2_INV = 5 };
// Item i of op: element i, or group i of TG_INV_BATCH elements for FQB_BATCH_INV.  FQB_INV is finv_fermat on the device and inv_std on
// the host; FQB_FQ2_INV reads c0 from a and c1 from b and writes out[i] = {c0, c1} (8 words).
GL_HD void fq_batch_item(int op, const u64* a, const u64* b, u64* out, size_t i) {
  if (op == FQB_MUL) { from_m(mmul(to_m(a + 4 * i), to_m(b + 4 * i)), out + 4 * i); return; }
  if (op == FQB_ADD || op == FQB_SUB) {
    Fq x, y;
    for (int j = 0; j < 4; j++) { x.l[j] = a[4 * i + j]; y.l[j] = b[4 * i + j]; }
    const Fq r = op == FQB_ADD ? fadd(x, y) : fsub(x, y);
    for (int j = 0; j < 4; j++) out[4 * i + j] = r.l[j];
    return;
  }
  if (op == FQB_INV) {
#if defined(__HIP_DEVICE_COMPILE__)
    from_m(finv_fermat(to_m(a + 4 * i)), out + 4 * i);
#else
    inv_std(a + 4 * i, out + 4 * i);
#endif
    return;
  }
  if (op == FQB_BATCH_INV) {
    Fq v[TG_INV_BATCH];
    for (int j = 0; j < TG_INV_BATCH; j++) v[j] = to_m(a + 4 * (TG_INV_BATCH * i + j));
    batch_inverse(v);
    for (int j = 0; j < TG_INV_BATCH; j++) from_m(v[j], out + 4 * (TG_INV_BATCH * i + j));
    return;
  }
  if (op == FQB_FQ2_INV) {
    Co<2> c; c.c[0] = to_m(a + 4 * i); c.c[1] = to_m(b + 4 * i);
    const Co<2> r = cinv_from_norm(c, finv_fermat(cnorm(c)));
    from_m(r.c[0], out + 8 * i); from_m(r.c[1], out + 8 * i + 4);
  }
}
__global__ void fq_batch_kernel(int op, const u64* __restrict__ a, const u64* __restrict__ b, u64* __restrict__ out, size_t items) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < items) fq_batch_item(op, a, b, out, i);
}

}  // namespace tg
