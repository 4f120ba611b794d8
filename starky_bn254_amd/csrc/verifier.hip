// Host verifier: replaces starky verifier.rs `verify_stark_proof` (+ get_challenges.rs) and plonky2
// fri/verifier.rs `verify_fri_proof` for the reference's call at src/curves/g1/exp.rs:826.
// The constraint code is the SAME templates the device quotient kernel runs (air.cuh), instantiated
// over the quadratic extension -- as the reference's verifier reuses eval_packed_generic with
// P = F::Extension.  Verification is a few thousand field operations and 84 Merkle paths; it runs on
// the calling thread like the reference's.
#include "verifier_core.hpp"
#include <cstring>

using namespace sbn;

namespace {

struct HostRow {
  const E2* lv; const E2* nv;
  E2 l(int c) const { return lv[c]; }
  E2 n(int c) const { return nv[c]; }
};
struct HostZRow {
  const E2* lz; const E2* nz;
  E2 zl(int z) const { return lz[z]; }
  E2 zn(int z) const { return nz[z]; }
};

struct Reader {
  const u64* w; size_t n, pos = 0; bool ok = true;
  u64 word() { if (pos >= n) { ok = false; return 0; } return w[pos++]; }
  F f() { u64 v = word(); if (v >= GLP) ok = false; return F(v >= GLP ? 0 : v); }
  E2 e() { F a = f(); F b = f(); return E2(a, b); }
  Digest4 d() { Digest4 r; for (int i = 0; i < 4; i++) r.e[i] = f(); return r; }
};

Digest4 hash_or_noop(const F* v, size_t n) {
  Digest4 d;
  if (n <= 4) { for (int i = 0; i < 4; i++) d.e[i] = i < (int)n ? v[i] : F(0); return d; }
  F s[12]; for (auto& x : s) x = F(0);
  for (size_t off = 0; off < n; off += 8) {
    size_t len = n - off < 8 ? n - off : 8;
    for (size_t i = 0; i < len; i++) s[i] = v[off + i];
    poseidon_permute(s);
  }
  for (int i = 0; i < 4; i++) d.e[i] = s[i];
  return d;
}
bool digest_eq(const Digest4& a, const Digest4& b) { for (int i = 0; i < 4; i++) if (a.e[i] != b.e[i]) return false; return true; }
// merkle_proofs.rs `verify_merkle_proof_to_cap`
bool merkle_verify(const F* leaf, size_t leaf_len, size_t index, const std::vector<Digest4>& cap, const std::vector<Digest4>& sib) {
  Digest4 cur = hash_or_noop(leaf, leaf_len);
  for (auto& s : sib) { cur = (index & 1) ? poseidon_two_to_one(s, cur) : poseidon_two_to_one(cur, s); index >>= 1; }
  return index < cap.size() && digest_eq(cur, cap[index]);
}

// fri/verifier.rs `compute_evaluation`: interpolate on the coset and evaluate at beta.
E2 compute_evaluation(F x, size_t within, u32 arity_bits, const std::vector<E2>& evals_in, E2 beta) {
  size_t arity = (size_t)1 << arity_bits;
  F g = f_root_of_unity(arity_bits);
  std::vector<E2> evals(arity);
  for (size_t i = 0; i < arity; i++) evals[bitrev32((u32)i, arity_bits)] = evals_in[i];
  size_t rev = bitrev32((u32)within, arity_bits);
  F start = x * f_pow(g, arity - rev);
  std::vector<F> pts(arity);
  { F y(1); for (size_t i = 0; i < arity; i++) { pts[i] = start * y; y = y * g; } }
  E2 res{F(0), F(0)};
  for (size_t i = 0; i < arity; i++) {
    E2 num{F(1), F(0)}; F den(1);
    for (size_t j = 0; j < arity; j++) if (j != i) { num = num * (beta - pts[j]); den = den * (pts[i] - pts[j]); }
    res = res + evals[i] * num * f_inv(den);
  }
  return res;
}

// both sources from the parsed proof, on the calling thread, when the core asks
struct HostSources : VerifySources {
  const VerifyProof& p;
  explicit HostSources(const VerifyProof& p_) : p(p_) {}
  bool merkle_ok(size_t q, size_t tree) override {
    const VerifyRound& r = p.rounds[q];
    const size_t ninit = p.num_initial();
    if (tree < ninit) {
      const std::vector<Digest4>& cap = tree == 0 ? p.trace_cap : (tree + 1 == ninit ? p.q_cap : p.z_cap);
      return merkle_verify(r.init[tree].evals.data(), r.init[tree].evals.size(), p.indices[q], cap, r.init[tree].sib);
    }
    const size_t i = tree - ninit;
    size_t coset_index = p.indices[q];
    for (size_t k = 0; k <= i; k++) coset_index >>= p.fs.arity_bits[k];
    const VerifyStep& s = r.steps[i];
    std::vector<F> flat(2 * s.evals.size());
    for (size_t j = 0; j < s.evals.size(); j++) { flat[2 * j] = s.evals[j].a; flat[2 * j + 1] = s.evals[j].b; }
    return merkle_verify(flat.data(), flat.size(), coset_index, p.fri_caps[i], s.sib);
  }
  E2 row_reduction(size_t q, size_t t) override {
    const std::vector<F>& v = p.rounds[q].init[t].evals;
    E2 acc{F(0), F(0)};
    for (size_t j = v.size(); j-- > 0;) acc = acc * p.fri_alpha + v[j];
    return acc;
  }
};

}  // namespace

namespace sbn {

int verify_parse(const sbn_air_desc* air, const sbn_config* cfg, const uint8_t* bytes, size_t len, VerifyProof& p, u32 device_degree_bits) {
  if (!air || !cfg || !bytes) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (!config_supported(cfg)) return fail(SBN_ERR_UNSUPPORTED, "unsupported StarkConfig");
  AirShape& as = p.as;
  if (!air_shape(air, cfg, as)) return fail(SBN_ERR_BAD_ARG, "unknown air kind / num_io");
  if (len % 8 || len < 12 * 8) return fail(SBN_ERR_MALFORMED_PROOF, "proof length is not a whole number of words");
  p.cfg = *cfg;
  std::vector<u64> words(len / 8);
  memcpy(words.data(), bytes, len);  // LE host
  Reader rd{words.data(), words.size()};
  // header + validate_proof_shape
  u64 magic = rd.word(), degree_bits = rd.word(), ncol = rd.word(), nz = rd.word(), nq = rd.word(), npi = rd.word(), cap_h = rd.word(),
      rate_bits = rd.word(), nlayers = rd.word(), arity_bits = rd.word(), fpl = rd.word(), nqueries = rd.word();
  if (magic != PROOF_MAGIC) return fail(SBN_ERR_MALFORMED_PROOF, "bad magic");
  if (degree_bits < 1 || degree_bits > 30) return fail(SBN_ERR_MALFORMED_PROOF, "bad degree_bits");
  FriShape& fs = p.fs;
  fs = fri_shape(*cfg, (u32)degree_bits);
  if (ncol != as.ncols || nz != as.nzs || nq != 2 * cfg->num_challenges || npi != as.npi || cap_h != cfg->cap_height || rate_bits != cfg->rate_bits ||
      nlayers != fs.arity_bits.size() || arity_bits != cfg->fri_arity_bits || fpl != fs.final_poly_len() || nqueries != cfg->num_query_rounds)
    return fail(SBN_ERR_MALFORMED_PROOF, "proof shape does not match the table / config");
  if ((is_exp_air(as.kind) || as.kind == SBN_AIR_FLAGS || as.kind == SBN_AIR_FLAGS_U64) && ((u64)exp_rows_per_instance(as.kind) * as.num_io) != ((u64)1 << degree_bits)) return fail(SBN_ERR_MALFORMED_PROOF, "degree_bits does not match num_io");
  const u32 lde_bits = (u32)degree_bits + cfg->rate_bits;
  if (lde_bits < cfg->cap_height + fs.total_arity()) return fail(SBN_ERR_MALFORMED_PROOF, "degree too small for the FRI parameters");
  p.degree_bits = (u32)degree_bits; p.lde_bits = lde_bits; p.ncol = ncol; p.nz = nz; p.nq = nq; p.npi = npi; p.nqueries = nqueries;
  const size_t capn = (size_t)1 << cfg->cap_height;
  auto read_cap = [&](std::vector<Digest4>& c) { c.resize(capn); for (auto& d : c) d = rd.d(); };
  read_cap(p.trace_cap); if (nz) read_cap(p.z_cap); read_cap(p.q_cap);
  auto read_ext = [&](std::vector<E2>& v, size_t k) { v.resize(k); for (auto& e : v) e = rd.e(); };
  read_ext(p.local, ncol); read_ext(p.next, ncol); read_ext(p.zs, nz); read_ext(p.zs_next, nz); read_ext(p.quot, nq);
  p.fri_caps.resize(nlayers);
  for (auto& c : p.fri_caps) read_cap(c);
  if (!rd.ok) return fail(SBN_ERR_MALFORMED_PROOF, "truncated proof or non-canonical element");
  std::vector<size_t> widths; widths.push_back(ncol); if (nz) widths.push_back(nz); widths.push_back(nq);
  const bool lean = device_degree_bits && degree_bits == device_degree_bits;
  p.has_query_rows = !lean;
  p.rounds.resize(nqueries);
  for (auto& r : p.rounds) {
    for (size_t wd : widths) {
      if (lean) { for (size_t k = wd + 4 * (size_t)(lde_bits - cfg->cap_height); k-- > 0;) (void)rd.f(); continue; }
      VerifyInitial in; in.evals.resize(wd); for (auto& v : in.evals) v = rd.f();
      in.sib.resize(lde_bits - cfg->cap_height); for (auto& d : in.sib) d = rd.d();
      r.init.push_back(std::move(in));
    }
    u32 bits = lde_bits;
    for (u32 ab : fs.arity_bits) {
      bits -= ab;
      VerifyStep s; s.evals.resize((size_t)1 << ab); for (auto& e : s.evals) e = rd.e();
      if (lean) for (size_t k = 4 * (size_t)(bits - cfg->cap_height); k-- > 0;) (void)rd.f();
      else { s.sib.resize(bits - cfg->cap_height); for (auto& d : s.sib) d = rd.d(); }
      r.steps.push_back(std::move(s));
    }
    if (!rd.ok) return fail(SBN_ERR_MALFORMED_PROOF, "truncated proof or non-canonical element");
  }
  read_ext(p.final_poly, fpl);
  p.pow_witness = rd.f();
  p.pi.resize(npi); for (auto& v : p.pi) v = rd.f();
  if (!rd.ok || rd.pos != words.size()) return fail(SBN_ERR_MALFORMED_PROOF, "truncated proof, trailing words or non-canonical element");
  return SBN_OK;
}

// get_challenges (starky get_challenges.rs)
void verify_challenges(VerifyProof& p) {
  const sbn_config* cfg = &p.cfg;
  Challenger ch;
  for (auto& d : p.trace_cap) for (int i = 0; i < 4; i++) ch.observe(d.e[i]);
  if (p.nz) {
    for (int s = 0; s < 2; s++) for (u32 c = 0; c < cfg->num_challenges; c++) { (void)ch.challenge(); p.gam[s][c] = ch.challenge(); }
    for (auto& d : p.z_cap) for (int i = 0; i < 4; i++) ch.observe(d.e[i]);
  }
  for (int j = 0; j < SBN_NCH; j++) p.alphas[j] = ch.challenge();
  for (auto& d : p.q_cap) for (int i = 0; i < 4; i++) ch.observe(d.e[i]);
  p.zeta = ch.ext_challenge();
  for (auto& e : p.local) ch.observe(e);
  for (auto& e : p.zs) ch.observe(e);
  for (auto& e : p.quot) ch.observe(e);
  for (auto& e : p.next) ch.observe(e);
  for (auto& e : p.zs_next) ch.observe(e);
  p.fri_alpha = ch.ext_challenge();
  p.betas.clear();
  for (auto& c : p.fri_caps) { for (auto& d : c) for (int i = 0; i < 4; i++) ch.observe(d.e[i]); p.betas.push_back(ch.ext_challenge()); }
  for (auto& e : p.final_poly) ch.observe(e);
  ch.observe(p.pow_witness);
  p.pow_response = ch.challenge();
  p.indices.resize(p.nqueries);
  for (auto& x : p.indices) x = (size_t)(ch.challenge().v % ((u64)1 << p.lde_bits));
}

int verify_finish(const VerifyProof& p, VerifySources& src) {
  const sbn_config* cfg = &p.cfg;
  const AirShape& as = p.as;
  const FriShape& fs = p.fs;
  const u32 degree_bits = p.degree_bits, lde_bits = p.lde_bits;
  const size_t ncol = p.ncol, nz = p.nz, npi = p.npi, nqueries = p.nqueries;
  const E2 zeta = p.zeta, fri_alpha = p.fri_alpha;
  // vanishing polynomial at zeta (verifier.rs verify_stark_proof_with_challenges)
  F g = f_root_of_unity((u32)degree_bits);
  E2 zeta_pow_deg = e2_exp_pow2(zeta, (u32)degree_bits);
  E2 z_h_zeta = zeta_pow_deg - F(1);
  F nn = F((u64)1 << degree_bits);
  Cons<E2> cs;
  std::vector<E2> apow[SBN_NCH];
  for (int j = 0; j < SBN_NCH; j++) {
    apow[j].resize(apow_len(as.nconstraints, as.nzs));
    E2 a{F(1), F(0)}, al(p.alphas[j]);
    for (size_t k = 0; k < apow[j].size(); k++) { apow[j][k] = a; a = a * al; }
    cs.alpha[j] = al; cs.apow[j] = apow[j].data();
  }
  cs.start((int)(as.nconstraints + 2 * nz));   // the AIR's constraints, then nz first-row and nz transition permutation checks
  cs.z_last = zeta - f_inv(g);
  cs.l_first = z_h_zeta * e2_inv((zeta - F(1)) * nn);        // eval_l_0_and_l_last
  cs.l_last = z_h_zeta * e2_inv((zeta * g - F(1)) * nn);
  HostRow row{p.local.data(), p.next.data()};
  HostZRow zrow{p.zs.data(), p.zs_next.data()};
  E2 g0(p.gam[0][0]), g1(p.gam[1][1]);
  if (as.kind == SBN_AIR_G1_OP) {
    g1op_eval(cs, row);
    permutation_checks(cs, row, zrow, G1OpShape(), (int)nz, g0, g1);
  } else if (is_op_air(as.kind)) {
    const OpShape sh(as.kind);
    if (as.kind == SBN_AIR_FQ12_MUL) op_eval<8>(cs, row, sh); else op_eval<7>(cs, row, sh);
    permutation_checks(cs, row, zrow, sh, (int)nz, g0, g1);
  } else if (as.kind == SBN_AIR_LOOKUP) {
    lookup_eval(cs, row);
    permutation_checks(cs, row, zrow, LookupShape(), (int)nz, g0, g1);
  } else if (as.kind == SBN_AIR_FLAGS) {
    flag_eval(cs, row, FlagShape((int)as.num_io));   // no permutation pairs: nz = 0, no Z cap, no permutation challenges
  } else if (as.kind == SBN_AIR_FLAGS_U64) {
    flag_u64_eval(cs, row, FlagU64Shape((int)as.num_io));
  } else {
    ExpShape sh = exp_shape(as);
    std::vector<E2> epi(npi); for (size_t i = 0; i < npi; i++) epi[i] = E2(p.pi[i]);
    static thread_local ExpPiConsts<E2> pic;
    const E2* app[SBN_NCH] = {apow[0].data(), apow[1].data()};
    exp_pi_consts<E2>(sh, app, epi.data(), pic);
    if (sh.E == 1) exp_eval<1>(cs, row, sh, &pic); else if (sh.E == 2) exp_eval<2>(cs, row, sh, &pic); else if (sh.E == 0) exp_eval<0>(cs, row, sh, &pic); else if (sh.E == 13) exp_eval<13>(cs, row, sh, &pic); else exp_eval<12>(cs, row, sh, &pic);
    permutation_checks(cs, row, zrow, sh, (int)nz, g0, g1);
  }
  for (u32 i = 0; i < cfg->num_challenges; i++) {
    // quotient_degree_factor = 2 chunks per challenge: t(zeta) = t0 + zeta^N t1
    E2 t = p.quot[2 * i] + zeta_pow_deg * p.quot[2 * i + 1];
    if (cs.rem != 0) return fail(SBN_ERR_VERIFY_FAILED, "internal: constraint count mismatch (%d left)", cs.rem);
    if (cs.result((int)i) != z_h_zeta * t) return fail(SBN_ERR_VERIFY_FAILED, "mismatch between evaluation and opening of quotient polynomial");
  }

  // verify_fri_proof
  {
    u32 lz = p.pow_response.v ? (u32)__builtin_clzll(p.pow_response.v) : 64;
    if (lz < cfg->proof_of_work_bits) return fail(SBN_ERR_VERIFY_FAILED, "invalid proof of work");
  }
  // batch zeta: trace ++ zs ++ quotient ; batch g*zeta: trace ++ zs
  E2 zeta_next = zeta * g;
  auto reduce = [&](const std::vector<const std::vector<E2>*>& parts) {
    E2 acc{F(0), F(0)};
    for (size_t q = parts.size(); q-- > 0;) for (size_t j = parts[q]->size(); j-- > 0;) acc = acc * fri_alpha + (*parts[q])[j];
    return acc;
  };
  E2 red0 = reduce({&p.local, &p.zs, &p.quot}), red1 = reduce({&p.next, &p.zs_next});
  E2 shift1 = e2_pow(fri_alpha, ncol + nz);
  // the opened rows enter fri_combine_initial as one Horner sum over trace ++ zs ++ quotient: oracle t's own sum P_t times alpha^(columns before it)
  const size_t ninit = p.num_initial();
  E2 init_shift[3] = {E2(F(1), F(0)), e2_pow(fri_alpha, ncol), shift1};
  if (!nz) init_shift[1] = shift1;
  for (size_t q = 0; q < nqueries; q++) {
    size_t x_index = p.indices[q];
    const VerifyRound& r = p.rounds[q];
    for (size_t t = 0; t < ninit; t++)
      if (!src.merkle_ok(q, t))
        return fail(SBN_ERR_VERIFY_FAILED, "invalid Merkle proof (initial oracle %zu, query %zu)", t, q);
    F subgroup_x = F(GL_GEN) * f_pow(f_root_of_unity(lde_bits), bitrev32((u32)x_index, lde_bits));
    // fri_combine_initial
    E2 e0{F(0), F(0)}, e1(F(0), F(0));
    for (size_t t = 0; t < ninit; t++) {
      const E2 pt = src.row_reduction(q, t) * init_shift[t];
      e0 = e0 + pt;
      if (t + 1 < ninit) e1 = e1 + pt;
    }
    E2 sum = (e0 - red0) * e2_inv(E2(subgroup_x) - zeta);
    sum = sum * shift1 + (e1 - red1) * e2_inv(E2(subgroup_x) - zeta_next);
    // plonky2 0.1.x fri_combine_initial: "Multiply the final polynomial by `X`" (PR #436): `sum * subgroup_x`
    E2 old_eval = fri_times_x(*cfg) ? sum * subgroup_x : sum;
    for (size_t i = 0; i < fs.arity_bits.size(); i++) {
      u32 ab = fs.arity_bits[i];
      size_t arity = (size_t)1 << ab, coset_index = x_index >> ab, within = x_index & (arity - 1);
      const VerifyStep& s = r.steps[i];
      if (s.evals[within] != old_eval) return fail(SBN_ERR_VERIFY_FAILED, "FRI fold consistency check failed (query %zu, layer %zu)", q, i);
      old_eval = compute_evaluation(subgroup_x, within, ab, s.evals, p.betas[i]);
      if (!src.merkle_ok(q, ninit + i))
        return fail(SBN_ERR_VERIFY_FAILED, "invalid Merkle proof (FRI layer %zu, query %zu)", i, q);
      subgroup_x = f_exp_pow2(subgroup_x, ab);
      x_index = coset_index;
    }
    E2 fe{F(0), F(0)};
    for (size_t j = p.final_poly.size(); j-- > 0;) fe = fe * E2(subgroup_x) + p.final_poly[j];
    if (fe != old_eval) return fail(SBN_ERR_VERIFY_FAILED, "final polynomial evaluation is invalid (query %zu)", q);
  }
  return SBN_OK;
}

int verify_finish_host(const VerifyProof& p) {
  if (!p.has_query_rows) return fail(SBN_ERR_BAD_ARG, "internal: the parsed proof carries no query rows");
  HostSources src(p);
  return verify_finish(p, src);
}

bool verify_layout(const AirShape& as, const sbn_config& cfg, u32 degree_bits, VerifyLayout& L) {
  const FriShape fs = fri_shape(cfg, degree_bits);
  const u32 lde_bits = degree_bits + cfg.rate_bits;
  if (lde_bits < cfg.cap_height + fs.total_arity()) return false;
  const size_t capn = (size_t)1 << cfg.cap_height, ncol = as.ncols, nz = as.nzs, nq = 2 * (size_t)cfg.num_challenges;
  L.trees.clear();
  L.nqueries = cfg.num_query_rounds; L.lde_bits = lde_bits; L.ninit = nz ? 3 : 2;
  size_t pos = 12;
  std::vector<size_t> cap_off;
  for (u32 t = 0; t < L.ninit; t++) { cap_off.push_back(pos); pos += capn * 4; }
  pos += 2 * (2 * ncol + 2 * nz + nq);
  for (size_t i = 0; i < fs.arity_bits.size(); i++) { cap_off.push_back(pos); pos += capn * 4; }
  L.query_off = pos;
  size_t off = 0;
  const size_t widths[3] = {ncol, nz ? nz : nq, nq};
  for (u32 t = 0; t < L.ninit; t++) {
    VerifyTree v{(u32)off, (u32)widths[t], lde_bits - cfg.cap_height, (u32)cap_off[t], 0, 1};
    L.trees.push_back(v);
    off += v.leaf_len + 4 * (size_t)v.nsib;
  }
  u32 bits = lde_bits, shift = 0;
  for (size_t i = 0; i < fs.arity_bits.size(); i++) {
    const u32 ab = fs.arity_bits[i];
    bits -= ab; shift += ab;
    VerifyTree v{(u32)off, 2u << ab, bits - cfg.cap_height, (u32)cap_off[L.ninit + i], shift, 0};
    L.trees.push_back(v);
    off += v.leaf_len + 4 * (size_t)v.nsib;
  }
  L.query_stride = off;
  pos += off * L.nqueries;
  pos += 2 * fs.final_poly_len() + 1 + as.npi;
  L.proof_words = pos;
  return pos < ((size_t)1 << 32);   // the kernels index a proof with 32-bit word offsets
}

}  // namespace sbn

extern "C" int sbn_verify(const sbn_air_desc* air, const sbn_config* cfg, const uint8_t* bytes, size_t len) {
  VerifyProof p;
  if (int rc = verify_parse(air, cfg, bytes, len, p)) return rc;
  verify_challenges(p);
  return verify_finish_host(p);
}

// Parity hook (include/sbn.h): the table's AIR constraints -- the regrouped templates of air.cuh, here over the base
// field as in the quotient kernel -- folded into the two Horner accumulators on ONE (local, next) row pair.  No
// permutation checks.  Host only; tests compare it with the oracle's constraint-by-constraint evaluation on random rows.
namespace {
struct HostRowF {
  const u64* lv; const u64* nv;
  F l(int c) const { return F(lv[c]); }
  F n(int c) const { return F(nv[c]); }
};
}  // namespace
extern "C" int sbn_eval_constraints_host(const sbn_air_desc* air, const uint64_t* local_row, const uint64_t* next_row, const uint64_t* public_inputs,
                                         size_t n_pi, const uint64_t* alphas, uint64_t z_last, uint64_t l_first, uint64_t l_last, uint64_t* acc_out) {
  if (!air || !local_row || !next_row || !alphas || !acc_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  AirShape as;
  if (!air_shape(air, nullptr, as)) return fail(SBN_ERR_BAD_ARG, "unknown air kind / num_io");
  if (n_pi != as.npi || (n_pi && !public_inputs)) return fail(SBN_ERR_BAD_ARG, "expected %zu public inputs", as.npi);
  for (size_t c = 0; c < as.ncols; c++) if (local_row[c] >= GLP || next_row[c] >= GLP) return fail(SBN_ERR_NON_CANONICAL, "row word %zu is not canonical", c);
  for (size_t i = 0; i < n_pi; i++) if (public_inputs[i] >= GLP) return fail(SBN_ERR_NON_CANONICAL, "public input %zu is not canonical", i);
  if (z_last >= GLP || l_first >= GLP || l_last >= GLP || alphas[0] >= GLP || alphas[1] >= GLP) return fail(SBN_ERR_NON_CANONICAL, "non-canonical scalar");
  Cons<F> cs;
  std::vector<F> apow[SBN_NCH];
  for (int j = 0; j < SBN_NCH; j++) {
    apow[j].resize(apow_len(as.nconstraints, as.nzs));
    F a(1), al(alphas[j]);
    for (size_t k = 0; k < apow[j].size(); k++) { apow[j][k] = a; a = a * al; }
    cs.alpha[j] = al; cs.apow[j] = apow[j].data();
  }
  cs.start((int)as.nconstraints);
  cs.z_last = F(z_last); cs.l_first = F(l_first); cs.l_last = F(l_last);
  HostRowF row{local_row, next_row};
  if (as.kind == SBN_AIR_G1_OP) {
    g1op_eval(cs, row);
  } else if (is_op_air(as.kind)) {
    const OpShape sh(as.kind);
    if (as.kind == SBN_AIR_FQ12_MUL) op_eval<8>(cs, row, sh); else op_eval<7>(cs, row, sh);
  } else if (as.kind == SBN_AIR_LOOKUP) {
    lookup_eval(cs, row);
  } else if (as.kind == SBN_AIR_FLAGS) {
    flag_eval(cs, row, FlagShape((int)as.num_io));
  } else if (as.kind == SBN_AIR_FLAGS_U64) {
    flag_u64_eval(cs, row, FlagU64Shape((int)as.num_io));
  } else {
    ExpShape sh = exp_shape(as);
    std::vector<F> fpi(n_pi); for (size_t i = 0; i < n_pi; i++) fpi[i] = F(public_inputs[i]);
    static thread_local ExpPiConsts<F> pic;
    const F* app[SBN_NCH] = {apow[0].data(), apow[1].data()};
    exp_pi_consts<F>(sh, app, fpi.data(), pic);
    if (sh.E == 1) exp_eval<1>(cs, row, sh, &pic); else if (sh.E == 2) exp_eval<2>(cs, row, sh, &pic); else if (sh.E == 0) exp_eval<0>(cs, row, sh, &pic);
    else if (sh.E == 13) exp_eval<13>(cs, row, sh, &pic); else exp_eval<12>(cs, row, sh, &pic);
  }
  if (cs.rem != 0) return fail(SBN_ERR_HIP, "internal: the evaluator emitted %d constraints fewer than the table declares", cs.rem);
  for (int j = 0; j < SBN_NCH; j++) acc_out[j] = cs.result(j).v;
  return SBN_OK;
}
