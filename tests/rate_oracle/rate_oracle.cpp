// The CPU oracle at a chosen rate_bits -- TEST INFRASTRUCTURE ONLY.  oracle/capi.cpp's make_config carries no rate_bits word; the
// oracle's stark.hpp / fri.hpp / poly.hpp are general in it.  This unit includes capi.cpp (for its static make_air / make_config)
// and adds orc_prove_cfg / orc_verify_cfg with cfg.fri.rate_bits set from an argument.  tests/rate_oracle.py builds and binds it.
#include "../../oracle/capi.cpp"

extern "C" {

int orc_prove_rate(int kind, size_t num_io, const uint64_t* trace, unsigned degree_bits, const uint64_t* pi, size_t npi, const uint32_t* config,
                   unsigned rate_bits, uint64_t** proof_out, size_t* nwords_out, double* seconds_out) {
  auto air = make_air(kind, num_io);
  if (!air) return -1;
  size_t n = (size_t)1 << degree_bits, ncols = air->num_columns();
  if (npi != air->num_public_inputs()) return -2;
  std::vector<std::vector<GF>> cols(ncols, std::vector<GF>(n));
  for (size_t c = 0; c < ncols; c++) for (size_t i = 0; i < n; i++) { if (trace[c * n + i] >= GL_P) return -3; cols[c][i] = GF(trace[c * n + i]); }
  std::vector<GF> pis(npi); for (size_t i = 0; i < npi; i++) pis[i] = GF(pi[i]);
  StarkConfig cfg = make_config(config);
  cfg.fri.rate_bits = rate_bits;
  auto t0 = std::chrono::steady_clock::now();
  StarkProofWithPublicInputs p = prove(*air, cfg, cols, pis);
  auto t1 = std::chrono::steady_clock::now();
  if (seconds_out) *seconds_out = std::chrono::duration<double>(t1 - t0).count();
  std::vector<u64> w = serialize_proof(p, cfg);
  *proof_out = (uint64_t*)malloc(w.size() * 8);
  memcpy(*proof_out, w.data(), w.size() * 8);
  *nwords_out = w.size();
  return 0;
}

// 0 = accepted; negative = rejected (message in *why)
int orc_verify_rate(int kind, size_t num_io, const uint64_t* proof, size_t nwords, const uint32_t* config, unsigned rate_bits, const char** why) {
  static const char* w0 = ""; if (why) *why = w0;
  auto air = make_air(kind, num_io);
  if (!air) { if (why) *why = "unknown air"; return -1; }
  StarkProofWithPublicInputs p;
  if (!deserialize_proof(proof, nwords, p)) { if (why) *why = "malformed proof bytes"; return -2; }
  StarkConfig cfg = make_config(config);
  cfg.fri.rate_bits = rate_bits;
  const char* reason = "";
  if (!verify(*air, cfg, p, &reason)) { if (why) *why = reason; return -3; }
  return 0;
}

}  // extern "C"
