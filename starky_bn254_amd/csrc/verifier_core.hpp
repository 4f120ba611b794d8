// The verification core (verifier.hip) behind its two callers: sbn_verify (everything on the calling thread) and the batch
// verifier of verifier_device.hip (Merkle hashing and row reductions on the device).  One verification logic: parse, then the
// transcript, then the algebra, which asks a VerifySources for the two kinds of per-query data it does not compute itself.
#pragma once
#include "host_common.hpp"

namespace sbn {

struct VerifyInitial { std::vector<F> evals; std::vector<Digest4> sib; };
struct VerifyStep { std::vector<E2> evals; std::vector<Digest4> sib; };
struct VerifyRound { std::vector<VerifyInitial> init; std::vector<VerifyStep> steps; };

// A parsed proof (verify_parse) and, after verify_challenges, its Fiat-Shamir challenges.
struct VerifyProof {
  AirShape as; sbn_config cfg; FriShape fs;
  u32 degree_bits = 0, lde_bits = 0;
  size_t ncol = 0, nz = 0, nq = 0, npi = 0, nqueries = 0;
  std::vector<Digest4> trace_cap, z_cap, q_cap;
  std::vector<E2> local, next, zs, zs_next, quot;
  std::vector<std::vector<Digest4>> fri_caps;
  std::vector<VerifyRound> rounds;
  std::vector<E2> final_poly;
  F pow_witness;
  std::vector<F> pi;
  // get_challenges
  F gam[2][2] = {};
  F alphas[SBN_NCH];
  E2 zeta, fri_alpha;
  std::vector<E2> betas;
  F pow_response;
  std::vector<size_t> indices;
  // false: the parse checked the opened rows and every sibling word but kept only the FRI evaluations (verify_parse, device_degree_bits)
  bool has_query_rows = true;
  size_t num_initial() const { return nz ? 3 : 2; }   // trace, [permutation Z], quotient
};

// The per-query data the algebra takes from outside.  tree: the initial oracles 0 .. num_initial() - 1, then FRI layer i as
// num_initial() + i.  The core asks in the order of the checks, so a source may compute lazily.
struct VerifySources {
  virtual ~VerifySources() {}
  // verify_merkle_proof_to_cap of the opened leaf of (query, tree)
  virtual bool merkle_ok(size_t query, size_t tree) = 0;
  // P_t = sum_j alpha^j row_t[j] over the opened row of initial oracle t (alpha = the FRI batching challenge)
  virtual E2 row_reduction(size_t query, size_t t) = 0;
};

// Header, shape and canonical-form checks; fills `p` up to the public inputs.  SBN_OK or the code sbn_verify returns (message set).
// device_degree_bits != 0 and equal to the proof's: the opened rows and the siblings are read and checked like everything else but
// not kept (the device reads them from the proof's words): rounds[q].init stays empty and the steps carry no siblings.
int verify_parse(const sbn_air_desc* air, const sbn_config* cfg, const uint8_t* bytes, size_t len, VerifyProof& p, u32 device_degree_bits = 0);
// The transcript: every challenge, the proof-of-work response and the query indices.  Cannot fail.
void verify_challenges(VerifyProof& p);
// Constraints at zeta, proof of work, then per query: initial oracles, per layer fold consistency / evaluation / Merkle path, final polynomial.
int verify_finish(const VerifyProof& p, VerifySources& src);
// verify_finish with both sources computed on the calling thread from the parsed proof (what sbn_verify does; needs has_query_rows).
int verify_finish_host(const VerifyProof& p);

// Where the query answers of a proof of (table, config, degree_bits) lie in its word stream (include/sbn.h): every proof that
// passes verify_parse with this degree_bits has exactly this layout.  Offsets in words.
struct VerifyTree { u32 leaf_off, leaf_len, nsib, cap_off, shift, initial; };   // leaf_off: inside a query's block; siblings follow the leaf; shift: index >> shift
struct VerifyLayout {
  size_t proof_words = 0, query_off = 0, query_stride = 0;
  u32 nqueries = 0, lde_bits = 0, ninit = 0;
  std::vector<VerifyTree> trees;   // initial oracles, then the FRI layers
};
bool verify_layout(const AirShape& as, const sbn_config& cfg, u32 degree_bits, VerifyLayout& L);

// verifier_device.hip, for the guard of a prover context (guard.hip): sbn_verifier_create on `device` instead of the calling
// thread's (device < 0: the calling thread's, which is what the C ABI passes), and the device memory the verifier allocated
int verifier_create_on(int device, const sbn_air_desc* air, const sbn_config* cfg, u32 degree_bits, u32 max_batch, sbn_verifier** out);
size_t verifier_device_bytes(const sbn_verifier* v);

}  // namespace sbn
