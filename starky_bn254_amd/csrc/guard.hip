// Verified proving (include/sbn.h sbn_prover_set_guard): a context with a guard hands every proof it has assembled to a verifier
// before the call returns -- the host verifier (sbn_verify) or a device verifier of batch 1 that the context owns.  What is checked
// is the word array the caller would receive.  The guard runs on the thread of the call, behind the last stage of prove_streamed
// (prover.hip): it enqueues nothing on the prover's streams, takes no lock and shares nothing between contexts, so the contexts of
// a batch prover check side by side (a one-proof call of the device verifier runs its host loops inline: host_parallel_for(1, ...)).
#include "prover_ctx.hpp"
#include "verifier_core.hpp"
#include <chrono>

int guard_check(sbn_prover* P, sbn_proof** out) {
  const auto t0 = std::chrono::steady_clock::now();
  const sbn_air_desc air{(int32_t)P->air.kind, P->air.num_io};
  const uint8_t* bytes = (const uint8_t*)(*out)->words.data();   // sbn_proof_serialize: the words, little-endian
  const size_t len = (*out)->words.size() * sizeof(u64);
  int rc = 0, verdict = 0;
  std::string reason;
  if (P->guard_mode == SBN_GUARD_HOST) {
    if ((verdict = sbn_verify(&air, &P->cfg, bytes, len))) reason = g_last_error;
  } else {
    if (!P->guard_verifier) rc = verifier_create_on(P->device, &air, &P->cfg, P->degree_bits, 1, &P->guard_verifier);
    int32_t status = 0;
    if (!rc) rc = sbn_verifier_verify(P->guard_verifier, &bytes, &len, 1, &status);
    if (!rc && (verdict = status)) reason = sbn_verifier_reason(P->guard_verifier, 0);
  }
  if (!rc) {
    P->guard_checked++;
    if (verdict) P->guard_rejected++;
  }
  P->guard_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  if (!rc && !verdict) return SBN_OK;
  delete *out; *out = nullptr;
  return rc ? rc : fail(verdict, "%s", reason.c_str());   // (rc: the check itself failed, its message is in place)
}

size_t guard_device_bytes(const sbn_prover* P) { return verifier_device_bytes(P->guard_verifier); }
void guard_destroy(sbn_prover* P) { sbn_verifier_destroy(P->guard_verifier); P->guard_verifier = nullptr; }

extern "C" {

int sbn_prover_set_guard(sbn_prover* P, uint32_t mode) {
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (mode > SBN_GUARD_HOST) return fail(SBN_ERR_BAD_ARG, "unknown guard mode %u (0 off, 1 device, 2 host)", mode);
  if (P->sp) return fail(SBN_ERR_UNSUPPORTED, "a guard covers single-GPU provers: the ranks of a split prover would have to agree on the verdict");
  P->guard_mode = mode;   // (the device verifier, once created, stays for the context's lifetime)
  return SBN_OK;
}

int sbn_prover_guard_stats(const sbn_prover* P, uint64_t out[4]) {
  if (!P || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  out[0] = P->guard_checked; out[1] = P->guard_rejected; out[2] = P->guard_ns; out[3] = guard_device_bytes(P);
  return SBN_OK;
}

}  // extern "C"
