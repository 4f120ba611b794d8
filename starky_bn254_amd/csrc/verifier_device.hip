// Batch verifier (include/sbn.h sbn_verifier_*): the verification core of verifier.hip with its two per-query data sources -- the
// Merkle checks and the alpha-reductions of the opened rows -- computed on the device for a whole batch of proofs
// (kernels_verify.cuh), everything sequential or tiny on the host.  Per call:
//   1. every proof is parsed on the host pool (verify_parse: the codes and messages of sbn_verify; the opened rows and siblings
//      are checked but not copied); a proof that fails keeps its code and is not uploaded;
//   2. a copy thread moves the others through a pinned ring into the verifier's device buffer while the pool runs their
//      transcripts (verify_challenges: ~1,220 dependent permutations per G1ExpStark(128) proof);
//   3. query indices, alpha and alpha^8 go up, one kernel launch checks every (proof, query, tree), the pass / fail bytes and
//      the partial sums come back;
//   4. the pool finishes every proof with verify_finish, which asks for those results in the order sbn_verify computes them,
//      so the first failing check, its code and its message are the same.
// A proof that parses but names another degree_bits than the verifier's has another layout: it is finished with the host
// sources (the same verdict; nothing of it is uploaded).
#include "verifier_core.hpp"
#include "kernels_verify.cuh"
#include "pinned_ring.hpp"
#include <cstring>
#include <thread>

using namespace sbn;

#define VHIPC(expr)                                                                                                         \
  do {                                                                                                                      \
    hipError_t e_ = (expr);                                                                                                 \
    if (e_ != hipSuccess) return fail(SBN_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

static constexpr unsigned VERIFY_SLOTS = 4;
static constexpr size_t VERIFY_SLOT_WORDS = (size_t)1 << 19;   // 4 MiB per slot of the pinned ring
static constexpr uint32_t VERIFY_MAX_BATCH = 1u << 16;

struct sbn_verifier {
  sbn_air_desc air; sbn_config cfg; AirShape as;
  u32 degree_bits = 0, max_batch = 0;
  int device = 0;
  VerifyLayout L;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {};
  PinnedRing ring;   // the proofs' way up (pinned_ring.hpp)
  u64 *d_proofs = nullptr, *d_alpha = nullptr, *d_psum = nullptr, *h_alpha = nullptr, *h_psum = nullptr;
  u32 *d_idx = nullptr, *h_idx = nullptr;
  unsigned char *d_ok = nullptr, *h_ok = nullptr;
  VerifyTreeDev* d_trees = nullptr;
  float stage_ms[3] = {0, 0, 0};   // upload, kernels, download of the last call
  size_t dev_bytes = 0;            // device memory of the buffers above
  std::vector<std::string> reasons;
};

namespace {

struct DeviceSources : VerifySources {
  const unsigned char* ok; const u64* psum; size_t ntrees, ninit;
  bool merkle_ok(size_t q, size_t tree) override { return ok[q * ntrees + tree] != 0; }
  E2 row_reduction(size_t q, size_t t) override { const u64* s = psum + (q * ninit + t) * 2; return E2(F(s[0]), F(s[1])); }
};

// proofs[act[0 .. n)] -> d_proofs[0 .. n), through the pinned ring (the caller's memory is only read, never pinned)
int upload_proofs(sbn_verifier* V, const uint8_t* const* proofs, const std::vector<size_t>& act) {
  VHIPC(hipSetDevice(V->device));
  const size_t pw = V->L.proof_words;
  for (size_t a = 0; a < act.size(); a++)
    for (size_t w0 = 0; w0 < pw; w0 += VERIFY_SLOT_WORDS) {
      const size_t len = std::min(VERIFY_SLOT_WORDS, pw - w0);
      u64* slot; unsigned s;
      VHIPC(V->ring.claim(&slot, &s));
      memcpy(slot, proofs[act[a]] + w0 * 8, len * 8);
      VHIPC(hipMemcpyAsync(V->d_proofs + a * pw + w0, slot, len * 8, hipMemcpyHostToDevice, V->stream));
      VHIPC(V->ring.sent(s, V->stream));
    }
  return 0;
}

}  // namespace

extern "C" {

void sbn_verifier_destroy(sbn_verifier* V) {
  if (!V) return;
  if (V->stream || V->d_proofs || V->ring.base) {
    (void)hipSetDevice(V->device);
    if (V->stream) (void)hipStreamSynchronize(V->stream);
  }
  V->ring.destroy();
  for (auto e : V->ev) if (e) (void)hipEventDestroy(e);
  if (V->d_proofs) (void)hipFree(V->d_proofs);
  if (V->d_alpha) (void)hipFree(V->d_alpha);
  if (V->d_psum) (void)hipFree(V->d_psum);
  if (V->d_idx) (void)hipFree(V->d_idx);
  if (V->d_ok) (void)hipFree(V->d_ok);
  if (V->d_trees) (void)hipFree(V->d_trees);
  if (V->h_alpha) (void)hipHostFree(V->h_alpha);
  if (V->h_psum) (void)hipHostFree(V->h_psum);
  if (V->h_idx) (void)hipHostFree(V->h_idx);
  if (V->h_ok) (void)hipHostFree(V->h_ok);
  if (V->stream) (void)hipStreamDestroy(V->stream);
  delete V;
}

int sbn_verifier_create(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, uint32_t max_batch, sbn_verifier** out) {
  return verifier_create_on(-1, air, cfg, degree_bits, max_batch, out);
}

}  // extern "C"

size_t sbn::verifier_device_bytes(const sbn_verifier* V) { return V ? V->dev_bytes : 0; }

int sbn::verifier_create_on(int device, const sbn_air_desc* air, const sbn_config* cfg, u32 degree_bits, u32 max_batch, sbn_verifier** out) {
  if (!air || !cfg || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  *out = nullptr;
  if (!config_supported(cfg)) return fail(SBN_ERR_UNSUPPORTED, "unsupported StarkConfig");
  AirShape as;
  if (!air_shape(air, cfg, as)) return fail(SBN_ERR_BAD_ARG, "unknown air kind / num_io");
  if (max_batch == 0 || max_batch > VERIFY_MAX_BATCH) return fail(SBN_ERR_BAD_ARG, "bad arguments (1 <= max_batch <= %u)", VERIFY_MAX_BATCH);
  if (!height_supported(cfg, degree_bits)) return fail(SBN_ERR_UNSUPPORTED, "%s", HEIGHT_REFUSAL);
  if ((is_exp_air(as.kind) || as.kind == SBN_AIR_FLAGS || as.kind == SBN_AIR_FLAGS_U64) && (exp_rows_per_instance(as.kind) * as.num_io) != ((size_t)1 << degree_bits))
    return fail(SBN_ERR_BAD_ARG, "degree_bits does not match num_io");
  VerifyLayout L;
  if (!verify_layout(as, *cfg, degree_bits, L)) return fail(SBN_ERR_UNSUPPORTED, "degree too small for the FRI parameters");
  if (int rc = use_current_device("sbn_verify is the host verifier")) return rc;
  if (device >= 0) VHIPC(hipSetDevice(device));   // (a prover context's guard: the context's device, whatever the calling thread selected)
  sbn_verifier* V = new sbn_verifier();
  V->air = *air; V->cfg = *cfg; V->as = as; V->degree_bits = degree_bits; V->max_batch = max_batch; V->device = device >= 0 ? device : current_device(); V->L = L;
  int rc = 0;
  auto hipc = [&](hipError_t e, const char* what) { if (e != hipSuccess && !rc) rc = fail(SBN_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e)); };
  const size_t B = max_batch, nq = L.nqueries, nt = L.trees.size();
  V->dev_bytes = B * L.proof_words * sizeof(u64) + B * 4 * sizeof(u64) + B * nq * L.ninit * 2 * sizeof(u64) + B * nq * sizeof(u32) + B * nq * nt + nt * sizeof(VerifyTreeDev);   // the six hipMallocs below
  hipc(hipStreamCreate(&V->stream), "hipStreamCreate");
  for (auto& e : V->ev) hipc(hipEventCreate(&e), "hipEventCreate");
  hipc(hipMalloc((void**)&V->d_proofs, B * L.proof_words * sizeof(u64)), "hipMalloc (proofs)");
  hipc(hipMalloc((void**)&V->d_alpha, B * 4 * sizeof(u64)), "hipMalloc");
  hipc(hipMalloc((void**)&V->d_psum, B * nq * L.ninit * 2 * sizeof(u64)), "hipMalloc");
  hipc(hipMalloc((void**)&V->d_idx, B * nq * sizeof(u32)), "hipMalloc");
  hipc(hipMalloc((void**)&V->d_ok, B * nq * nt), "hipMalloc");
  hipc(hipMalloc((void**)&V->d_trees, nt * sizeof(VerifyTreeDev)), "hipMalloc");
  hipc(V->ring.create(VERIFY_SLOTS, VERIFY_SLOT_WORDS), "the pinned ring");
  hipc(hipHostMalloc((void**)&V->h_alpha, B * 4 * sizeof(u64), hipHostMallocDefault), "hipHostMalloc");
  hipc(hipHostMalloc((void**)&V->h_psum, B * nq * L.ninit * 2 * sizeof(u64), hipHostMallocDefault), "hipHostMalloc");
  hipc(hipHostMalloc((void**)&V->h_idx, B * nq * sizeof(u32), hipHostMallocDefault), "hipHostMalloc");
  hipc(hipHostMalloc((void**)&V->h_ok, B * nq * nt, hipHostMallocDefault), "hipHostMalloc");
  if (!rc) {
    std::vector<VerifyTreeDev> td(nt);
    for (size_t t = 0; t < nt; t++) { const VerifyTree& s = L.trees[t]; td[t] = VerifyTreeDev{s.leaf_off, s.leaf_len, s.nsib, s.cap_off, s.shift, s.initial}; }
    hipc(hipMemcpy(V->d_trees, td.data(), nt * sizeof(VerifyTreeDev), hipMemcpyHostToDevice), "hipMemcpy");
  }
  if (rc) { const std::string msg = g_last_error; sbn_verifier_destroy(V); g_last_error = msg; return rc; }
  *out = V;
  return SBN_OK;
}

extern "C" {

int sbn_verifier_verify(sbn_verifier* V, const uint8_t* const* proofs, const size_t* lens, size_t count, int32_t* status_out) {
  if (!V || !proofs || !lens || !status_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (count == 0 || count > V->max_batch) return fail(SBN_ERR_BAD_ARG, "count must be between 1 and max_batch = %u", V->max_batch);
  VHIPC(hipSetDevice(V->device));
  const VerifyLayout& L = V->L;
  const size_t nq = L.nqueries, nt = L.trees.size(), ninit = L.ninit;
  std::vector<VerifyProof> P(count);
  std::vector<int> rc(count, 0);
  std::vector<std::string> reasons(count);
  host_parallel_for(count, [&](size_t i) {
    rc[i] = verify_parse(&V->air, &V->cfg, proofs[i], lens[i], P[i], V->degree_bits);
    if (rc[i]) reasons[i] = g_last_error;
  });
  std::vector<size_t> act, other;   // on the device / parsed, but of another height: host sources
  for (size_t i = 0; i < count; i++)
    if (!rc[i]) {
      // (a proof of this table, config and degree_bits that parses has the layout's length: the parse read exactly these words)
      if (!P[i].has_query_rows && lens[i] != L.proof_words * 8) return fail(SBN_ERR_HIP, "internal: proof %zu does not have the verifier's layout", i);
      (P[i].has_query_rows ? other : act).push_back(i);
    }
  const size_t na = act.size();
  V->stage_ms[0] = V->stage_ms[1] = V->stage_ms[2] = 0;
  if (na) {
    VHIPC(hipEventRecord(V->ev[0], V->stream));
    int up_rc = 0; std::string up_msg;
    std::thread up([&] { up_rc = upload_proofs(V, proofs, act); if (up_rc) up_msg = g_last_error; });
    host_parallel_for(na + other.size(), [&](size_t k) { verify_challenges(P[k < na ? act[k] : other[k - na]]); });
    up.join();
    if (up_rc) { (void)hipStreamSynchronize(V->stream); return fail(up_rc, "%s", up_msg.c_str()); }
    for (size_t a = 0; a < na; a++) {
      const VerifyProof& p = P[act[a]];
      for (size_t q = 0; q < nq; q++) V->h_idx[a * nq + q] = (u32)p.indices[q];
      const E2 al = p.fri_alpha, a2 = al * al, a4 = a2 * a2, a8 = a4 * a4;
      u64* h = V->h_alpha + a * 4;
      h[0] = al.a.v; h[1] = al.b.v; h[2] = a8.a.v; h[3] = a8.b.v;
    }
    VHIPC(hipMemcpyAsync(V->d_idx, V->h_idx, na * nq * sizeof(u32), hipMemcpyHostToDevice, V->stream));
    VHIPC(hipMemcpyAsync(V->d_alpha, V->h_alpha, na * 4 * sizeof(u64), hipMemcpyHostToDevice, V->stream));
    VHIPC(hipEventRecord(V->ev[1], V->stream));
    VerifyKernelParams kp;
    kp.proofs = V->d_proofs; kp.indices = V->d_idx; kp.alpha = V->d_alpha; kp.trees = V->d_trees; kp.ok = V->d_ok; kp.psum = V->d_psum;
    kp.proof_words = L.proof_words; kp.query_off = L.query_off; kp.query_stride = L.query_stride;
    kp.nproofs = (u32)na; kp.nqueries = (u32)nq; kp.ntrees = (u32)nt; kp.ninit = (u32)ninit; kp.lde_bits = L.lde_bits;
    kp.cap_mask = (1u << V->cfg.cap_height) - 1u;
    const size_t items = na * nq;
    hipLaunchKernelGGL(verify_items_kernel, dim3((unsigned)((items + 15) / 16), (unsigned)nt), dim3(256), 0, V->stream, kp);
    VHIPC(hipGetLastError());
    VHIPC(hipEventRecord(V->ev[2], V->stream));
    VHIPC(hipMemcpyAsync(V->h_ok, V->d_ok, items * nt, hipMemcpyDeviceToHost, V->stream));
    VHIPC(hipMemcpyAsync(V->h_psum, V->d_psum, items * ninit * 2 * sizeof(u64), hipMemcpyDeviceToHost, V->stream));
    VHIPC(hipEventRecord(V->ev[3], V->stream));
    VHIPC(hipStreamSynchronize(V->stream));
    for (int s = 0; s < 3; s++) VHIPC(hipEventElapsedTime(&V->stage_ms[s], V->ev[s], V->ev[s + 1]));
  } else {
    if (!other.empty()) host_parallel_for(other.size(), [&](size_t k) { verify_challenges(P[other[k]]); });
  }
  if (na + other.size()) host_parallel_for(na + other.size(), [&](size_t k) {
    const size_t i = k < na ? act[k] : other[k - na];
    if (k < na) {
      DeviceSources src;
      src.ok = V->h_ok + k * nq * nt; src.psum = V->h_psum + k * nq * ninit * 2; src.ntrees = nt; src.ninit = ninit;
      rc[i] = verify_finish(P[i], src);
    } else rc[i] = verify_finish_host(P[i]);
    if (rc[i]) reasons[i] = g_last_error;
  });
  V->reasons.swap(reasons);
  for (size_t i = 0; i < count; i++) status_out[i] = rc[i];
  return SBN_OK;
}

const char* sbn_verifier_reason(const sbn_verifier* V, size_t i) { return V && i < V->reasons.size() ? V->reasons[i].c_str() : ""; }

int sbn_verifier_stage_times(const sbn_verifier* V, float* ms_out, int cap) {
  if (!V || !ms_out) return 0;
  int n = cap < 3 ? (cap < 0 ? 0 : cap) : 3;
  for (int s = 0; s < n; s++) ms_out[s] = V->stage_ms[s];
  return n;
}

}  // extern "C"
