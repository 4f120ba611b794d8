// C ABI glue (include/sbn.h): configuration, table shapes, proof object, one-shot prove().
#include "host_common.hpp"
#include <cstring>
#include <atomic>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

using namespace sbn;

// ---- the context cache of the one-shot call (include/sbn.h sbn_prove_cache_configure) ---------------------------------
// Idle contexts only: a context leaves the list while a call works on it, so two threads never share one, and a thread that
// finds its key busy creates a temporary context instead of waiting.  bytes = the idle contexts' device memory <= budget at
// every return; what does not fit when it comes back is destroyed.  The list lives on the heap and is never destroyed by a
// static destructor (the HIP runtime may be gone by then): sbn_prove_cache_configure(0) releases the contexts.
namespace {
struct CacheKey {
  int device; int32_t kind; uint32_t num_io, degree_bits; sbn_config cfg;
  bool operator==(const CacheKey& o) const {
    return device == o.device && kind == o.kind && num_io == o.num_io && degree_bits == o.degree_bits && cfg.security_bits == o.cfg.security_bits &&
           cfg.num_challenges == o.cfg.num_challenges && cfg.rate_bits == o.cfg.rate_bits && cfg.cap_height == o.cfg.cap_height &&
           cfg.proof_of_work_bits == o.cfg.proof_of_work_bits && cfg.fri_arity_bits == o.cfg.fri_arity_bits &&
           cfg.fri_final_poly_bits == o.cfg.fri_final_poly_bits && cfg.num_query_rounds == o.cfg.num_query_rounds && cfg.fri_variant == o.cfg.fri_variant;
  }
};
struct CacheEntry { CacheKey key; sbn_prover* P; uint64_t bytes; };
struct ProveCache {
  std::mutex m;
  std::vector<CacheEntry> idle;   // least recently used first
  uint64_t budget = 0, bytes = 0, hits = 0, misses = 0, evictions = 0;
};
ProveCache& prove_cache() { static ProveCache* c = new ProveCache(); return *c; }
// the guard of the one-shot calls (include/sbn.h sbn_prove_set_guard): process-wide, given to the context of every call
std::atomic<uint32_t> g_one_shot_guard{SBN_GUARD_OFF};

// an idle context of this key, or null (counted as a miss: the caller creates one)
sbn_prover* cache_take(const CacheKey& key) {
  ProveCache& c = prove_cache();
  std::lock_guard<std::mutex> g(c.m);
  if (c.budget == 0) return nullptr;   // the cache is off: nothing is counted
  for (size_t i = 0; i < c.idle.size(); i++)
    if (c.idle[i].key == key) {
      sbn_prover* P = c.idle[i].P;
      c.bytes -= c.idle[i].bytes;
      c.idle.erase(c.idle.begin() + (long)i);
      c.hits++;
      return P;
    }
  c.misses++;
  return nullptr;
}
// after a successful call: keep the context if the budget allows (evicting the least recently used), else destroy it
void cache_give(const CacheKey& key, sbn_prover* P) {
  ProveCache& c = prove_cache();
  const uint64_t bytes = prover_device_bytes(P);
  std::vector<sbn_prover*> drop;
  {
    std::lock_guard<std::mutex> g(c.m);
    if (bytes > c.budget) drop.push_back(P);   // (the cache is off, or the context alone exceeds the budget)
    else {
      while (c.bytes + bytes > c.budget) {
        drop.push_back(c.idle.front().P); c.bytes -= c.idle.front().bytes; c.idle.erase(c.idle.begin()); c.evictions++;
      }
      c.idle.push_back(CacheEntry{key, P, bytes});
      c.bytes += bytes;
    }
  }
  for (sbn_prover* q : drop) sbn_prover_destroy(q);   // outside the lock: freeing 6.5 GB takes milliseconds
}
}  // namespace

extern "C" {

int sbn_prove_cache_configure(uint64_t budget_bytes) {
  ProveCache& c = prove_cache();
  std::vector<sbn_prover*> drop;
  {
    std::lock_guard<std::mutex> g(c.m);
    c.budget = budget_bytes;
    while (!c.idle.empty() && (budget_bytes == 0 || c.bytes > budget_bytes)) {
      drop.push_back(c.idle.front().P); c.bytes -= c.idle.front().bytes; c.idle.erase(c.idle.begin());
      if (budget_bytes) c.evictions++;
    }
  }
  for (sbn_prover* q : drop) sbn_prover_destroy(q);
  return SBN_OK;
}
int sbn_prove_cache_stats(uint64_t out[6]) {
  if (!out) return fail(SBN_ERR_BAD_ARG, "null argument");
  ProveCache& c = prove_cache();
  std::lock_guard<std::mutex> g(c.m);
  out[0] = c.hits; out[1] = c.misses; out[2] = c.evictions; out[3] = c.idle.size(); out[4] = c.bytes; out[5] = c.budget;
  return SBN_OK;
}

int sbn_prove_set_guard(uint32_t mode) {
  if (mode > SBN_GUARD_HOST) return fail(SBN_ERR_BAD_ARG, "unknown guard mode %u (0 off, 1 device, 2 host)", mode);
  g_one_shot_guard.store(mode);
  return SBN_OK;
}

const char* sbn_version(void) { return "starky-bn254-amd 0.3 (gfx950)"; }
int sbn_abi_version(void) { return SBN_ABI_VERSION; }
const char* sbn_last_error(void) { return g_last_error.c_str(); }

// starky config.rs `StarkConfig::standard_fast_config` (the reference passes the column / public-input
// counts at run time, src/curves/g1/exp.rs:250-253; here they come from the table descriptor).
void sbn_standard_fast_config(sbn_config* c) {
  if (!c) return;
  c->security_bits = 100; c->num_challenges = 2; c->rate_bits = 1; c->cap_height = 4; c->proof_of_work_bits = 16;
  c->fri_arity_bits = 4; c->fri_final_poly_bits = 5; c->num_query_rounds = 84;
  c->fri_variant = SBN_FRI_TIMES_X;
}
// the same security from another blowup: rate_bits * num_query_rounds + proof_of_work_bits >= security_bits
void sbn_config_for_rate(uint32_t rate_bits, sbn_config* c) {
  if (!c) return;
  sbn_standard_fast_config(c);
  if (rate_bits == 0) rate_bits = 1;
  c->rate_bits = rate_bits;
  c->num_query_rounds = (c->security_bits - c->proof_of_work_bits + rate_bits - 1) / rate_bits;
}

size_t sbn_air_num_columns(const sbn_air_desc* air) { AirShape s; return air_shape(air, nullptr, s) ? s.ncols : 0; }
size_t sbn_air_num_public_inputs(const sbn_air_desc* air) { AirShape s; return air_shape(air, nullptr, s) ? s.npi : 0; }
size_t sbn_air_num_permutation_zs(const sbn_air_desc* air, const sbn_config* cfg) { AirShape s; return air_shape(air, cfg, s) ? s.nzs : 0; }
size_t sbn_air_num_constraints(const sbn_air_desc* air) { AirShape s; return air_shape(air, nullptr, s) ? s.nconstraints : 0; }

size_t sbn_proof_num_words(const sbn_proof* p) { return p ? p->words.size() : 0; }
const uint64_t* sbn_proof_words(const sbn_proof* p) { return p ? p->words.data() : nullptr; }
size_t sbn_proof_serialize(const sbn_proof* p, uint8_t* buf, size_t cap) {
  if (!p) return 0;
  size_t need = p->words.size() * 8;
  if (buf && cap >= need) memcpy(buf, p->words.data(), need);  // little-endian host
  return need;
}
uint32_t sbn_proof_degree_bits(const sbn_proof* p) { return p ? p->degree_bits : 0; }
void sbn_proof_free(sbn_proof* p) { delete p; }

// the one-shot call on a context of the cache (or a fresh one): `call` is the prover call with the caller's trace
static int prove_one_shot(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, sbn_proof** out, const std::function<int(sbn_prover*)>& call) {
  if (!out) return fail(SBN_ERR_BAD_ARG, "null argument");
  *out = nullptr;
  CacheKey key{};
  const bool keyed = air && cfg;   // (null arguments: sbn_prover_create reports them)
  if (keyed) { key.device = current_device(); key.kind = air->kind; key.num_io = air->num_io; key.degree_bits = degree_bits; key.cfg = *cfg; }
  sbn_prover* P = keyed ? cache_take(key) : nullptr;
  int rc = 0;
  if (!P && (rc = sbn_prover_create(air, cfg, degree_bits, &P))) return rc;
  rc = sbn_prover_set_guard(P, g_one_shot_guard.load());   // (a cached context may carry the mode of an earlier call; its verifier stays)
  if (!rc) rc = call(P);
  if (rc) {   // a context whose call failed is not kept (destroy leaves the message of the failure in place)
    const std::string msg = g_last_error;
    sbn_prover_destroy(P);
    g_last_error = msg;
    return rc;
  }
  cache_give(key, P);
  return rc;
}
int sbn_prove(const sbn_air_desc* air, const sbn_config* cfg, const uint64_t* trace, uint32_t degree_bits, const uint64_t* pi, size_t n_pi,
              sbn_proof** out) {
  return prove_one_shot(air, cfg, degree_bits, out, [&](sbn_prover* P) {
    if (!trace) return fail(SBN_ERR_BAD_ARG, "null argument");
    return sbn_prover_prove_host_trace(P, trace, pi, n_pi, out);
  });
}
// sbn_prove for a trace held as one allocation per column (sbn_prover_prove_host_columns): the same cache, key and statistics
int sbn_prove_columns(const sbn_air_desc* air, const sbn_config* cfg, const uint64_t* const* columns, size_t n_columns, uint32_t degree_bits, uint32_t flags,
                      const uint64_t* pi, size_t n_pi, sbn_proof** out) {
  return prove_one_shot(air, cfg, degree_bits, out, [&](sbn_prover* P) { return sbn_prover_prove_host_columns(P, columns, n_columns, flags, pi, n_pi, nullptr, out); });
}
// sbn_prove for a row-major trace (sbn_prover_prove_host_rows): the same cache, key and statistics; the refusals that need no prover
// run first, so a bad call never creates a context (or looks for a device)
int sbn_prove_rows(const sbn_air_desc* air, const sbn_config* cfg, const sbn_host_rows* rows, uint32_t flags, const uint64_t* pi, size_t n_pi, sbn_proof** out) {
  if (out) *out = nullptr;
  if (!air || !cfg || !rows || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  uint32_t degree_bits = 0;
  if (int rc = host_rows_precheck(air, rows, flags, pi, n_pi, &degree_bits)) return rc;
  return prove_one_shot(air, cfg, degree_bits, out, [&](sbn_prover* P) { return sbn_prover_prove_host_rows(P, rows, flags, pi, n_pi, nullptr, out); });
}

// ---- batch mode (BASELINE config[2]: a batch of independent proofs per GPU) -------------------------------------------
// `inflight` prover contexts on the current GPU, one host thread each; every unit = one instance list of the table,
// witness generated on the device, then proved.  While one proof sits in a latency-bound tail or waits for the host
// transcript, the kernels of the others fill the GPU (30.7 instead of 26.5 proofs/s for G1ExpStark(128)).
struct sbn_batch_prover { std::vector<sbn_prover*> provers; int kind = 0; uint32_t num_io = 0; };

int sbn_batch_prover_create(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, uint32_t inflight, sbn_batch_prover** out) {
  return sbn_batch_prover_create_with(air, cfg, degree_bits, inflight, nullptr, out);
}
// opt: every context of the batch is created with it (sbn_prover_create_with checks it)
int sbn_batch_prover_create_with(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, uint32_t inflight, const sbn_prover_options* opt,
                                 sbn_batch_prover** out) {
  if (!out || inflight == 0 || inflight > 16) return fail(SBN_ERR_BAD_ARG, "bad arguments (1 <= inflight <= 16)");
  *out = nullptr;
  if (!air) return fail(SBN_ERR_BAD_ARG, "null argument");
  sbn_batch_prover* B = new sbn_batch_prover();
  B->kind = air->kind; B->num_io = air->num_io;
  for (uint32_t i = 0; i < inflight; i++) {
    sbn_prover* P = nullptr;
    int rc = sbn_prover_create_with(air, cfg, degree_bits, opt, &P);
    if (rc) { for (auto q : B->provers) sbn_prover_destroy(q); delete B; return rc; }
    B->provers.push_back(P);
  }
  *out = B;
  return SBN_OK;
}
void sbn_batch_prover_destroy(sbn_batch_prover* B) {
  if (!B) return;
  for (auto q : B->provers) sbn_prover_destroy(q);
  delete B;
}
// The unit loop of the batch calls: context 0 works on the caller's thread, context i on thread i (min(contexts, count) threads),
// and each takes the next unit -- unit(P, u) is witness, then proof, of unit u on context P -- until one fails.  The failure
// rule: the failing unit with the smallest index, its message behind "unit %zu: ", and every proof slot nulled (a guarded context
// fails a unit whose proof its verifier rejects, on the thread that proved it).
static int prove_units(sbn_batch_prover* B, size_t count, sbn_proof** proofs_out, const std::function<int(sbn_prover*, size_t)>& unit) {
  std::atomic<size_t> next(0), first_unit(count);
  std::mutex m; int first_rc = 0; std::string msg;
  auto work = [&](sbn_prover* P) {
    for (size_t u; (u = next.fetch_add(1)) < count && first_unit.load() == count;) {
      const int rc = unit(P, u);
      if (rc) { std::lock_guard<std::mutex> g(m); if (u < first_unit.load()) { first_unit = u; first_rc = rc; msg = g_last_error; } }
    }
  };
  std::vector<std::thread> th;
  for (size_t i = 1; i < B->provers.size() && i < count; i++) th.emplace_back(work, B->provers[i]);
  work(B->provers[0]);
  for (auto& t : th) t.join();
  if (first_rc) {
    for (size_t i = 0; i < count; i++) { delete proofs_out[i]; proofs_out[i] = nullptr; }
    return fail(first_rc, "unit %zu: %s", first_unit.load(), msg.c_str());
  }
  return SBN_OK;
}
int sbn_batch_prover_prove_ios(sbn_batch_prover* B, const uint32_t* ios, size_t ios_words_per_unit, size_t num_io, size_t count, sbn_proof** proofs_out) {
  if (!B || !ios || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  for (size_t i = 0; i < count; i++) proofs_out[i] = nullptr;
  if (exp_io_words(B->kind) == 0 || ios_words_per_unit != exp_io_words(B->kind) * num_io)
    return fail(SBN_ERR_BAD_ARG, "ios_words_per_unit must be %zu u32 words per instance times num_io", exp_io_words(B->kind));
  return prove_units(B, count, proofs_out, [&](sbn_prover* P, size_t u) {
    const int rc = sbn_prover_generate_trace(P, ios + u * ios_words_per_unit, num_io, nullptr);
    return rc ? rc : sbn_prover_prove(P, &proofs_out[u]);
  });
}

// Verified proving (include/sbn.h): the mode of every context; each owns its verifier and checks on its own worker thread
int sbn_batch_prover_set_guard(sbn_batch_prover* B, uint32_t mode) {
  if (!B) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (mode > SBN_GUARD_HOST) return fail(SBN_ERR_BAD_ARG, "unknown guard mode %u (0 off, 1 device, 2 host)", mode);
  for (sbn_prover* P : B->provers) if (int rc = sbn_prover_set_guard(P, mode)) return rc;
  return SBN_OK;
}
int sbn_batch_prover_guard_stats(const sbn_batch_prover* B, uint64_t out[4]) {
  if (!B || !out) return fail(SBN_ERR_BAD_ARG, "null argument");
  for (int i = 0; i < 4; i++) out[i] = 0;
  for (const sbn_prover* P : B->provers) {
    uint64_t s[4];
    if (int rc = sbn_prover_guard_stats(P, s)) return rc;
    for (int i = 0; i < 4; i++) out[i] += s[i];
  }
  return SBN_OK;
}

// Units whose traces are already in host memory, one allocation per column (sbn_prover_prove_host_columns per unit): the shape of
// prove_ios above, each context's thread takes the next unit.  Every context uploads on its own copy stream through its own pinned
// ring, so one unit's PCIe time runs beside the others' kernels; the host copies into the rings share the worker pool, which runs
// one parallel loop at a time (tracegen.hip WorkerPool::run), as the witness loops of prove_ios do.
int sbn_batch_prover_prove_host_columns(sbn_batch_prover* B, const uint64_t* const* columns, size_t n_columns, uint32_t flags,
                                        const uint64_t* const* public_inputs, size_t n_pi, size_t count, sbn_proof** proofs_out) {
  if (!B || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  for (size_t i = 0; i < count; i++) proofs_out[i] = nullptr;
  if (count && (!columns || (n_pi && !public_inputs))) return fail(SBN_ERR_BAD_ARG, "null argument");
  return prove_units(B, count, proofs_out, [&](sbn_prover* P, size_t u) {
    return sbn_prover_prove_host_columns(P, columns + u * n_columns, n_columns, flags, n_pi ? public_inputs[u] : nullptr, n_pi, nullptr, &proofs_out[u]);
  });
}

// What the four calls below share: every proof slot of the `units` units is nulled; `derive(ios)` checks what is left to check and
// derives the padded, unit-cut list once on the host pool (into ios_out, or into a buffer of this call); then the units go through
// the explicit-list path above, so the proofs, their public inputs and ios_out are those of sbn_batch_prover_prove_ios on that list
// by construction, in every placement of the table's chains.
static int prove_derived_units(sbn_batch_prover* B, size_t units, uint32_t* ios_out, sbn_proof** proofs_out, const std::function<int(uint32_t*)>& derive) {
  const size_t unit_words = exp_io_words(B->kind) * B->num_io;
  for (size_t u = 0; u < units; u++) proofs_out[u] = nullptr;
  std::vector<uint32_t> own;
  uint32_t* ios = ios_out;
  if (!ios) { own.resize(unit_words * units); ios = own.data(); }
  if (int rc = derive(ios)) return rc;
  return sbn_batch_prover_prove_ios(B, ios, unit_words, B->num_io, units, proofs_out);
}

// A chained list of any length as units of the batch prover's table (include/sbn.h, "Long chained lists"; csrc/msm.hip).
int sbn_batch_prover_prove_msm(sbn_batch_prover* B, const uint32_t* terms, size_t count, const uint32_t* start, sbn_proof** proofs_out,
                               uint32_t* final_out, uint32_t* ios_out) {
  if (!B || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  return prove_derived_units(B, sbn_msm_num_units(count, B->num_io), ios_out, proofs_out, [&](uint32_t* ios) {
    if (exp_io_words(B->kind) == 0) return fail(SBN_ERR_UNSUPPORTED, "chained lists cover the Exp tables");
    if (!terms || !start || count == 0) return fail(SBN_ERR_BAD_ARG, "null argument or no instance");
    return sbn_msm_instances(B->kind, terms, count, B->num_io, start, ios, final_out);
  });
}

// Independent scalar multiplications of any count (include/sbn.h, "Scalar multiplications"; csrc/scalar_mul.hip): the products
// are derived with the list.
int sbn_batch_prover_prove_scalar_muls(sbn_batch_prover* B, const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t count,
                                       const uint32_t* offset, sbn_proof** proofs_out, uint32_t* products_out, uint8_t* infinity_out, uint32_t* ios_out) {
  if (!B || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  return prove_derived_units(B, sbn_msm_num_units(count, B->num_io), ios_out, proofs_out, [&](uint32_t* ios) {
    return sbn_scalar_mul_instances(B->kind, points, scalars, scalar_count, count, B->num_io, offset, ios, products_out, infinity_out);
  });
}

// Field powers and power towers of any count (include/sbn.h, "Field powers"; csrc/powers.hip): the powers are derived with the
// list, so a tower that straddles two units needs no context to wait for another.
int sbn_batch_prover_prove_powers(sbn_batch_prover* B, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count, size_t depth,
                                  sbn_proof** proofs_out, uint32_t* powers_out, uint32_t* ios_out) {
  if (!B || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  const bool fits = count && depth <= (size_t)-1 / 2 / count;   // (what does not fit has no unit count: sbn_power_instances refuses it)
  return prove_derived_units(B, fits ? sbn_msm_num_units(count * depth, B->num_io) : 0, ios_out, proofs_out, [&](uint32_t* ios) {
    return sbn_power_instances(B->kind, bases, exps, exp_count, count, depth, B->num_io, ios, powers_out);
  });
}

// Field programs of any count (include/sbn.h, "Field programs"; csrc/program.hip): every link is resolved with the list, so a link
// across a unit boundary needs no context to wait for another.
int sbn_batch_prover_prove_program(sbn_batch_prover* B, const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values,
                                   const uint32_t* exps, size_t n_exps, sbn_proof** proofs_out, uint32_t* outs_out, uint32_t* ios_out) {
  if (!B || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  const bool fits = count && count < 0x7fffffffu;   // (what does not fit has no unit count: sbn_program_instances refuses it)
  return prove_derived_units(B, fits ? sbn_msm_num_units(count, B->num_io) : 0, ios_out, proofs_out, [&](uint32_t* ios) {
    return sbn_program_instances(B->kind, nodes, count, values, n_values, exps, n_exps, B->num_io, ios, outs_out);
  });
}

// Mapped programs of any count (include/sbn.h, "Mapped links and the final exponentiation"): the list holds the mapped words, so the
// units go through the same loop.
int sbn_batch_prover_prove_program_m(sbn_batch_prover* B, const sbn_program_node_m* nodes, size_t count, const uint32_t* values, size_t n_values,
                                     const uint32_t* exps, size_t n_exps, sbn_proof** proofs_out, uint32_t* outs_out, uint32_t* ios_out) {
  if (!B || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  const bool fits = count && count < 0x7fffffffu;   // (as above: sbn_program_m_instances refuses what does not fit)
  return prove_derived_units(B, fits ? sbn_msm_num_units(count, B->num_io) : 0, ios_out, proofs_out, [&](uint32_t* ios) {
    return sbn_program_m_instances(B->kind, nodes, count, values, n_values, exps, n_exps, B->num_io, ios, outs_out);
  });
}

// Curve programs of any count (include/sbn.h, "Curve programs"; csrc/curve_program.hip): the start, every link, the outputs and the
// values are derived with the list.
int sbn_batch_prover_prove_curve_program(sbn_batch_prover* B, const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points,
                                         const uint32_t* exps, size_t n_exps, sbn_proof** proofs_out, uint32_t* outs_out, uint32_t* values_out,
                                         uint8_t* infinity_out, uint8_t* choice_out, uint32_t* ios_out) {
  if (!B || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  const bool fits = count && count < 0x7fffffffu && exp_io_words(B->kind);   // (what does not fit has no unit count: sbn_curve_program_instances refuses it)
  return prove_derived_units(B, fits ? sbn_msm_num_units(count, B->num_io) : 0, ios_out, proofs_out, [&](uint32_t* ios) {
    return sbn_curve_program_instances(B->kind, nodes, count, points, n_points, exps, n_exps, B->num_io, ios, outs_out, values_out, infinity_out, choice_out);
  });
}

// Batches of short MSMs of any total length (include/sbn.h, "Batches of short MSMs"; csrc/msm_batch.hip): a segment that straddles
// two units needs no context to wait for another.
int sbn_batch_prover_prove_msm_batch(sbn_batch_prover* B, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts, size_t start_count,
                                     sbn_proof** proofs_out, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out, uint32_t* ios_out) {
  if (!B || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  size_t M = 0;   // (a list whose lengths are refused has no unit count: M stays 0 and nothing of proofs_out is touched)
  const int bad = msm_batch_check_args(B->kind, terms, lengths, segments, &starts, &start_count, B->num_io, sums_out, infinity_out, &M);
  const size_t units = sbn_msm_num_units(M, B->num_io);
  return prove_derived_units(B, units, ios_out, proofs_out, [&](uint32_t* ios) {
    return bad ? bad : msm_batch_derive(B->kind, terms, lengths, segments, starts, start_count, M, units * B->num_io, ios, finals_out, sums_out, infinity_out);
  });
}

// Complete sums of any total length (include/sbn.h, "Complete sums"): the effective terms, the choice of every segment's start and
// the list are derived once on the host pool, then the units take the explicit-list path.
int sbn_batch_prover_prove_msm_batch_complete(sbn_batch_prover* B, const uint32_t* terms, const uint8_t* term_infinity, const uint64_t* lengths, size_t segments,
                                              sbn_proof** proofs_out, uint32_t* terms_out, uint32_t* starts_out, uint8_t* choice_out, uint32_t* finals_out,
                                              uint32_t* sums_out, uint8_t* infinity_out, uint32_t* ios_out) {
  if (!B || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  size_t M = 0;   // (as above: a refused list has no unit count)
  const int bad = msm_batch_complete_args(B->kind, terms, lengths, segments, B->num_io, &M);
  const size_t units = sbn_msm_num_units(M, B->num_io);
  return prove_derived_units(B, units, ios_out, proofs_out, [&](uint32_t* ios) {
    if (bad) return bad;
    std::vector<uint32_t> own;
    uint32_t* eff = terms_out;
    if (!eff) { own.resize(exp_io_words(B->kind) * M); eff = own.data(); }   // (an ios row is wider than a term)
    if (int rc = msm_batch_effective_terms(B->kind, terms, term_infinity, lengths, segments, M, eff)) return rc;
    return msm_batch_complete_choose(B->kind, eff, lengths, segments, M, units * B->num_io, ios, starts_out, choice_out, finals_out, sums_out, infinity_out);
  });
}

int sbn_batch_prover_prove_mul_by_cofactor(sbn_batch_prover* B, const uint32_t* points, size_t count, sbn_proof** proofs_out, uint32_t* cleared_out,
                                           uint8_t* infinity_out, uint32_t* ios_out) {
  if (!B || !proofs_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  for (size_t u = 0; u < sbn_msm_num_units(count, B->num_io); u++) proofs_out[u] = nullptr;
  if (B->kind != SBN_AIR_G2_EXP) return fail(SBN_ERR_BAD_ARG, "cofactor clearing is a call of the G2_EXP table (the twist), this batch prover's table is kind %d", B->kind);
  return sbn_batch_prover_prove_scalar_muls(B, points, g2_cofactor_words(), 1, count, nullptr, proofs_out, cleared_out, infinity_out, ios_out);
}

}  // extern "C"
