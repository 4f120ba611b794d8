// Chained instance lists on the host (sbn_chain_instances): the call shape of the reference's *_msm tests
// (src/curves/g1/circuit.rs:459-509 and its G2 / Fq12 / Fq12U64 twins), where offset[0] is a fixed start value and offset[k+1] is
// the output of instance k, so that the last output is start + sum e_k x_k on the curves and start * prod x_k^e_k in the fields.
// The reference derives every offset with arkworks per instance (G1ExpOutputGenerator::run_once, circuit.rs:111-123); here a
// chained list is a segmented list of ONE segment and is derived as such (msm_batch.hip says how).  This unit holds what the chained
// calls say differently: the refusals of the values, which name no segment, and the wording of what the derivation cannot derive.
// tracegen_device.hip runs the same derivation on the device and falls back to this one where the chains are host work anyway.
#include "instance_lists.hpp"

using namespace sbn;
using namespace sbn::curve_host;

namespace {
// the field tables, instance by instance: a value / coefficient >= p, then (Fq12ExpU64Stark) an exponent that is no field element
int check_field_terms(const PiLayout& t, const uint32_t* terms, size_t K, const uint32_t* start) {
  const char* what = t.xw == 8 ? "value" : "coefficient";
  if (!below_p(start, t.values())) return fail(SBN_ERR_BAD_ARG, "%s >= p (start)", what);
  for (size_t k = 0; k < K; k++) {
    if (!below_p(terms + t.T() * k, t.values())) return fail(SBN_ERR_BAD_ARG, "%s >= p (instance %zu)", what, k);
    if (t.ew == 2 && ((u64)terms[t.T() * k + 96] | ((u64)terms[t.T() * k + 97] << 32)) >= GLP)
      return fail(SBN_ERR_NON_CANONICAL, "exponent of instance %zu is not a canonical field element", k);
  }
  return SBN_OK;
}
}  // namespace

namespace sbn {
int chain_terms_check_curve(int E, const uint32_t* terms, size_t K, const uint32_t* start) {
  const size_t T = curve_layout(E).T();
  return E == 1 ? check_curve_points<1>(terms, T, K, start, "start") : check_curve_points<2>(terms, T, K, start, "start");
}
int chain_instances_host(int kind, const uint32_t* terms, size_t K, const uint32_t* start, uint32_t* ios, uint32_t* final_out) {
  PiLayout t;
  if (!pi_layout(kind, t)) return fail(SBN_ERR_BAD_ARG, "kind %d is not an Exp table", kind);
  if (int rc = t.E ? chain_terms_check_curve(t.E, terms, K, start) : check_field_terms(t, terms, K, start)) return rc;
  const uint64_t length = K;
  ListRefusal why;
  if (segmented_derive(kind, terms, &length, 1, start, 1, K, K, ios, final_out, nullptr, nullptr, &why)) return SBN_OK;
  switch (why.what) {
    case ListRefusal::OFFSET_AT_INFINITY: return fail(SBN_ERR_WITNESS, "the offset of instance %zu is the point at infinity", why.at);
    case ListRefusal::OUTPUT_AT_INFINITY: return fail(SBN_ERR_WITNESS, "the output of instance %zu is the point at infinity", why.at);
    default: return fail(SBN_ERR_WITNESS, UNNAMED_WALK_TEXT);   // (a chained list names no instance of a degenerate walk)
  }
}
}  // namespace sbn

extern "C" int sbn_chain_instances(int32_t kind, const uint32_t* terms, size_t count, const uint32_t* start, uint32_t* ios_out, uint32_t* final_out) {
  if (!terms || !start || !ios_out || count == 0) return fail(SBN_ERR_BAD_ARG, "null argument or no instance");
  return chain_instances_host((int)kind, terms, count, start, ios_out, final_out);
}
