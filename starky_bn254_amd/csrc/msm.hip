// Long chained lists (include/sbn.h, "Long chained lists"): an MSM / multi-exponentiation of any length as units of one table.
// The reference's g1_exp_circuit (src/curves/g1/circuit.rs:273-277, 303) resizes a short list with copies of its LAST input and
// uses outputs[..n] only; its *_msm tests connect offset[k+1] to output[k] inside the circuit (circuit.rs:480-483).  Here
//  * sbn_msm_instances derives the whole list once on the host pool (chain_instances.hip) and pads the last unit that way;
//  * sbn_msm_check_links is what the `connect` calls are: it reads the public inputs of the unit proofs and checks that they
//    are one chained list.  It verifies no proof.
// Host code only: no kernel is launched from this unit.
#include "instance_lists.hpp"

using namespace sbn;
using namespace sbn::curve_host;

extern "C" size_t sbn_msm_num_units(size_t count, size_t num_io) {
  if (count == 0 || num_io == 0) return 0;
  return count / num_io + (count % num_io ? 1 : 0);
}

extern "C" int sbn_msm_instances(int32_t kind, const uint32_t* terms, size_t count, size_t num_io, const uint32_t* start, uint32_t* ios_out,
                                 uint32_t* final_out) {
  if (!terms || !start || !ios_out || count == 0 || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no instance or num_io = 0");
  if (int rc = chain_instances_host((int)kind, terms, count, start, ios_out, final_out)) return rc;   // (names the global instance)
  pad_rows(ios_out, exp_io_words((int)kind), count, sbn_msm_num_units(count, num_io) * num_io);
  return SBN_OK;
}

extern "C" int sbn_msm_check_links(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count,
                                   const uint32_t* terms, const uint32_t* start, uint32_t* final_out) {
  PiLayout L;
  if (!pi_layout((int)kind, L)) return fail(SBN_ERR_BAD_ARG, "kind %d is not an Exp table", (int)kind);
  if (!public_inputs || !start || count == 0 || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no instance or num_io = 0");
  if (units != sbn_msm_num_units(count, num_io))
    return fail(SBN_ERR_VERIFY_FAILED, "%zu units given, a list of %zu instances in tables of %zu has %zu units", units, count, num_io, sbn_msm_num_units(count, num_io));
  const UnitInputs U((int)kind, num_io, public_inputs, units);
  if (int rc = U.null_unit()) return rc;
  if (!U.value_is(0, U.oOff, start)) return fail(SBN_ERR_VERIFY_FAILED, "instance 0: offset differs from start");
  for (size_t g = 0; g < U.rows(); g++) {
    if (g >= count) { if (int rc = U.pad(g, count - 1)) return rc; continue; }
    if (terms) {
      if (!U.value_is(g, U.oX, terms + L.T() * g)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: x differs from the caller's term", g);
      if (!U.exp_is(g, terms + L.T() * g + L.xw)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: exponent differs from the caller's term", g);
    }
    if (g > 0 && !same(U.inst(g) + U.oOff, U.inst(g - 1) + U.oOut, L.W))
      return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: offset differs from the output of instance %zu", g, g - 1);
  }
  // the last output in the word shape of start
  std::vector<uint32_t> last(L.xw);
  size_t limb;
  if (!U.output(count - 1, last.data(), &limb)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output limb %zu is out of range", count - 1, limb);
  if (final_out) memcpy(final_out, last.data(), L.xw * sizeof(uint32_t));
  return SBN_OK;
}
