// Long chained lists (include/sbn.h, "Long chained lists"): an MSM / multi-exponentiation of any length as units of one table.
// The reference's g1_exp_circuit (src/curves/g1/circuit.rs:273-277, 303) resizes a short list with copies of its LAST input and
// uses outputs[..n] only; its *_msm tests connect offset[k+1] to output[k] inside the circuit (circuit.rs:480-483).  Here
//  * sbn_msm_instances derives the whole list once on the host pool (chain_instances.hip) and pads the last unit that way;
//  * sbn_msm_check_links is what the `connect` calls are: it reads the public inputs of the unit proofs and checks that they
//    are one chained list.  It verifies no proof.
// Host code only: no kernel is launched from this unit.
#include "host_common.hpp"
#include <cstring>
#include <vector>

using namespace sbn;

namespace {
// (the public inputs of one instance: PiLayout, host_common.hpp)
bool same(const uint64_t* a, const uint64_t* b, size_t n) { return memcmp(a, b, n * sizeof(uint64_t)) == 0; }
}  // namespace

extern "C" size_t sbn_msm_num_units(size_t count, size_t num_io) {
  if (count == 0 || num_io == 0) return 0;
  return count / num_io + (count % num_io ? 1 : 0);
}

extern "C" int sbn_msm_instances(int32_t kind, const uint32_t* terms, size_t count, size_t num_io, const uint32_t* start, uint32_t* ios_out,
                                 uint32_t* final_out) {
  if (!terms || !start || !ios_out || count == 0 || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no instance or num_io = 0");
  if (int rc = chain_instances_host((int)kind, terms, count, start, ios_out, final_out)) return rc;   // (names the global instance)
  const size_t IOW = exp_io_words((int)kind), total = sbn_msm_num_units(count, num_io) * num_io;
  for (size_t g = count; g < total; g++) memcpy(ios_out + IOW * g, ios_out + IOW * (count - 1), IOW * sizeof(uint32_t));
  return SBN_OK;
}

extern "C" int sbn_msm_check_links(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count,
                                   const uint32_t* terms, const uint32_t* start, uint32_t* final_out) {
  PiLayout L;
  if (!pi_layout((int)kind, L)) return fail(SBN_ERR_BAD_ARG, "kind %d is not an Exp table", (int)kind);
  if (!public_inputs || !start || count == 0 || num_io == 0) return fail(SBN_ERR_BAD_ARG, "null argument, no instance or num_io = 0");
  if (units != sbn_msm_num_units(count, num_io))
    return fail(SBN_ERR_VERIFY_FAILED, "%zu units given, a list of %zu instances in tables of %zu has %zu units", units, count, num_io, sbn_msm_num_units(count, num_io));
  for (size_t u = 0; u < units; u++) if (!public_inputs[u]) return fail(SBN_ERR_BAD_ARG, "null public inputs (unit %zu)", u);
  const size_t per = L.per(), T = L.xw + L.ew;
  auto inst = [&](size_t g) { return public_inputs[g / num_io] + per * (g % num_io); };
  const size_t oX = 0, oOff = L.W, oExp = 2 * L.W, oOut = 2 * L.W + L.EW;
  std::vector<uint64_t> want(L.W);
  value_to_pi(L, start, want.data());
  if (!same(inst(0) + oOff, want.data(), L.W)) return fail(SBN_ERR_VERIFY_FAILED, "instance 0: offset differs from start");
  const uint64_t* last = inst(count - 1);
  for (size_t g = 0; g < units * num_io; g++) {
    const uint64_t* p = inst(g);
    if (g < count) {
      if (terms) {
        value_to_pi(L, terms + T * g, want.data());
        if (!same(p + oX, want.data(), L.W)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: x differs from the caller's term", g);
        uint64_t e[8];
        exp_to_pi(L, terms + T * g + L.xw, e);
        if (!same(p + oExp, e, L.EW)) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: exponent differs from the caller's term", g);
      }
      if (g > 0 && !same(p + oOff, inst(g - 1) + oOut, L.W))
        return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: offset differs from the output of instance %zu", g, g - 1);
    } else {   // a pad instance is instance count - 1 again
      static const char* const field[4] = {"x", "offset", "exponent", "output"};
      const size_t at[4] = {oX, oOff, oExp, oOut}, len[4] = {L.W, L.W, L.EW, L.W};
      for (int f = 0; f < 4; f++)
        if (!same(p + at[f], last + at[f], len[f]))
          return fail(SBN_ERR_VERIFY_FAILED, "instance %zu (pad): %s differs from instance %zu", g, field[f], count - 1);
    }
  }
  // the last output in the word shape of start; a limb wider than its slot is no output of the table
  const uint64_t lim = L.limb16 ? 0xffffULL : 0xffffffffULL;
  for (size_t i = 0; i < L.W; i++)
    if (last[oOut + i] > lim) return fail(SBN_ERR_VERIFY_FAILED, "instance %zu: output limb %zu is out of range", count - 1, i);
  if (final_out) {
    if (!L.limb16) for (size_t i = 0; i < L.W; i++) final_out[i] = (uint32_t)last[oOut + i];
    else for (size_t i = 0; i < L.xw; i++) final_out[i] = (uint32_t)(last[oOut + 2 * i] | (last[oOut + 2 * i + 1] << 16));
  }
  return SBN_OK;
}
