// AddressSanitizer + UBSan driver of the field programs (csrc/program.hip on instance_lists.hpp, with the units it links: msm.hip,
// msm_batch.hip, scalar_mul.hip, chain_instances.hip, tracegen.hip; tests/test_program_sanitize.py builds and runs it): on the three field tables,
// with num_io = 4 and every buffer allocated at its exact size, a program of 11 nodes (3 units, 1 pad) with x-links, offset-links,
// both links to one node, links across unit boundaries, a zero base, a zero exponent and SBN_NODE_ONE; the same call with every
// output pointer null; the schedule; the check on public inputs formed here from the derived list, and its rejections; and the
// refusals, an unused literal >= p among them.  No kernel is launched.
#include "../../include/sbn.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace sbn { thread_local std::string g_last_error; }   // defined in prover.hip in the library proper

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, sbn::g_last_error.c_str()); failures++; } } while (0)

template <typename T> struct Exact {   // a buffer of exactly n elements (a null pointer for none), zeroed
  T* p;
  explicit Exact(size_t n) : p(n ? (T*)calloc(n, sizeof(T)) : nullptr) {}
  ~Exact() { free(p); }
  Exact(const Exact&) = delete;
};

static const size_t NUM_IO = 4, COUNT = 11, UNITS = 3, NV = 4, NE = 4;
static const uint32_t OUT = SBN_NODE_OUTPUT, ONE = SBN_NODE_ONE;
static bool names(const char* a, const char* b = "") { return sbn::g_last_error.find(a) != std::string::npos && sbn::g_last_error.find(b) != std::string::npos; }

// W / ew: u32 words of a value / an exponent in `ios`; the public inputs carry a value as PW limbs (16-bit in the Fq12 tables) and
// the exponent as PE words (one u64 in FQ12_EXP_U64)
static void run(int32_t kind, size_t W, size_t ew) {
  const size_t IOW = 2 * W + ew, PW = W == 8 ? 8 : 192, PE = ew == 2 ? 1 : 8, PER = 3 * PW + PE;
  const bool limb16 = W != 8;
  Exact<sbn_program_node> nodes(COUNT);
  const sbn_program_node nd[COUNT] = {{0, ONE, 2}, {1, 0, 1}, {OUT | 0, ONE, 3}, {1, OUT | 0, 2}, {OUT | 2, OUT | 3, 1}, {OUT | 4, OUT | 4, 3},
                                      {2, OUT | 1, 2}, {OUT | 5, ONE, 0}, {2, OUT | 5, 0}, {OUT | 6, OUT | 8, 1}, {OUT | 9, OUT | 2, 3}};
  memcpy(nodes.p, nd, sizeof nd);
  Exact<uint32_t> values(W * NV), exps(ew * NE);
  for (size_t i = 0; i < W; i++) { values.p[i] = (uint32_t)(0x9e3779b9u * (i + 1)) >> (i % 8 == 7 ? 4 : 0); values.p[W + i] = (uint32_t)(0x85ebca6bu * (i + 3)) >> (i % 8 == 7 ? 4 : 0); }
  memset(values.p + 3 * W, 0xff, W * 4);            // literal 2 is zero; literal 3 is >= p and no node uses it: never read
  exps.p[ew * 1] = 1;                               // exponent 0 is zero, exponent 1 is one
  for (size_t i = 0; i < ew; i++) { exps.p[ew * 2 + i] = 0x7f4a7c15u + (uint32_t)i; exps.p[ew * 3 + i] = 0x12345678u * (uint32_t)(i + 1); }

  // ---- the schedule ---------------------------------------------------------------------------------------------------------------
  Exact<uint32_t> level(COUNT);
  uint32_t depth = 0;
  EXPECT(sbn_program_levels(nodes.p, COUNT, level.p, &depth) == SBN_OK && depth == 7);
  const uint32_t want_level[COUNT] = {0, 0, 1, 1, 2, 3, 1, 4, 4, 5, 6};
  EXPECT(memcmp(level.p, want_level, sizeof want_level) == 0);
  EXPECT(sbn_program_levels(nodes.p, COUNT, nullptr, nullptr) == SBN_OK);

  // ---- the list and the outputs ---------------------------------------------------------------------------------------------------
  Exact<uint32_t> ios(IOW * UNITS * NUM_IO), outs(W * COUNT), outs2(W * COUNT);
  EXPECT(sbn_program_instances(kind, nodes.p, COUNT, values.p, NV, exps.p, NE, NUM_IO, ios.p, outs.p) == SBN_OK);
  EXPECT(memcmp(ios.p + IOW * 2, outs.p, W * 4) == 0);                                       // x of node 2 = the output of node 0
  EXPECT(memcmp(ios.p + IOW * 4 + W, outs.p + W * 3, W * 4) == 0);                           // offset of node 4, across the unit boundary
  EXPECT(memcmp(ios.p + IOW * 11, ios.p + IOW * 10, IOW * 4) == 0);                          // the pad copies row count - 1
  EXPECT(outs.p[W * 7] == 1 && memcmp(outs.p + W * 8, outs.p + W * 5, W * 4) == 0);          // x^0 = 1 and 0^0 = 1
  for (size_t i = 0; i < W; i++) EXPECT(outs.p[W * 6 + i] == 0);                             // a zero base
  EXPECT(sbn_program_instances(kind, nodes.p, COUNT, values.p, NV, exps.p, NE, NUM_IO, nullptr, nullptr) == SBN_OK);
  EXPECT(sbn_program_instances(kind, nodes.p, COUNT, values.p, NV, exps.p, NE, NUM_IO, nullptr, outs2.p) == SBN_OK && memcmp(outs.p, outs2.p, W * COUNT * 4) == 0);

  // ---- the check, on public inputs formed from the derived list ----------------------------------------------------------------------
  Exact<uint64_t> pi(PER * UNITS * NUM_IO);
  auto put = [&](uint64_t* p, const uint32_t* w) { for (size_t i = 0; i < PW; i++) p[i] = limb16 ? (w[i >> 1] >> (16 * (i & 1))) & 0xffff : w[i]; };
  for (size_t g = 0; g < UNITS * NUM_IO; g++) {
    uint64_t* p = pi.p + PER * g;
    const uint32_t* io = ios.p + IOW * g;
    put(p, io); put(p + PW, io + W);
    if (PE == 1) p[2 * PW] = (uint64_t)io[2 * W] | ((uint64_t)io[2 * W + 1] << 32);
    else for (size_t i = 0; i < 8; i++) p[2 * PW + i] = io[2 * W + i];
    put(p + 2 * PW + PE, outs.p + W * (g < COUNT ? g : COUNT - 1));
  }
  Exact<const uint64_t*> units(UNITS);
  for (size_t u = 0; u < UNITS; u++) units.p[u] = pi.p + PER * NUM_IO * u;
  auto check = [&](uint32_t* o) { return sbn_program_check(kind, NUM_IO, units.p, UNITS, nodes.p, COUNT, values.p, NV, exps.p, NE, o); };
  EXPECT(check(outs2.p) == SBN_OK && memcmp(outs.p, outs2.p, W * COUNT * 4) == 0);
  EXPECT(check(nullptr) == SBN_OK);
  auto edited = [&](size_t g, size_t at, const char* a, const char* b) {
    pi.p[PER * g + at] ^= 1;
    EXPECT(check(nullptr) == SBN_ERR_VERIFY_FAILED && names(a, b));
    pi.p[PER * g + at] ^= 1;
  };
  edited(0, 0, "instance 0:", "x differs from the caller's literal 0");
  edited(1, PW, "instance 1:", "offset differs from the caller's literal 0");
  edited(7, PW, "instance 7:", "offset is not one");
  edited(10, 2 * PW, "instance 10:", "exponent");
  edited(4, 3, "instance 4:", "x differs from the output of node 2");
  edited(10, PW + PW - 1, "instance 10:", "offset differs from the output of node 2");
  edited(11, 2 * PW + PE + PW - 1, "instance 11 (pad)", "output");
  pi.p[PER * 10 + 2 * PW + PE + 1] |= (uint64_t)1 << (limb16 ? 16 : 32);
  EXPECT(check(nullptr) == SBN_ERR_VERIFY_FAILED && names("instance 10:", "output limb 1 "));
  pi.p[PER * 10 + 2 * PW + PE + 1] &= limb16 ? 0xffff : 0xffffffffu;
  for (size_t i = 0; i < (limb16 ? 16u : 8u); i++) pi.p[PER * 10 + 2 * PW + PE + i] = limb16 ? 0xffff : 0xffffffffu;
  EXPECT(check(nullptr) == SBN_ERR_VERIFY_FAILED && names("instance 10:", "coefficient >= p"));
  put(pi.p + PER * 10 + 2 * PW + PE, outs.p + W * 10);
  EXPECT(check(nullptr) == SBN_OK);
  EXPECT(sbn_program_check(kind, NUM_IO, units.p, UNITS - 1, nodes.p, COUNT, values.p, NV, exps.p, NE, nullptr) == SBN_ERR_VERIFY_FAILED && names("2 units given"));
  { const uint64_t* t = units.p[0]; units.p[0] = units.p[1]; units.p[1] = t; }                // two units swapped
  EXPECT(check(nullptr) == SBN_ERR_VERIFY_FAILED && names("instance 0:"));
  { const uint64_t* t = units.p[0]; units.p[0] = units.p[1]; units.p[1] = t; }
  units.p[2] = nullptr;
  EXPECT(check(nullptr) == SBN_ERR_BAD_ARG && names("unit 2"));

  // ---- the refusals, in the header's order -------------------------------------------------------------------------------------------
  auto inst = [&](const sbn_program_node* n, size_t count, size_t nv, size_t ne, size_t num_io) { return sbn_program_instances(kind, n, count, values.p, nv, exps.p, ne, num_io, nullptr, nullptr); };
  EXPECT(sbn_program_instances(SBN_AIR_G1_EXP, nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr, nullptr) == SBN_ERR_UNSUPPORTED);
  EXPECT(inst(nullptr, COUNT, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && inst(nodes.p, 0, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && inst(nodes.p, COUNT, NV, NE, 0) == SBN_ERR_BAD_ARG);
  EXPECT(sbn_program_instances(kind, nodes.p, COUNT, nullptr, NV, exps.p, NE, NUM_IO, nullptr, nullptr) == SBN_ERR_BAD_ARG);
  EXPECT(sbn_program_instances(kind, nodes.p, COUNT, values.p, NV, nullptr, NE, NUM_IO, nullptr, nullptr) == SBN_ERR_BAD_ARG);
  EXPECT(inst(nodes.p, 0x7fffffffu, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && inst(nodes.p, COUNT, 0x7fffffffu, NE, NUM_IO) == SBN_ERR_BAD_ARG);
  Exact<sbn_program_node> one(1);
  one.p[0] = {OUT | 0, 9, 9};
  EXPECT(inst(one.p, 1, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: x links to node 0"));
  one.p[0] = {ONE, 4, 9};
  EXPECT(inst(one.p, 1, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: offset is literal 4 of 4"));
  one.p[0] = {ONE, 0, 9};
  EXPECT(inst(one.p, 1, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: x is SBN_NODE_ONE"));
  one.p[0] = {3, 0, 4};
  EXPECT(inst(one.p, 1, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: exponent is index 4 of 4"));
  one.p[0] = {0, 3, 0};
  EXPECT(inst(one.p, 1, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names(">= p (literal 3)"));
  EXPECT(inst(one.p, 1, 3, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: offset is literal 3 of 3"));   // ... and is not read past n_values
  if (ew == 2) {
    Exact<uint32_t> e64(2);
    e64.p[0] = 1; e64.p[1] = 0xffffffffu;           // 2^64 - 2^32 + 1
    one.p[0] = {0, ONE, 0};
    EXPECT(sbn_program_instances(kind, one.p, 1, values.p, NV, e64.p, 1, NUM_IO, nullptr, nullptr) == SBN_ERR_NON_CANONICAL && names("exponent 0"));
  }
  EXPECT(sbn_program_levels(nullptr, 1, nullptr, nullptr) == SBN_ERR_BAD_ARG && sbn_program_levels(one.p, 0, nullptr, nullptr) == SBN_ERR_BAD_ARG);
}

int main() {
  run(SBN_AIR_FQ_EXP, 8, 8);
  run(SBN_AIR_FQ12_EXP, 96, 8);
  run(SBN_AIR_FQ12_EXP_U64, 96, 2);
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("field programs: the schedule, links, pads, optional outputs, the check's rejections and the refusals ok\n");
  return 0;
}
