// AddressSanitizer + UBSan driver of the curve programs (csrc/curve_program.hip on instance_lists.hpp, with the units it links:
// program.hip, msm.hip, msm_batch.hip, scalar_mul.hip, chain_instances.hip, tracegen.hip; tests/test_curve_program_sanitize.py builds
// and runs it): on both curve tables, with num_io = 4 and every buffer allocated at its exact size, a program of 10 nodes (3 units,
// 2 pads) with literals, SBN_NODE_START offsets, x-links and offset-links within a unit and across both unit boundaries, a
// literal-only node, and a literal crafted from the library's own output so that candidate 0 fails and the choice is 1; the same
// call with every output pointer null; the check on public inputs formed here from the derived list, and its rejections; a program
// no candidate can mend; and the refusals, an unused literal off the curve among them.  No kernel is launched.
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

static const size_t NUM_IO = 4, COUNT = 10, UNITS = 3, NP = 4, NE = 4;
static const uint32_t OUT = SBN_NODE_OUTPUT, START = SBN_NODE_START, ONE = SBN_NODE_ONE;
static bool names(const char* a, const char* b = "") { return sbn::g_last_error.find(a) != std::string::npos && sbn::g_last_error.find(b) != std::string::npos; }

static void run(int32_t kind, size_t W) {
  const size_t IOW = 2 * W + 8, PER = IOW + W;
  // literal 0 the generator, literal 1 start candidate 5 (a point with no relation to it), literal 2 = H_0 + e0 G, taken from the
  // library's own output of the one-node program (G, START, e0): behind node 0 it makes candidate 0 meet B = A; literal 3 is off the
  // curve and no node uses it: never read
  Exact<uint32_t> points(W * NP), exps(8 * NE);
  EXPECT(sbn_curve_generator(kind, points.p) == SBN_OK && sbn_start_candidate(kind, 5, points.p + W) == SBN_OK);
  for (size_t i = 0; i < 8; i++) exps.p[i] = 0x7f4a7c15u + (uint32_t)i;      // e0
  exps.p[8] = 1;                                                             // exponent 1 is one
  for (size_t i = 0; i < 7; i++) exps.p[16 + i] = 0x12345678u * (uint32_t)(i + 1);
  exps.p[24] = 5;
  uint8_t choice = 9;
  {
    Exact<sbn_program_node> first(1);
    first.p[0] = {0, START, 0};
    EXPECT(sbn_curve_program_instances(kind, first.p, 1, points.p, 1, exps.p, 1, NUM_IO, nullptr, points.p + 2 * W, nullptr, nullptr, &choice) == SBN_OK && choice == 0);
  }
  memcpy(points.p + 3 * W, points.p, W * 4);
  points.p[3 * W] ^= 1;
  Exact<sbn_program_node> nodes(COUNT);
  const sbn_program_node nd[COUNT] = {{0, START, 0}, {2, OUT | 0, 1}, {1, OUT | 0, 2}, {OUT | 1, START, 3}, {1, OUT | 2, 3}, {OUT | 3, OUT | 1, 2},
                                      {0, 1, 3}, {OUT | 6, OUT | 4, 3}, {1, START, 2}, {OUT | 7, OUT | 5, 3}};
  memcpy(nodes.p, nd, sizeof nd);

  // ---- the list, the outputs and the values ----------------------------------------------------------------------------------------
  Exact<uint32_t> ios(IOW * UNITS * NUM_IO), outs(W * COUNT), values(W * COUNT), outs2(W * COUNT), values2(W * COUNT), cand(W);
  Exact<uint8_t> inf(COUNT), inf2(COUNT);
  EXPECT(sbn_curve_program_instances(kind, nodes.p, COUNT, points.p, NP, exps.p, NE, NUM_IO, ios.p, outs.p, values.p, inf.p, &choice) == SBN_OK);
  EXPECT(choice == 1 && sbn_start_candidate(kind, 1, cand.p) == SBN_OK);
  EXPECT(memcmp(ios.p + W, cand.p, W * 4) == 0 && memcmp(ios.p + IOW * 8 + W, cand.p, W * 4) == 0);   // the START offsets
  EXPECT(memcmp(ios.p + IOW * 1 + W, outs.p, W * 4) == 0);                                   // offset of node 1 = the output of node 0
  EXPECT(memcmp(ios.p + IOW * 5, outs.p + W * 3, W * 4) == 0);                               // x of node 5, across the first unit boundary
  EXPECT(memcmp(ios.p + IOW * 9 + W, outs.p + W * 5, W * 4) == 0);                           // offset of node 9, across the second one
  EXPECT(memcmp(ios.p + IOW * 10, ios.p + IOW * 9, IOW * 4) == 0 && memcmp(ios.p + IOW * 11, ios.p + IOW * 9, IOW * 4) == 0);   // the pads copy row count - 1
  EXPECT(memcmp(values.p + W * 6, outs.p + W * 6, W * 4) == 0);                              // a literal-only node: T = O, value = out
  for (size_t g = 0; g < COUNT; g++) EXPECT(inf.p[g] == 0);
  EXPECT(sbn_curve_program_instances(kind, nodes.p, COUNT, points.p, NP, exps.p, NE, NUM_IO, nullptr, nullptr, nullptr, nullptr, nullptr) == SBN_OK);
  EXPECT(sbn_curve_program_instances(kind, nodes.p, COUNT, points.p, NP, exps.p, NE, NUM_IO, nullptr, outs2.p, nullptr, inf2.p, nullptr) == SBN_OK &&
         memcmp(outs.p, outs2.p, W * COUNT * 4) == 0);

  // ---- the check, on public inputs formed from the derived list ----------------------------------------------------------------------
  Exact<uint64_t> pi(PER * UNITS * NUM_IO);
  for (size_t g = 0; g < UNITS * NUM_IO; g++) {
    uint64_t* p = pi.p + PER * g;
    for (size_t i = 0; i < IOW; i++) p[i] = ios.p[IOW * g + i];
    for (size_t i = 0; i < W; i++) p[IOW + i] = outs.p[W * (g < COUNT ? g : COUNT - 1) + i];
  }
  Exact<const uint64_t*> units(UNITS);
  for (size_t u = 0; u < UNITS; u++) units.p[u] = pi.p + PER * NUM_IO * u;
  auto check = [&](uint32_t c, uint32_t* o, uint32_t* v, uint8_t* f) {
    return sbn_curve_program_check(kind, NUM_IO, units.p, UNITS, nodes.p, COUNT, points.p, NP, exps.p, NE, c, o, v, f);
  };
  EXPECT(check(1, outs2.p, values2.p, inf2.p) == SBN_OK && memcmp(outs.p, outs2.p, W * COUNT * 4) == 0 && memcmp(values.p, values2.p, W * COUNT * 4) == 0 &&
         memcmp(inf.p, inf2.p, COUNT) == 0);
  EXPECT(check(1, nullptr, nullptr, nullptr) == SBN_OK);
  EXPECT(check(0, nullptr, nullptr, nullptr) == SBN_ERR_VERIFY_FAILED && names("instance 0:", "offset differs from start candidate 0"));
  EXPECT(check(8, nullptr, nullptr, nullptr) == SBN_ERR_BAD_ARG);
  auto edited = [&](size_t g, size_t at, const char* a, const char* b) {
    pi.p[PER * g + at] ^= 1;
    EXPECT(check(1, nullptr, nullptr, nullptr) == SBN_ERR_VERIFY_FAILED && names(a, b));
    pi.p[PER * g + at] ^= 1;
  };
  edited(0, 0, "instance 0:", "x differs from the caller's literal 0");
  edited(6, W, "instance 6:", "offset differs from the caller's literal 1");
  edited(8, 2 * W - 1, "instance 8:", "offset differs from start candidate 1");
  edited(4, 2 * W, "instance 4:", "exponent");
  edited(3, 3, "instance 3:", "x differs from the output of node 1");
  edited(5, W - 1, "instance 5:", "x differs from the output of node 3");
  edited(9, W, "instance 9:", "offset differs from the output of node 5");
  edited(11, IOW + W - 1, "instance 11 (pad)", "output");
  edited(9, IOW, "instance 9:", "output is not a point of the curve");
  pi.p[PER * 9 + IOW + 1] |= (uint64_t)1 << 32;
  EXPECT(check(1, nullptr, nullptr, nullptr) == SBN_ERR_VERIFY_FAILED && names("instance 9:", "output limb 1 "));
  pi.p[PER * 9 + IOW + 1] &= 0xffffffffu;
  for (size_t i = 0; i < 8; i++) pi.p[PER * 9 + IOW + i] = 0xffffffffu;
  EXPECT(check(1, nullptr, nullptr, nullptr) == SBN_ERR_VERIFY_FAILED && names("instance 9:", "coordinate >= p"));
  for (size_t i = 0; i < 8; i++) pi.p[PER * 9 + IOW + i] = outs.p[W * 9 + i];
  EXPECT(check(1, nullptr, nullptr, nullptr) == SBN_OK);
  EXPECT(sbn_curve_program_check(kind, NUM_IO, units.p, UNITS - 1, nodes.p, COUNT, points.p, NP, exps.p, NE, 1, nullptr, nullptr, nullptr) == SBN_ERR_VERIFY_FAILED && names("2 units given"));
  { const uint64_t* t = units.p[0]; units.p[0] = units.p[1]; units.p[1] = t; }                // two units swapped
  EXPECT(check(1, nullptr, nullptr, nullptr) == SBN_ERR_VERIFY_FAILED && names("instance 0:"));
  { const uint64_t* t = units.p[0]; units.p[0] = units.p[1]; units.p[1] = t; }
  units.p[2] = nullptr;
  EXPECT(check(1, nullptr, nullptr, nullptr) == SBN_ERR_BAD_ARG && names("unit 2"));

  // ---- a program no candidate can mend, and the refusals in the header's order --------------------------------------------------------
  auto inst = [&](const sbn_program_node* n, size_t count, size_t np, size_t ne, size_t num_io) {
    return sbn_curve_program_instances(kind, n, count, points.p, np, exps.p, ne, num_io, nullptr, nullptr, nullptr, nullptr, nullptr);
  };
  Exact<sbn_program_node> two(2);
  two.p[0] = {0, START, 0}; two.p[1] = {1, 1, 1};                            // x + x with exponent one: B = A whatever the start
  EXPECT(inst(two.p, 2, NP, NE, NUM_IO) == SBN_ERR_WITNESS && names("candidate 7 fails at node 1)", "no candidate can mend"));
  EXPECT(sbn_curve_program_instances(SBN_AIR_FQ_EXP, nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SBN_ERR_UNSUPPORTED);
  EXPECT(inst(nullptr, COUNT, NP, NE, NUM_IO) == SBN_ERR_BAD_ARG && inst(nodes.p, 0, NP, NE, NUM_IO) == SBN_ERR_BAD_ARG && inst(nodes.p, COUNT, NP, NE, 0) == SBN_ERR_BAD_ARG);
  EXPECT(sbn_curve_program_instances(kind, nodes.p, COUNT, nullptr, NP, exps.p, NE, NUM_IO, nullptr, nullptr, nullptr, nullptr, nullptr) == SBN_ERR_BAD_ARG);
  EXPECT(sbn_curve_program_instances(kind, nodes.p, COUNT, points.p, NP, nullptr, NE, NUM_IO, nullptr, nullptr, nullptr, nullptr, nullptr) == SBN_ERR_BAD_ARG);
  EXPECT(inst(nodes.p, 0x7fffffffu, NP, NE, NUM_IO) == SBN_ERR_BAD_ARG && inst(nodes.p, COUNT, 0x7fffffffu, NE, NUM_IO) == SBN_ERR_BAD_ARG);
  Exact<sbn_program_node> one(1);
  one.p[0] = {OUT | 0, 9, 9};
  EXPECT(inst(one.p, 1, NP, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: x links to node 0"));
  one.p[0] = {ONE, 4, 9};
  EXPECT(inst(one.p, 1, NP, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: offset is literal 4 of 4"));
  one.p[0] = {0, ONE, 9};
  EXPECT(inst(one.p, 1, NP, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: offset is SBN_NODE_ONE"));
  one.p[0] = {START, 0, 9};
  EXPECT(inst(one.p, 1, NP, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: x is SBN_NODE_START"));
  one.p[0] = {3, 0, 4};
  EXPECT(inst(one.p, 1, NP, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: exponent is index 4 of 4"));
  one.p[0] = {0, 3, 0};
  EXPECT(inst(one.p, 1, NP, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("literal 3 is not a point of the curve"));
  EXPECT(inst(one.p, 1, 3, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 0: offset is literal 3 of 3"));   // ... and is not read past n_points
  memset(points.p + 3 * W, 0xff, 32);
  EXPECT(inst(one.p, 1, NP, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("coordinate >= p (literal 3)"));
}

int main() {
  run(SBN_AIR_G1_EXP, 16);
  run(SBN_AIR_G2_EXP, 32);
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("curve programs: links, starts, pads, values, optional outputs, the check's rejections and the refusals ok\n");
  return 0;
}
