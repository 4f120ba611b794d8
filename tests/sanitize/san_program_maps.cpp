// AddressSanitizer + UBSan driver of the mapped links of the field programs (csrc/program.hip on instance_lists.hpp, with the units
// it links: msm.hip, msm_batch.hip, scalar_mul.hip, chain_instances.hip, tracegen.hip; tests/test_program_maps_sanitize.py builds
// and runs it): on the two Fq12 tables, with num_io = 4 and every buffer allocated at its exact size, a mapped program of 11 nodes
// (3 units, 1 pad: the last node is mapped) with every map 1 .. 11, both operands of a node linked to one node under different
// maps and mapped links across unit boundaries; the same call with every output pointer null; the schedule; the check on public
// inputs formed here from the derived list, and its rejections; the added refusals, FQ_EXP's among them; and the two host helpers
// sbn_fq12_frobenius and sbn_fq12_inverse.  No kernel is launched.
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

static const size_t NUM_IO = 4, COUNT = 11, UNITS = 3, NV = 3, NE = 3, W = 96;
static const uint32_t OUT = SBN_NODE_OUTPUT, ONE = SBN_NODE_ONE;
static bool names(const char* a, const char* b = "") { return sbn::g_last_error.find(a) != std::string::npos && sbn::g_last_error.find(b) != std::string::npos; }
static uint32_t M(uint32_t mx, uint32_t mo) { return mx | (mo << 8); }

static void fill_values(uint32_t* v, size_t n) {   // coefficients below p: the top word of each is shifted down
  for (size_t i = 0; i < W * n; i++) v[i] = (uint32_t)(0x9e3779b9u * (i + 1)) >> (i % 8 == 7 ? 4 : 0);
}

static void helpers() {
  Exact<uint32_t> f(W), a(W), b(W), c(W);
  fill_values(f.p, 1);
  EXPECT(sbn_fq12_frobenius(f.p, 0, a.p) == SBN_OK && memcmp(a.p, f.p, W * 4) == 0);
  for (uint32_t m = 0; m < 12; m++) {   // frob_m then frob_(12 - m) is the identity; frob_1 applied m times is frob_m
    EXPECT(sbn_fq12_frobenius(f.p, m, a.p) == SBN_OK && sbn_fq12_frobenius(a.p, (12 - m) % 12, b.p) == SBN_OK && memcmp(b.p, f.p, W * 4) == 0);
    memcpy(c.p, f.p, W * 4);
    for (uint32_t i = 0; i < m; i++) EXPECT(sbn_fq12_frobenius(c.p, 1, c.p) == SBN_OK);   // in place
    EXPECT(memcmp(c.p, a.p, W * 4) == 0);
  }
  EXPECT(sbn_fq12_frobenius(f.p, 12, a.p) == SBN_ERR_BAD_ARG && sbn_fq12_frobenius(nullptr, 1, a.p) == SBN_ERR_BAD_ARG && sbn_fq12_frobenius(f.p, 1, nullptr) == SBN_ERR_BAD_ARG);
  // the inverse: f * f^-1 = 1 as one instance of FQ12_EXP_U64, offset * x^1
  EXPECT(sbn_fq12_inverse(f.p, a.p) == SBN_OK);
  Exact<uint32_t> vals(2 * W), e(2), outs(W);
  memcpy(vals.p, f.p, W * 4); memcpy(vals.p + W, a.p, W * 4);
  e.p[0] = 1;
  Exact<sbn_program_node_m> n(1);
  n.p[0] = {0, 1, 0, 0};
  EXPECT(sbn_program_m_instances(SBN_AIR_FQ12_EXP_U64, n.p, 1, vals.p, 2, e.p, 1, NUM_IO, nullptr, outs.p) == SBN_OK);
  EXPECT(outs.p[0] == 1);
  for (size_t i = 1; i < W; i++) EXPECT(outs.p[i] == 0);
  memset(b.p, 0, W * 4);
  EXPECT(sbn_fq12_inverse(b.p, a.p) == SBN_ERR_BAD_ARG && names("zero"));
  memset(b.p + W - 8, 0xff, 32);
  EXPECT(sbn_fq12_inverse(b.p, a.p) == SBN_ERR_BAD_ARG && names(">= p") && sbn_fq12_frobenius(b.p, 1, a.p) == SBN_ERR_BAD_ARG);
  EXPECT(sbn_fq12_inverse(nullptr, a.p) == SBN_ERR_BAD_ARG && sbn_fq12_inverse(f.p, nullptr) == SBN_ERR_BAD_ARG);
}

// ew: u32 words of an exponent in `ios`; the public inputs carry a value as 192 16-bit limbs and the exponent as PE words
static void run(int32_t kind, size_t ew) {
  const size_t IOW = 2 * W + ew, PW = 192, PE = ew == 2 ? 1 : 8, PER = 3 * PW + PE;
  Exact<sbn_program_node_m> nodes(COUNT);
  const sbn_program_node_m nd[COUNT] = {{0, ONE, 1, 0}, {1, 0, 0, 0}, {OUT | 0, ONE, 1, M(1, 0)}, {OUT | 0, OUT | 0, 2, M(2, 3)}, {OUT | 1, OUT | 1, 0, M(3, 4)},
                                        {OUT | 2, OUT | 3, 1, 0}, {OUT | 4, OUT | 5, 0, M(5, 6)}, {OUT | 4, OUT | 6, 1, M(0, 7)}, {OUT | 7, OUT | 2, 0, M(8, 9)},
                                        {OUT | 8, OUT | 7, 1, M(10, 11)}, {OUT | 9, OUT | 8, 1, M(11, 10)}};
  memcpy(nodes.p, nd, sizeof nd);
  Exact<uint32_t> values(W * NV), exps(ew * NE);
  fill_values(values.p, 2);
  memset(values.p + 2 * W, 0xff, W * 4);            // literal 2 is >= p and no node uses it: never read
  exps.p[0] = 1; exps.p[ew] = 3;
  for (size_t i = 0; i < ew; i++) exps.p[ew * 2 + i] = 0x7f4a7c15u + (uint32_t)i;

  // ---- the schedule: a map adds no level ----------------------------------------------------------------------------------------------
  Exact<uint32_t> level(COUNT);
  uint32_t depth = 0;
  EXPECT(sbn_program_m_levels(nodes.p, COUNT, level.p, &depth) == SBN_OK && depth == 8);
  const uint32_t want_level[COUNT] = {0, 0, 1, 1, 1, 2, 3, 4, 5, 6, 7};
  EXPECT(memcmp(level.p, want_level, sizeof want_level) == 0);
  EXPECT(sbn_program_m_levels(nodes.p, COUNT, nullptr, nullptr) == SBN_OK);

  // ---- the list and the outputs ---------------------------------------------------------------------------------------------------------
  Exact<uint32_t> ios(IOW * UNITS * NUM_IO), outs(W * COUNT), outs2(W * COUNT), mapped(W);
  EXPECT(sbn_program_m_instances(kind, nodes.p, COUNT, values.p, NV, exps.p, NE, NUM_IO, ios.p, outs.p) == SBN_OK);
  EXPECT(sbn_fq12_frobenius(outs.p, 1, mapped.p) == SBN_OK && memcmp(ios.p + IOW * 2, mapped.p, W * 4) == 0);             // x of node 2 = frob_1(node 0)
  EXPECT(sbn_fq12_frobenius(outs.p + W, 4, mapped.p) == SBN_OK && memcmp(ios.p + IOW * 4 + W, mapped.p, W * 4) == 0);    // offset of node 4, across the unit boundary
  EXPECT(memcmp(ios.p + IOW * 7, outs.p + W * 4, W * 4) == 0);                                                           // an unmapped x beside a mapped offset
  EXPECT(sbn_fq12_frobenius(outs.p + W * 9, 11, mapped.p) == SBN_OK && memcmp(ios.p + IOW * 10, mapped.p, W * 4) == 0);  // the mapped last node ...
  EXPECT(memcmp(ios.p + IOW * 11, ios.p + IOW * 10, IOW * 4) == 0);                                                      // ... and the pad copies its mapped words
  EXPECT(sbn_program_m_instances(kind, nodes.p, COUNT, values.p, NV, exps.p, NE, NUM_IO, nullptr, nullptr) == SBN_OK);
  EXPECT(sbn_program_m_instances(kind, nodes.p, COUNT, values.p, NV, exps.p, NE, NUM_IO, nullptr, outs2.p) == SBN_OK && memcmp(outs.p, outs2.p, W * COUNT * 4) == 0);

  // ---- the check, on public inputs formed from the derived list -------------------------------------------------------------------------
  Exact<uint64_t> pi(PER * UNITS * NUM_IO);
  auto put = [&](uint64_t* p, const uint32_t* w) { for (size_t i = 0; i < PW; i++) p[i] = (w[i >> 1] >> (16 * (i & 1))) & 0xffff; };
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
  auto check = [&](uint32_t* o) { return sbn_program_m_check(kind, NUM_IO, units.p, UNITS, nodes.p, COUNT, values.p, NV, exps.p, NE, o); };
  EXPECT(check(outs2.p) == SBN_OK && memcmp(outs.p, outs2.p, W * COUNT * 4) == 0);
  EXPECT(check(nullptr) == SBN_OK);
  auto edited = [&](size_t g, size_t at, const char* a, const char* b) {
    pi.p[PER * g + at] ^= 1;
    EXPECT(check(nullptr) == SBN_ERR_VERIFY_FAILED && names(a, b));
    pi.p[PER * g + at] ^= 1;
  };
  edited(2, 3, "instance 2:", "x differs from frob_1 of the output of node 0");
  edited(3, PW + 5, "instance 3:", "offset differs from frob_3 of the output of node 0");
  edited(8, PW + PW - 1, "instance 8:", "offset differs from frob_9 of the output of node 2");
  edited(7, 0, "instance 7:", "x differs from the output of node 4");
  edited(0, 2 * PW + PE, "instance 2:", "x differs from frob_1 of the output of node 0");       // a tampered output: its first reader
  edited(11, 0, "instance 11 (pad)", "x differs from instance 10");
  edited(11, 2 * PW + PE + PW - 1, "instance 11 (pad)", "output");
  put(pi.p + PER * 2, outs.p);                                                                    // the unmapped output where a map was stated
  EXPECT(check(nullptr) == SBN_ERR_VERIFY_FAILED && names("instance 2:", "x differs from frob_1 of the output of node 0"));
  EXPECT(sbn_fq12_frobenius(outs.p, 2, mapped.p) == SBN_OK);
  put(pi.p + PER * 2, mapped.p);                                                                  // the output mapped by m + 1
  EXPECT(check(nullptr) == SBN_ERR_VERIFY_FAILED && names("instance 2:", "x differs from frob_1 of the output of node 0"));
  put(pi.p + PER * 2, ios.p + IOW * 2);
  EXPECT(check(nullptr) == SBN_OK);
  EXPECT(sbn_program_m_check(kind, NUM_IO, units.p, UNITS - 1, nodes.p, COUNT, values.p, NV, exps.p, NE, nullptr) == SBN_ERR_VERIFY_FAILED && names("2 units given"));
  units.p[2] = nullptr;
  EXPECT(check(nullptr) == SBN_ERR_BAD_ARG && names("unit 2"));

  // ---- the refusals: the twin's, then the added ones in their order ---------------------------------------------------------------------
  auto inst = [&](const sbn_program_node_m* n, size_t count, size_t nv, size_t ne, size_t num_io) { return sbn_program_m_instances(kind, n, count, values.p, nv, exps.p, ne, num_io, nullptr, nullptr); };
  EXPECT(sbn_program_m_instances(SBN_AIR_G1_EXP, nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr, nullptr) == SBN_ERR_UNSUPPORTED);
  EXPECT(inst(nullptr, COUNT, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && inst(nodes.p, 0, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && inst(nodes.p, COUNT, NV, NE, 0) == SBN_ERR_BAD_ARG);
  EXPECT(inst(nodes.p, 0x7fffffffu, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("below 2^31 - 1"));   // ... and no node is read
  Exact<sbn_program_node_m> two(2);
  two.p[0] = {0, ONE, 0, 0};
  two.p[1] = {OUT | 0, 1, 3, 0x10000u | M(12, 3)};
  EXPECT(inst(two.p, 2, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 1: exponent is index 3 of 3"));
  two.p[1] = {OUT | 0, 1, 0, 0x10000u | M(12, 3)};
  EXPECT(inst(two.p, 2, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 1: maps has bits 16..31 set"));
  two.p[1] = {OUT | 0, 1, 0, M(12, 3)};
  EXPECT(inst(two.p, 2, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 1: the map of x is 12"));
  two.p[1] = {OUT | 0, 1, 0, M(11, 3)};
  EXPECT(inst(two.p, 2, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 1: offset carries map 3 and is no link"));
  two.p[1] = {OUT | 0, ONE, 0, M(11, 3)};
  EXPECT(inst(two.p, 2, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 1: offset carries map 3 and is no link"));
  two.p[1] = {OUT | 0, OUT | 0, 0, M(11, 3)};
  EXPECT(inst(two.p, 2, NV, NE, NUM_IO) == SBN_OK);
  EXPECT(sbn_program_m_levels(two.p, 2, nullptr, nullptr) == SBN_OK);
  two.p[1] = {OUT | 0, OUT | 0, 0, M(11, 12)};
  EXPECT(sbn_program_m_levels(two.p, 2, nullptr, nullptr) == SBN_ERR_BAD_ARG && names("node 1: the map of offset is 12"));
  EXPECT(sbn_program_m_levels(nullptr, 1, nullptr, nullptr) == SBN_ERR_BAD_ARG && sbn_program_m_levels(two.p, 0, nullptr, nullptr) == SBN_ERR_BAD_ARG);
  two.p[1] = {0, 2, 0, 0};
  EXPECT(inst(two.p, 2, NV, NE, NUM_IO) == SBN_ERR_BAD_ARG && names(">= p (literal 2)"));
  EXPECT(inst(two.p, 2, 2, NE, NUM_IO) == SBN_ERR_BAD_ARG && names("node 1: offset is literal 2 of 2"));   // ... and is not read past n_values
}

// FQ_EXP takes no map: SBN_ERR_UNSUPPORTED behind the three BAD_ARG refusals; zero maps are the twin
static void fq_exp() {
  Exact<uint32_t> values(8 * 2), exps(8), outs(8 * 2), outs2(8 * 2);
  values.p[0] = 5; values.p[8] = 7; exps.p[0] = 3;
  Exact<sbn_program_node_m> two(2);
  Exact<sbn_program_node> twin(2);
  two.p[0] = {0, ONE, 0, 0}; two.p[1] = {OUT | 0, 1, 0, 0};
  twin.p[0] = {0, ONE, 0}; twin.p[1] = {OUT | 0, 1, 0};
  EXPECT(sbn_program_m_instances(SBN_AIR_FQ_EXP, two.p, 2, values.p, 2, exps.p, 1, NUM_IO, nullptr, outs.p) == SBN_OK);
  EXPECT(sbn_program_instances(SBN_AIR_FQ_EXP, twin.p, 2, values.p, 2, exps.p, 1, NUM_IO, nullptr, outs2.p) == SBN_OK && memcmp(outs.p, outs2.p, 64) == 0);
  two.p[1] = {OUT | 0, 1, 0, M(1, 0)};
  EXPECT(sbn_program_m_instances(SBN_AIR_FQ_EXP, two.p, 2, values.p, 2, exps.p, 1, NUM_IO, nullptr, nullptr) == SBN_ERR_UNSUPPORTED && names("node 1: x carries map 1"));
  two.p[1] = {OUT | 0, 1, 0, M(1, 1)};
  EXPECT(sbn_program_m_instances(SBN_AIR_FQ_EXP, two.p, 2, values.p, 2, exps.p, 1, NUM_IO, nullptr, nullptr) == SBN_ERR_BAD_ARG && names("node 1: offset carries map 1"));
}

int main() {
  helpers();
  run(SBN_AIR_FQ12_EXP, 8);
  run(SBN_AIR_FQ12_EXP_U64, 2);
  fq_exp();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("mapped programs: the maps, the inverse, the schedule, mapped links, pads, optional outputs, the check's rejections and the refusals ok\n");
  return 0;
}
