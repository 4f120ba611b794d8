// AddressSanitizer + UBSan driver of the complete sums (csrc/msm_batch.hip on instance_lists.hpp, with the units it calls:
// scalar_mul.hip, msm.hip, chain_instances.hip, tracegen.hip; tests/test_complete_sums_sanitize.py builds and runs it): on both curve
// tables, with num_io = 4 and every buffer allocated at its exact size, a list that mixes the trap of the default start, a head
// that kills candidate 0, a masked term whose words are garbage and an all-masked segment; the same call with every output
// pointer null; the list that exhausts the eight candidates; and the refusals.  The points come from the library's own explicit
// call (a final H + S is a point), so the driver needs no curve arithmetic of its own.  No kernel is launched.
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

static const size_t NUM_IO = 4;

static void run(int32_t kind, size_t W) {
  const size_t T = W + 8, IOW = 2 * W + 8;
  std::vector<uint32_t> gen(W), h0(W);
  EXPECT(sbn_curve_generator(kind, gen.data()) == SBN_OK && sbn_start_candidate(kind, 0, h0.data()) == SBN_OK);

  // ---- the mixed list: segments of 1, 3, 1, 4 -----------------------------------------------------------------------------------
  const uint64_t lengths_v[4] = {1, 3, 1, 4};
  const size_t M = 9, S = 4, units = (M + NUM_IO - 1) / NUM_IO;
  Exact<uint64_t> lengths(S);
  memcpy(lengths.p, lengths_v, sizeof lengths_v);
  Exact<uint32_t> terms(T * M);
  Exact<uint8_t> mask(M);
  auto term = [&](size_t g, const uint32_t* x, uint32_t e0, uint32_t e7) { memcpy(terms.p + T * g, x, W * 4); terms.p[T * g + W] = e0; terms.p[T * g + W + 7] = e7; };
  term(0, gen.data(), 0xdeadbeefu | 1, 0x0fffffffu);          // sk G: the default start refuses it
  term(1, h0.data(), 7, 0);                                   // a head that kills candidate 0
  term(2, gen.data(), 0, 0);                                  // a zero scalar
  memset(terms.p + T * 3, 0xff, T * 4); mask.p[3] = 1;        // masked: words >= p, never read
  memset(terms.p + T * 4, 0xff, T * 4); mask.p[4] = 1;        // an all-masked segment
  term(5, gen.data(), 5, 0);
  term(6, gen.data(), 5, 0);                                  // a repeated point
  term(7, h0.data(), 2, 1);
  term(8, gen.data(), 3, 0x10000000u);
  {
    Exact<uint32_t> ios(IOW * units * NUM_IO), eff(T * M), starts(W * S), finals(W * S), sums(W * S);
    Exact<uint8_t> choice(S), inf(S);
    EXPECT(sbn_msm_batch_instances_complete(kind, terms.p, mask.p, lengths.p, S, NUM_IO, ios.p, eff.p, starts.p, choice.p, finals.p, sums.p, inf.p) == SBN_OK);
    EXPECT(choice.p[0] == 0 && choice.p[1] == 1 && choice.p[2] == 0 && choice.p[3] == 0);
    EXPECT(inf.p[0] == 0 && inf.p[1] == 0 && inf.p[2] == 1 && inf.p[3] == 0);
    EXPECT(memcmp(finals.p + W * 2, starts.p + W * 2, W * 4) == 0);                       // a sum at infinity: final = start
    EXPECT(memcmp(eff.p + T * 3, gen.data(), W * 4) == 0 && eff.p[T * 3 + W] == 0 && eff.p[T * 4 + W + 7] == 0);
    EXPECT(memcmp(ios.p + IOW * (M + 2), ios.p + IOW * (M - 1), IOW * 4) == 0);           // the pads copy row M - 1
    // the defining property: the explicit call on (terms_eff, starts) gives the same words
    Exact<uint32_t> ios2(IOW * units * NUM_IO), finals2(W * S), sums2(W * S);
    Exact<uint8_t> inf2(S);
    EXPECT(sbn_msm_batch_instances(kind, eff.p, lengths.p, S, starts.p, S, NUM_IO, ios2.p, finals2.p, sums2.p, inf2.p) == SBN_OK);
    EXPECT(memcmp(ios.p, ios2.p, IOW * units * NUM_IO * 4) == 0 && memcmp(finals.p, finals2.p, W * S * 4) == 0);
    EXPECT(memcmp(sums.p, sums2.p, W * S * 4) == 0 && memcmp(inf.p, inf2.p, S) == 0);
    // every output pointer is optional, alone and together
    EXPECT(sbn_msm_batch_instances_complete(kind, terms.p, mask.p, lengths.p, S, NUM_IO, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SBN_OK);
    Exact<uint8_t> only(S);
    EXPECT(sbn_msm_batch_instances_complete(kind, terms.p, mask.p, lengths.p, S, NUM_IO, nullptr, nullptr, nullptr, only.p, nullptr, nullptr, nullptr) == SBN_OK);
    EXPECT(memcmp(only.p, choice.p, S) == 0);
  }

  // ---- the list that exhausts the candidates: e_g = 1, x_g = H_g + S_{g-1} = the final of x_0 .. x_{g-1} started from H_g ------------
  {
    const size_t K = SBN_START_CANDIDATES;
    Exact<uint32_t> kt(T * K);
    for (size_t g = 0; g < K; g++) {
      std::vector<uint32_t> hg(W), x(W);
      EXPECT(sbn_start_candidate(kind, (uint32_t)g, hg.data()) == SBN_OK);
      const uint64_t len = g;
      if (g == 0) x = hg;
      else EXPECT(sbn_msm_batch_instances(kind, kt.p, &len, 1, hg.data(), 1, NUM_IO, nullptr, x.data(), nullptr, nullptr) == SBN_OK);
      memcpy(kt.p + T * g, x.data(), W * 4);
      kt.p[T * g + W] = 1;
    }
    const uint64_t len = K;
    Exact<uint8_t> choice(1);
    choice.p[0] = 9;
    EXPECT(sbn_msm_batch_instances_complete(kind, kt.p, nullptr, &len, 1, NUM_IO, nullptr, nullptr, nullptr, choice.p, nullptr, nullptr, nullptr) == SBN_ERR_WITNESS);
    EXPECT(sbn::g_last_error.find("segment 0") != std::string::npos && sbn::g_last_error.find("instance 7") != std::string::npos && choice.p[0] == 9);
    Exact<uint8_t> all(K);                                                                // ... and with every term masked it is the empty sum
    memset(all.p, 1, K);
    Exact<uint8_t> inf(1);
    EXPECT(sbn_msm_batch_instances_complete(kind, kt.p, all.p, &len, 1, NUM_IO, nullptr, nullptr, nullptr, choice.p, nullptr, nullptr, inf.p) == SBN_OK);
    EXPECT(choice.p[0] == 0 && inf.p[0] == 1);
  }

  // ---- the refusals ---------------------------------------------------------------------------------------------------------------
  EXPECT(sbn_msm_batch_instances_complete(kind, nullptr, nullptr, lengths.p, S, NUM_IO, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SBN_ERR_BAD_ARG);
  EXPECT(sbn_msm_batch_instances_complete(kind, terms.p, nullptr, lengths.p, 0, NUM_IO, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SBN_ERR_BAD_ARG);
  EXPECT(sbn_msm_batch_instances_complete(kind, terms.p, nullptr, lengths.p, S, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SBN_ERR_BAD_ARG);
  EXPECT(sbn_msm_batch_instances_complete(kind, terms.p, nullptr, lengths.p, S, NUM_IO, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SBN_ERR_BAD_ARG);
  EXPECT(sbn::g_last_error.find("instance 3, segment 1") != std::string::npos);           // unmasked, the words of term 3 are >= p
  std::vector<uint32_t> out(W);
  EXPECT(sbn_start_candidate(kind, SBN_START_CANDIDATES, out.data()) == SBN_ERR_BAD_ARG && sbn_start_candidate(SBN_AIR_FQ_EXP, 0, out.data()) == SBN_ERR_UNSUPPORTED);
  EXPECT(sbn_msm_batch_instances_complete(SBN_AIR_FQ_EXP, terms.p, nullptr, lengths.p, S, NUM_IO, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SBN_ERR_UNSUPPORTED);
}

int main() {
  run(SBN_AIR_G1_EXP, 16);
  run(SBN_AIR_G2_EXP, 32);
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("complete sums: choices, masks, the exhausted list, optional outputs and refusals ok\n");
  return 0;
}
