// Every SBN_* environment switch of the library, read in ONE place.
//
// A prover reads the environment once, when it is created (create_ctx -> Settings::load), checks every value and keeps the
// resolved set for its lifetime (sbn_prover_describe prints it; bench.py copies it into `config`).  Two classes:
//   * production switches (host thread count, collective timeout, RCCL path, timing print, AVX-512 opt-out, chain placement of
//     the curve witness, reuse of the shape-constant columns' transforms) are always honoured;
//   * EXPERIMENT switches (A/B forms of kernels kept for measurement: every one of them yields the same proof bytes,
//     profiles/r4_v5_switch_parity.txt) are honoured only when SBN_EXPERIMENTAL=1 is set as well -- a stale export in a
//     production shell can then not change which kernels run or how long they take; without it they are reported as
//     ignored.  The A/B forms that lost their measurement have been retired with their switches; the transform plan (fused
//     passes, transform streams, the split 1,024-point pass) depends on the table size alone.
// A value that is not understood is an error (SBN_ERR_BAD_ARG), never a silent default.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

namespace sbn {

struct Settings {
  // ---- production ----
  int host_threads = 0;          // SBN_HOST_THREADS: worker threads of the host pool (0 = one per visible CPU, at most 64)
  double comm_timeout_s = 600;   // SBN_COMM_TIMEOUT_S: deadline of every wait on another rank of a split proof
  std::string rccl_lib;          // SBN_RCCL_LIB: path of librccl (default: the loader's search path, then /opt/rocm/lib)
  bool trace_timing = false;     // SBN_TRACE_TIMING: print per-kernel times of the device witness generation
  bool no_avx512 = false;        // SBN_NO_AVX512: scalar host transcript permutation
  int device_chain = -1;         // SBN_TRACEGEN_DEVICE_CHAIN: -1 auto (host pool with >= 8 threads, else 2), 0 host pool,
                                 //   1 one lane per instance, 2 one wave per instance (tg::chain_coop_kernel)
  bool fixed_columns = true;     // SBN_FIXED_COLUMNS=0: transform the shape-constant trace columns of an Exp table in every proof, as if
                                 //   their transforms were never resident (prover.hip stage_trace_commit); the same proof words
  bool experimental = false;     // SBN_EXPERIMENTAL=1
  // ---- experiments (need SBN_EXPERIMENTAL=1) ----
  int ntt_chunk = 0;             // SBN_NTT_CHUNK: columns per commit-pipeline chunk (0 = size-dependent default)
  bool fq12_host_chain = false;  // SBN_FQ12_HOST_CHAIN=1: Fq12 square-and-multiply chains on the host pool
  bool fq12_row_kernel = false;  // SBN_FQ12_ROW_KERNEL=1: round 2's one lane per row
  int range_check = 0;           // SBN_RANGE_CHECK: 0 default, 1 = the round-3 kernel (one lane per 64 consecutive values)
  int quotient_lookups = 0;      // SBN_QUOTIENT_LOOKUPS=1: the lookup constraints of the u16 range check beside the permutation checks instead of in the AIR tail segment (measured slower)
  std::string ignored;           // experiment switches that were set without SBN_EXPERIMENTAL=1

  // Reads the environment.  false: `err` names the variable whose value is not understood.
  bool load(std::string& err) {
    auto get = [](const char* n) -> const char* { const char* v = getenv(n); return v && *v ? v : nullptr; };
    auto integer = [&](const char* n, long lo, long hi, long* out) -> bool {   // true: unset or valid
      const char* v = get(n);
      if (!v) return true;
      char* end = nullptr;
      const long x = strtol(v, &end, 10);
      if (!end || *end || x < lo || x > hi) { err = std::string(n) + "=" + v + " is not an integer in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]"; return false; }
      *out = x;
      return true;
    };
    long x;
    x = 0; if (!integer("SBN_HOST_THREADS", 1, 256, &x)) return false; host_threads = (int)x;
    if (const char* v = get("SBN_COMM_TIMEOUT_S")) {
      char* end = nullptr;
      const double t = strtod(v, &end);
      if (!end || *end || !(t > 0)) { err = std::string("SBN_COMM_TIMEOUT_S=") + v + " is not a positive number of seconds"; return false; }
      comm_timeout_s = t;
    }
    if (const char* v = get("SBN_RCCL_LIB")) rccl_lib = v;
    trace_timing = get("SBN_TRACE_TIMING") != nullptr;
    no_avx512 = get("SBN_NO_AVX512") != nullptr;
    x = -1; if (!integer("SBN_TRACEGEN_DEVICE_CHAIN", 0, 2, &x)) return false; device_chain = (int)x;
    x = 1; if (!integer("SBN_FIXED_COLUMNS", 0, 1, &x)) return false; fixed_columns = x == 1;
    x = 0; if (!integer("SBN_EXPERIMENTAL", 0, 1, &x)) return false; experimental = x == 1;
    static const char* const EXP[] = {"SBN_NTT_CHUNK", "SBN_FQ12_HOST_CHAIN", "SBN_FQ12_ROW_KERNEL", "SBN_RANGE_CHECK", "SBN_QUOTIENT_LOOKUPS"};
    if (!experimental) {
      for (const char* n : EXP) if (get(n)) { if (!ignored.empty()) ignored += ","; ignored += n; }
      return true;
    }
    x = 0; if (!integer("SBN_NTT_CHUNK", 8, 256, &x)) return false;
    if (x % 8) { err = "SBN_NTT_CHUNK must be a multiple of 8 between 8 and 256"; return false; }
    ntt_chunk = (int)x;
    x = 0; if (!integer("SBN_FQ12_HOST_CHAIN", 0, 1, &x)) return false; fq12_host_chain = x != 0;
    x = 0; if (!integer("SBN_FQ12_ROW_KERNEL", 0, 1, &x)) return false; fq12_row_kernel = x != 0;
    x = 0; if (!integer("SBN_RANGE_CHECK", 0, 1, &x)) return false; range_check = (int)x;
    x = 0; if (!integer("SBN_QUOTIENT_LOOKUPS", 0, 1, &x)) return false; quotient_lookups = (int)x;
    return true;
  }
  // The environment of a caller that has no prover (library-level entry points): invalid values fall back to the defaults.
  static Settings from_env_or_default() { Settings s; std::string e; if (!s.load(e)) s = Settings(); return s; }
};

}  // namespace sbn
