// Explain on the device (include/sbn.h, sbn_prover_explain_rows / sbn_prover_explain_trace): which constraint BLOCKS the rows of
// the loaded trace break.  One thread per trace row reads the column-major d_trace as the check kernels do (row i against row
// i + 1 mod N, lanes = consecutive rows: coalesced) and runs the table's evaluator of air.cuh through the RECORDING consumer of
// air_record.cuh.  The emission sequence is the same in every lane, so in the whole-trace form a wave ballots the "non-zero" bit
// of every block and one lane issues one atomicAdd and one atomicMin per (wave, failing block): a trace on which every row
// fails costs one pair of atomics per wave and block, a clean block nothing.  The listed-rows form runs the same code with
// uncoalesced loads (the list is short) and every thread sets bits in the bitmap of its own row.
// The Z columns need no evaluator: a second kernel forms (Z_z - 1) L_first and the transition of every (row, z) directly.
// Shared with the check: launch_perm_z, upload_alpha_tables, the tables of the trace domain, the seed-to-challenge transcript.
// Scratch is per-proof scratch only: the tables of H in d_zpow, the statistics in d_open / h_open, the listed rows and their
// bitmaps in d_part (free once Z is written); a context that never explains allocates nothing for it.
#include "prover_ctx.hpp"
#include "kernels_explain.cuh"

__device__ __forceinline__ void explain_pair(int kind, const ExpShape& es, int z, int& l, int& r) {
  if (kind == SBN_AIR_G1_OP) G1OpShape::pair(z, l, r);
  else if (kind == SBN_AIR_LOOKUP) LookupShape().pair(z, l, r);
  else if (kind == SBN_AIR_MODULAR || kind == SBN_AIR_FQ12_MUL) OpShape(kind).pair(z, l, r);
  else es.pair(z, l, r);
}
__device__ __forceinline__ int explain_exp_e(int kind) { return kind == SBN_AIR_FQ12_EXP ? 12 : (kind == SBN_AIR_FQ12_EXP_U64 ? 13 : (kind == SBN_AIR_G2_EXP ? 2 : (kind == SBN_AIR_FQ_EXP ? 0 : 1))); }
// permutation.rs eval_permutation_checks for Z column z on row i: the first-row constraint or the transition is non-zero
__device__ __forceinline__ bool explain_z_nonzero(const ExplainParams& p, size_t i, int z, int lc, int rc) {
  const size_t n = p.n, inext = (i + 1) & (n - 1);
  const F g0(p.gamma0), g1(p.gamma1), one(1);
  const F l(p.trace[(size_t)lc * n + i]), r(p.trace[(size_t)rc * n + i]), zl(p.zval[(size_t)z * n + i]), zn(p.zval[(size_t)z * n + inext]);
  const F t = zn * ((r + g0) * (r + g1)) - zl * ((l + g0) * (l + g1));
  const F f = (zl - one) * F(p.lag_first[i]);
  return t.v != 0 || f.v != 0;
}
// whole-trace form: grid (n / 256, Z columns); the same ballot-and-atomic reduction as the blocks
__global__ __launch_bounds__(256) void explain_z_trace_kernel(ExplainParams p) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < p.n;
  const ExpShape es(explain_exp_e(p.kind), p.num_io);
  for (int z = blockIdx.y; z < p.num_zs; z += gridDim.y) {
    int lc, rc;
    explain_pair(p.kind, es, z, lc, rc);
    const bool nz = live && explain_z_nonzero(p, live ? i : 0, z, lc, rc);
    const unsigned long long b = __ballot(nz);
    if (b && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) {
      atomicAdd(&p.zstats[z], (unsigned long long)__popcll(b));
      atomicMin(&p.zstats[p.num_zs + z], (unsigned long long)i);
    }
  }
}
// listed-rows form: one thread per listed row walks the Z columns and owns the bytes it writes
__global__ __launch_bounds__(256) void explain_z_rows_kernel(ExplainParams p) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.n_rows) return;
  const size_t i = (size_t)p.rows[k];
  const ExpShape es(explain_exp_e(p.kind), p.num_io);
  unsigned char* out = p.zbits + k * p.zbytes;
  for (int z0 = 0; z0 < p.num_zs; z0 += 8) {
    u32 byte = 0;
    for (int z = z0; z < z0 + 8 && z < p.num_zs; z++) {
      int lc, rc;
      explain_pair(p.kind, es, z, lc, rc);
      if (explain_z_nonzero(p, i, z, lc, rc)) byte |= 1u << (z - z0);
    }
    out[z0 >> 3] = (unsigned char)byte;
  }
}

static void launch_explain_kernel(int kind, dim3 grid, hipStream_t st, const ExplainParams& ep, const u64* apow0, const u64* apow1, const void* pic) {
#define SBN_EXPLAIN_KIND(K) hipLaunchKernelGGL(explain_kernel<K>, grid, dim3(256), 0, st, ep, apow0, apow1, pic); break;
  switch (kind) {
    case SBN_AIR_FQ12_EXP: case SBN_AIR_FQ12_EXP_U64: case SBN_AIR_FQ12_MUL: launch_explain_kernel_fq12(kind, grid, st, ep, apow0, apow1, pic); break;
    case SBN_AIR_G1_OP: SBN_EXPLAIN_KIND(1)
    case SBN_AIR_G1_EXP: SBN_EXPLAIN_KIND(2)
    case SBN_AIR_G2_EXP: SBN_EXPLAIN_KIND(3)
    case SBN_AIR_FQ_EXP: SBN_EXPLAIN_KIND(5)
    case SBN_AIR_MODULAR: SBN_EXPLAIN_KIND(7)
    case SBN_AIR_LOOKUP: SBN_EXPLAIN_KIND(9)
    case SBN_AIR_FLAGS: SBN_EXPLAIN_KIND(10)
    default: SBN_EXPLAIN_KIND(11)
  }
#undef SBN_EXPLAIN_KIND
}

// rows == null: the whole-trace form into bstats / zstats; else the listed-rows form into bflags / zflags
static int explain_device(sbn_prover* P, uint64_t seed, const uint64_t* rows, size_t n_rows, uint8_t* bflags, uint8_t* zflags,
                          sbn_block_stat* bstats, sbn_block_stat* zstats) {
  if (!P) return fail(SBN_ERR_BAD_ARG, "null argument");
  if (P->sp && P->sp->comm.world > 1) return fail(SBN_ERR_UNSUPPORTED, "explain runs on single-GPU provers (this one is rank %u of %u)", P->sp->comm.rank, P->sp->comm.world);
  if (!P->loaded) return fail(SBN_ERR_BAD_ARG, "no trace loaded");
  const size_t n = P->n, Z = P->air.nzs, C = P->air.ncols;
  for (size_t k = 0; k < n_rows; k++) if (rows[k] >= n) return fail(SBN_ERR_BAD_ARG, "row %llu of a trace of %zu rows", (unsigned long long)rows[k], n);
  const sbn_air_desc desc{P->air.kind, P->air.num_io};
  const size_t B = sbn_air_constraint_blocks(&desc, nullptr, 0);
  if (!B) return SBN_ERR_BAD_ARG;
  if (2 * (B + Z) > (C + Z + 4) * 4) return fail(SBN_ERR_UNSUPPORTED, "%zu blocks do not fit the scratch of this context", B);
  HIPC(hipSetDevice(P->device));
  hipStream_t st = P->stream;
  hipEvent_t* ev = P->ev;   // the stage events are idle outside prove()
  int rc;
  F gamma0, gamma1, alphas[SBN_NCH];
  check_challenges(P->air, P->degree_bits, P->pi.data(), P->pi.size(), seed, gamma0, gamma1, alphas);

  HIPC(hipEventRecord(ev[0], st));
  if (Z) launch_perm_z(P, P->sp ? P->sp->d_pairs_own : P->d_pairs, Z, gamma0.v, gamma1.v, P->d_zval, st);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(ev[1], st));

  ExplainParams ep{};
  ep.trace = P->d_trace; ep.zval = P->d_zval; ep.n = n;
  ep.xs = P->d_zpow; ep.lag_first = P->d_zpow + n; ep.lag_last = P->d_zpow + 2 * n;
  ep.last = f_inv(f_root_of_unity(P->degree_bits)).v;
  launch_trace_domain_tables(P->d_zpow, P->d_zpow + n, P->d_zpow + 2 * n, n, P->degree_bits, st);
  HIPC(hipGetLastError());
  if ((rc = upload_alpha_tables(P, alphas))) return rc;
  for (int j = 0; j < SBN_NCH; j++) ep.alpha[j] = alphas[j].v;
  ep.gamma0 = gamma0.v; ep.gamma1 = gamma1.v;
  ep.kind = P->air.kind; ep.num_io = (int)P->air.num_io; ep.nconstraints = (int)P->air.nconstraints; ep.num_zs = (int)Z;
  const u64 *apow0 = P->d_apow, *apow1 = P->d_apow + P->apow_n;
  ep.nblk = (u32)B; ep.bbytes = (u32)((B + 7) / 8); ep.zbytes = (u32)((Z + 7) / 8);

  if (!rows) {
    unsigned long long* d_stats = (unsigned long long*)P->d_open;   // [B counts][B first rows][Z counts][Z first rows]
    ep.stats = d_stats; ep.zstats = d_stats + 2 * B;
    HIPC(hipMemsetAsync(d_stats, 0, B * sizeof(u64), st));
    HIPC(hipMemsetAsync(d_stats + B, 0xff, B * sizeof(u64), st));
    if (Z) {
      HIPC(hipMemsetAsync(ep.zstats, 0, Z * sizeof(u64), st));
      HIPC(hipMemsetAsync(ep.zstats + Z, 0xff, Z * sizeof(u64), st));
    }
    launch_explain_kernel(ep.kind, dim3((unsigned)((n + 255) / 256)), st, ep, apow0, apow1, P->d_pic);
    HIPC(hipGetLastError());
    if (Z) {
      hipLaunchKernelGGL(explain_z_trace_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)std::min<size_t>(Z, 65535)), dim3(256), 0, st, ep);
      HIPC(hipGetLastError());
    }
    HIPC(hipEventRecord(ev[2], st));
    HIPC(hipMemcpyAsync(P->h_open, d_stats, 2 * (B + Z) * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPC(hipEventRecord(ev[3], st));
    HIPC(hipStreamSynchronize(st));
    const u64* h = P->h_open;
    for (size_t b = 0; b < B; b++) bstats[b] = sbn_block_stat{h[b], h[B + b]};
    if (zstats) for (size_t z = 0; z < Z; z++) zstats[z] = sbn_block_stat{h[2 * B + z], h[2 * B + Z + z]};
  } else {
    // the listed rows and their bitmaps in d_part (64 n words; Z is written, the chunk products of launch_perm_z are done with it
    // on this stream), a chunk of the list at a time
    const size_t per_row = sizeof(u64) + ep.bbytes + ep.zbytes, room = (size_t)64 * n * sizeof(u64);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(room / per_row, 65536));
    for (size_t k0 = 0; k0 < n_rows; k0 += chunk) {
      const size_t cnt = std::min(chunk, n_rows - k0);
      u64* d_rows = P->d_part;
      unsigned char* d_bits = (unsigned char*)(d_rows + cnt);
      unsigned char* d_zbits = d_bits + cnt * ep.bbytes;
      HIPC(hipMemcpyAsync(d_rows, rows + k0, cnt * sizeof(u64), hipMemcpyHostToDevice, st));
      HIPC(hipMemsetAsync(d_bits, 0, cnt * (ep.bbytes + ep.zbytes), st));
      ep.rows = d_rows; ep.n_rows = cnt; ep.bits = d_bits; ep.zbits = d_zbits;
      launch_explain_kernel(ep.kind, dim3((unsigned)((cnt + 255) / 256)), st, ep, apow0, apow1, P->d_pic);
      HIPC(hipGetLastError());
      if (Z && zflags) {
        hipLaunchKernelGGL(explain_z_rows_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, ep);
        HIPC(hipGetLastError());
      }
      HIPC(hipStreamSynchronize(st));
      HIPC(hipMemcpy(bflags + k0 * ep.bbytes, d_bits, cnt * ep.bbytes, hipMemcpyDeviceToHost));   // the caller's memory is pageable: plain copies
      if (Z && zflags) HIPC(hipMemcpy(zflags + k0 * ep.zbytes, d_zbits, cnt * ep.zbytes, hipMemcpyDeviceToHost));
    }
    HIPC(hipEventRecord(ev[2], st));
    HIPC(hipEventRecord(ev[3], st));
    HIPC(hipStreamSynchronize(st));
  }
  for (int k = 0; k < 3; k++) HIPC(hipEventElapsedTime(&P->explain_ms[k], ev[k], ev[k + 1]));
  return SBN_OK;
}

extern "C" int sbn_prover_explain_rows(sbn_prover* P, uint64_t seed, const uint64_t* rows, size_t n_rows, uint8_t* block_flags_out, uint8_t* z_flags_out) {
  if (!P || (n_rows && (!rows || !block_flags_out))) return fail(SBN_ERR_BAD_ARG, "null argument");
  static const uint64_t none = 0;
  return explain_device(P, seed, rows ? rows : &none, n_rows, block_flags_out, z_flags_out, nullptr, nullptr);
}
extern "C" int sbn_prover_explain_trace(sbn_prover* P, uint64_t seed, sbn_block_stat* block_stats_out, sbn_block_stat* z_stats_out) {
  if (!P || !block_stats_out) return fail(SBN_ERR_BAD_ARG, "null argument");
  return explain_device(P, seed, nullptr, 0, nullptr, nullptr, block_stats_out, z_stats_out);
}
extern "C" int sbn_prover_explain_times(const sbn_prover* P, float* ms, int cap) {
  if (!P || !ms) return 0;
  const int k = std::min(cap, 3);
  for (int i = 0; i < k; i++) ms[i] = P->explain_ms[i];
  return k;
}
