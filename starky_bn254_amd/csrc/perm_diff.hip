// The values and rows behind a failing permutation pair (include/sbn.h, sbn_explain_permutations_host /
// sbn_prover_explain_permutations): the lhs column of every chosen pair against its rhs column as multisets of canonical words.
// The host form is perm_diff.hpp on the host pool, one pair per task.  The device form streams the resident d_trace through the
// signed LDS histograms of kernels_permdiff.cuh and finishes on the host; a pair ends on one of three ROUTES:
//   0  bins      every cell of the pair is below 2^16 (every pair of a right trace but LookupStark's): statistics and entries come
//                from the two kernels alone.
//   1  list      some cells are >= 2^16 and all such cells of the launch fitted the overflow list (LIST_CAP cells): the list is
//                grouped by pair and diffed by perm_diff.hpp's diff_cells; its values follow the binned ones, they are all larger.
//   2  download  the list overflowed (every pair with a cell >= 2^16 then), or per_pair > DEV_CAP and the pair has more binned
//                differing values than the rows pass holds: both columns are downloaded and diffed by diff_columns.
// Every route is exact.  Scratch is P->d_part alone (per-proof scratch, 64 n words): the pairs are taken in chunks that fit it.
#include "prover_ctx.hpp"
#include "trace_host.hpp"
#include "perm_diff.hpp"
#include "kernels_permdiff.cuh"
#include <atomic>
#include <chrono>

static_assert(sizeof(PermStat) == sizeof(sbn_perm_pair_stat) && sizeof(PermEntry) == sizeof(sbn_perm_diff_entry), "perm_diff.hpp mirrors include/sbn.h");
static constexpr unsigned LIST_CAP = 4096;   // cells of the overflow list: 64 KiB

// perm_hist_kernel keeps 128 KiB of bins in LDS (> the 64 KiB default); idempotent, per device (see range_check_setup)
static int perm_hist_setup(int device) {
  static std::atomic<bool> done[SBN_MAX_DEVICES];
  const int d = device >= 0 && device < SBN_MAX_DEVICES ? device : 0;
  if (!done[d].load()) {
    HIPC(hipFuncSetAttribute((const void*)pd::perm_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pd::HIST_LDS_BYTES));
    done[d].store(true);
  }
  return 0;
}

// The pairs of the call as columns: zs == null: all of them
static int chosen_pairs(const AirShape& as, const uint32_t* zs, size_t n_zs, std::vector<pd::Cols>& cols) {
  const size_t K = zs ? n_zs : as.nzs;
  cols.resize(K);
  for (size_t k = 0; k < K; k++) {
    const size_t z = zs ? zs[k] : k;
    if (z >= as.nzs) return fail(SBN_ERR_BAD_ARG, "pair %zu of a table of %zu Z columns", z, as.nzs);
    air_pair(as, z, cols[k].lhs, cols[k].rhs);
  }
  return SBN_OK;
}

extern "C" int sbn_explain_permutations_host(const sbn_air_desc* air, const uint64_t* trace, uint32_t degree_bits, const uint32_t* zs, size_t n_zs,
                                             size_t per_pair, sbn_perm_pair_stat* stats_out, sbn_perm_diff_entry* entries_out) {
  if (!air || !trace) return fail(SBN_ERR_BAD_ARG, "null argument");
  AirShape as;
  if (int rc = host_table_check(air, degree_bits, as)) return rc;
  std::vector<pd::Cols> cols;
  if (int rc = chosen_pairs(as, zs, n_zs, cols)) return rc;
  if (!cols.empty() && (!stats_out || (per_pair && !entries_out))) return fail(SBN_ERR_BAD_ARG, "null argument");
  const size_t n = (size_t)1 << degree_bits;
  if (int rc = host_canonical_check(trace, as.ncols * n)) return rc;
  host_parallel_for(cols.size(), [&](size_t k) {
    diff_columns(trace + (size_t)cols[k].lhs * n, trace + (size_t)cols[k].rhs * n, n, per_pair, *(PermStat*)&stats_out[k],
                 per_pair ? (PermEntry*)entries_out + k * per_pair : nullptr);
  });
  return SBN_OK;
}

extern "C" int sbn_prover_explain_permutations(sbn_prover* P, const uint32_t* zs, size_t n_zs, size_t per_pair, sbn_perm_pair_stat* stats_out,
                                               sbn_perm_diff_entry* entries_out) {
  if (int rc = diag_enter(P, "explain", false)) return rc;
  std::vector<pd::Cols> cols;
  if (int rc = chosen_pairs(P->air, zs, n_zs, cols)) return rc;
  const size_t K = cols.size(), n = P->n;
  if (K && (!stats_out || (per_pair && !entries_out))) return fail(SBN_ERR_BAD_ARG, "null argument");
  float* const times = P->diag_ms[DIAG_PERMDIFF];
  for (int i = 0; i < 3; i++) { times[i] = 0; P->permdiff_routes[i] = 0; }
  if (!K) return SBN_OK;
  if (int rc = perm_hist_setup(P->device)) return rc;
  hipStream_t st = P->stream;
  hipEvent_t* ev = P->ev;

  // d_part: [list count, 16 bytes][statistics][half counts][entries] -- the block that comes back -- then the list, the candidate
  // slots and the columns of the pairs
  const unsigned cap = (unsigned)std::min<size_t>(per_pair, pd::DEV_CAP);
  const size_t room = (size_t)64 * n * sizeof(u64), fixed = 32 + (size_t)LIST_CAP * sizeof(pd::Cell);   // (the count, the list, its alignment)
  const size_t per = 4 * sizeof(u64) + 2 * sizeof(unsigned) + (size_t)cap * sizeof(pd::Entry) + 2 * (size_t)cap * sizeof(unsigned) + sizeof(pd::Cols);
  const size_t chunk = std::min<size_t>({K, (room - fixed) / per, (size_t)65535});
  if (!chunk) return fail(SBN_ERR_UNSUPPORTED, "the scratch of this context holds no pair");
  char* const base = (char*)P->d_part;
  std::vector<u64> h_head(2 + chunk * 5), colL, colR;
  std::vector<pd::Entry> h_entries((size_t)chunk * cap);
  std::vector<pd::Cell> h_list;
  std::vector<PermCell> cl, cr;

  for (size_t k0 = 0; k0 < K; k0 += chunk) {
    const size_t cnt = std::min(chunk, K - k0);
    pd::Params p{};
    p.trace = (const pd::ull*)P->d_trace; p.n = n; p.cap = cap; p.list_cap = LIST_CAP;
    char* q = base;
    p.list_count = (pd::ull*)q; q += 16;
    p.stats = (pd::ull*)q; q += cnt * 4 * sizeof(u64);
    p.half_count = (unsigned*)q; q += cnt * 2 * sizeof(unsigned);
    p.entries = (pd::Entry*)q; q += cnt * cap * sizeof(pd::Entry);
    q = base + (((size_t)(q - base) + 15) & ~(size_t)15);
    p.list = (pd::Cell*)q; q += (size_t)LIST_CAP * sizeof(pd::Cell);
    p.cand = (unsigned*)q; q += cnt * 2 * cap * sizeof(unsigned);
    pd::Cols* d_cols = (pd::Cols*)q; q += cnt * sizeof(pd::Cols);
    p.cols = d_cols;
    if ((size_t)(q - base) > room) return fail(SBN_ERR_UNSUPPORTED, "internal: the pairs of a chunk do not fit the scratch");
    HIPC(hipMemcpyAsync(d_cols, cols.data() + k0, cnt * sizeof(pd::Cols), hipMemcpyHostToDevice, st));
    HIPC(hipMemsetAsync(base, 0, 16 + cnt * 4 * sizeof(u64), st));
    HIPC(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(pd::perm_hist_kernel, dim3(2, (unsigned)cnt), dim3(pd::THREADS), pd::HIST_LDS_BYTES, st, p);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], st));
    if (cap) {
      hipLaunchKernelGGL(pd::perm_rows_kernel, dim3((unsigned)cnt), dim3(pd::THREADS), 0, st, p);
      HIPC(hipGetLastError());
    }
    HIPC(hipEventRecord(ev[2], st));
    HIPC(hipStreamSynchronize(st));
    float ms;
    for (int i = 0; i < 2; i++) { HIPC(hipEventElapsedTime(&ms, ev[i], ev[i + 1])); times[i] += ms; }

    const auto t0 = std::chrono::steady_clock::now();
    // the count, the statistics and the half counts lie together; the caller's memory and these vectors are pageable: plain copies
    HIPC(hipMemcpy(h_head.data(), base, 16 + cnt * 5 * sizeof(u64), hipMemcpyDeviceToHost));
    const u64 listed = h_head[0], *h_stats = h_head.data() + 2;
    const unsigned* h_half = (const unsigned*)(h_stats + 4 * cnt);
    bool any = false;
    for (size_t k = 0; k < cnt && !any; k++) any = h_stats[4 * k] != 0;
    if (any && cap) HIPC(hipMemcpy(h_entries.data(), p.entries, cnt * cap * sizeof(pd::Entry), hipMemcpyDeviceToHost));
    const bool overflowed = listed > LIST_CAP;
    if (listed && !overflowed) {
      h_list.resize((size_t)listed);
      HIPC(hipMemcpy(h_list.data(), p.list, (size_t)listed * sizeof(pd::Cell), hipMemcpyDeviceToHost));
      std::sort(h_list.begin(), h_list.end(), [](const pd::Cell& a, const pd::Cell& b) { return a.pair < b.pair; });
    }
    size_t li = 0;   // walks the sorted list
    for (size_t k = 0; k < cnt; k++) {
      PermStat& s = *(PermStat*)&stats_out[k0 + k];
      PermEntry* out = per_pair ? (PermEntry*)entries_out + (k0 + k) * per_pair : nullptr;
      const u64 binned = h_stats[4 * k], outside = h_stats[4 * k + 3];
      if ((outside && overflowed) || (binned > cap && per_pair > cap)) {
        colL.resize(n); colR.resize(n);
        HIPC(hipMemcpy(colL.data(), P->d_trace + (size_t)cols[k0 + k].lhs * n, n * sizeof(u64), hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(colR.data(), P->d_trace + (size_t)cols[k0 + k].rhs * n, n * sizeof(u64), hipMemcpyDeviceToHost));
        diff_columns(colL.data(), colR.data(), n, per_pair, s, out);
        P->permdiff_routes[2]++;
        continue;
      }
      s = PermStat{binned, h_stats[4 * k + 1], h_stats[4 * k + 2], std::min<u64>(binned, cap)};
      if (h_half[2 * k] + (u64)h_half[2 * k + 1] != binned) return fail(SBN_ERR_HIP, "internal: the halves of pair %zu disagree with its statistics", k0 + k);
      for (size_t i = 0; i < s.entries; i++) {
        const pd::Entry& e = h_entries[k * cap + i];
        out[i] = PermEntry{e.value, e.count_lhs, e.count_rhs, e.first_row_lhs == pd::NO_ROW ? PERM_NO_ROW : e.first_row_lhs,
                           e.first_row_rhs == pd::NO_ROW ? PERM_NO_ROW : e.first_row_rhs};
      }
      if (!outside) { P->permdiff_routes[0]++; continue; }
      cl.clear(); cr.clear();
      while (li < h_list.size() && h_list[li].pair < k) li++;
      for (; li < h_list.size() && h_list[li].pair == k; li++)
        (h_list[li].side_row >> 31 ? cr : cl).push_back(PermCell{h_list[li].value, h_list[li].side_row & 0x7fffffffu});
      if (cl.size() + cr.size() != outside) return fail(SBN_ERR_HIP, "internal: the overflow list of pair %zu is incomplete", k0 + k);
      diff_cells(cl, cr, per_pair, s, out);
      P->permdiff_routes[1]++;
    }
    h_list.clear();
    times[2] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return SBN_OK;
}

extern "C" int sbn_prover_explain_permutation_times(const sbn_prover* P, float* ms, int cap) { return P ? copy_times(P->diag_ms[DIAG_PERMDIFF], 3, ms, cap) : 0; }
