// Kernels of the permutation explain (perm_diff.hip; include/sbn.h sbn_prover_explain_permutations): the lhs column of a pair
// against its rhs column as multisets, by signed histograms in LDS.  Every value of a range-checked pair is below 2^16, so a
// pair is two workgroups, each owning half of [0, 2^16): 32,768 signed 32-bit bins = 128 KiB of the CU's 160 KiB (counts reach
// n <= 2^22: nothing narrower than 32 bits).  No histogram bin ever lives in global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pd {
typedef unsigned long long ull;
static constexpr int THREADS = 1024, WAVES = THREADS / 64;
static constexpr unsigned HALF_BINS = 32768;                       // values of one workgroup
static constexpr size_t HIST_LDS_BYTES = (size_t)HALF_BINS * 4;    // 128 KiB, the dynamic part; the reduction words are static
static constexpr unsigned BINS_PER_THREAD = HALF_BINS / THREADS;   // 32 consecutive bins: the scan is in value order
static constexpr unsigned DEV_CAP = 1024;                          // candidates of a pair the rows pass holds in LDS
static constexpr unsigned NO_ROW = 0xffffffffu;

struct Cols { int lhs, rhs; };
struct Cell { unsigned pair, side_row; ull value; };               // side_row = side << 31 | row (row < 2^22)
struct Entry { unsigned value, count_lhs, count_rhs, first_row_lhs, first_row_rhs; };
// per pair k of the launch: [differing values, excess lhs, excess rhs, out-of-range cells]
struct Params {
  const ull* trace; size_t n;
  const Cols* cols;            // [pairs]
  ull* stats;                  // [pairs][4], zeroed
  unsigned* half_count;        // [pairs][2]: differing values of each half (exact, not capped)
  unsigned* cand;              // [pairs][2][cap]: the smallest `cap` differing values of each half, ascending
  Entry* entries;              // [pairs][cap]
  ull* list_count;             // cells offered to the overflow list (may exceed list_cap), zeroed
  Cell* list; unsigned list_cap;
  unsigned cap;                // min(per_pair, DEV_CAP)
};

// One column into the bins of this half, 16 bytes a lane; sign = +1 / -1.  A cell >= 2^16 is no bin's: half 0 counts it (a wave
// ballot, one global atomic per wave that saw one) and appends it to the bounded list.  n is a power of two >= 512, so a wave is
// wholly inside or outside the column and the ballots are wave-uniform.
__device__ __forceinline__ void hist_column(const Params& p, int* bins, const ull* col, unsigned half, unsigned k, unsigned side, int sign) {
  const ulonglong2* c2 = reinterpret_cast<const ulonglong2*>(col);
  const size_t n2 = p.n >> 1;
  const unsigned lane = threadIdx.x & 63;
  for (size_t j = threadIdx.x; j < n2; j += THREADS) {
    const ulonglong2 w = c2[j];
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const ull v = e ? w.y : w.x;
      if (v < 65536) {
        if ((unsigned)(v >> 15) == half) atomicAdd(&bins[(unsigned)v & (HALF_BINS - 1)], sign);
      }
      const ull b = __ballot(half == 0 && v >= 65536);
      if (b) {
        const int leader = __ffsll((long long)b) - 1;
        ull at = 0;
        if ((int)lane == leader) {
          atomicAdd(&p.stats[(size_t)k * 4 + 3], (ull)__popcll(b));
          at = atomicAdd(p.list_count, (ull)__popcll(b));
        }
        at = __shfl(at, leader);
        if ((b >> lane) & 1) {
          const ull slot = at + (ull)__popcll(b & (((ull)1 << lane) - 1));
          if (slot < p.list_cap) p.list[slot] = Cell{k, (side << 31) | (unsigned)(2 * j + e), v};
        }
      }
    }
  }
}

// grid (2 halves, pairs), THREADS threads, HIST_LDS_BYTES of dynamic LDS
__global__ __launch_bounds__(THREADS) void perm_hist_kernel(Params p) {
  extern __shared__ int bins[];
  __shared__ unsigned wave_cnt[WAVES];
  __shared__ unsigned tot[2];   // excess lhs, excess rhs of this half
  const unsigned half = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (unsigned i = tid; i < HALF_BINS; i += THREADS) bins[i] = 0;
  if (tid < 2) tot[tid] = 0;
  __syncthreads();
  const Cols c = p.cols[k];
  hist_column(p, bins, p.trace + (size_t)c.lhs * p.n, half, k, 0, +1);
  hist_column(p, bins, p.trace + (size_t)c.rhs * p.n, half, k, 1, -1);
  __syncthreads();
  // thread t owns bins [32 t, 32 t + 32); read rotated by t so that a wave's lanes spread over the banks
  unsigned nz = 0, pos = 0, neg = 0;
  const unsigned b0 = tid * BINS_PER_THREAD;
  for (unsigned i = 0; i < BINS_PER_THREAD; i++) {
    const int d = bins[b0 + ((i + tid) & (BINS_PER_THREAD - 1))];
    nz += d != 0;
    if (d > 0) pos += (unsigned)d; else neg += (unsigned)(-d);
  }
  // exclusive prefix of nz over the workgroup: the slot of this thread's first differing value, in value order
  unsigned incl = nz;
  for (int s = 1; s < 64; s <<= 1) { const unsigned u = __shfl_up(incl, s); if ((int)lane >= s) incl += u; }
  for (int s = 32; s; s >>= 1) { pos += __shfl_xor(pos, s); neg += __shfl_xor(neg, s); }
  if (lane == 63) wave_cnt[wave] = incl;
  if (lane == 0 && (pos | neg)) { atomicAdd(&tot[0], pos); atomicAdd(&tot[1], neg); }
  __syncthreads();
  unsigned before = 0, all = 0;
  for (unsigned w = 0; w < WAVES; w++) { const unsigned cw = wave_cnt[w]; if (w < wave) before += cw; all += cw; }
  unsigned at = before + incl - nz;
  if (nz && at < p.cap) {
    unsigned* out = p.cand + ((size_t)k * 2 + half) * p.cap;
    for (unsigned i = 0; i < BINS_PER_THREAD && at < p.cap; i++)
      if (bins[b0 + i] != 0) out[at++] = (half << 15) | (b0 + i);
  }
  if (tid == 0) {
    p.half_count[(size_t)k * 2 + half] = all;
    if (all) { atomicAdd(&p.stats[(size_t)k * 4 + 0], (ull)all); atomicAdd(&p.stats[(size_t)k * 4 + 1], (ull)tot[0]); atomicAdd(&p.stats[(size_t)k * 4 + 2], (ull)tot[1]); }
  }
}

// Counts and first rows of the candidates in one column.  The bitmap answers "no candidate" for nearly every cell; a candidate
// is found by bisection in the sorted list.
__device__ __forceinline__ void rows_column(const ull* col, size_t n, const unsigned* bitmap, const unsigned* cval, unsigned m, unsigned* count, unsigned* first) {
  const ulonglong2* c2 = reinterpret_cast<const ulonglong2*>(col);
  const size_t n2 = n >> 1;
  for (size_t j = threadIdx.x; j < n2; j += THREADS) {
    const ulonglong2 w = c2[j];
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const ull v = e ? w.y : w.x;
      if (v >= 65536 || !((bitmap[(unsigned)v >> 5] >> ((unsigned)v & 31)) & 1)) continue;
      unsigned lo = 0, hi = m;                      // cval[lo] <= v < cval[hi]; v is in the list
      while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (cval[mid] <= (unsigned)v) lo = mid; else hi = mid; }
      atomicAdd(&count[lo], 1u);
      atomicMin(&first[lo], (unsigned)(2 * j + e));
    }
  }
}

// grid (pairs), THREADS threads; a workgroup whose pair has no differing value leaves at once
__global__ __launch_bounds__(THREADS) void perm_rows_kernel(Params p) {
  __shared__ unsigned bitmap[65536 / 32];
  __shared__ unsigned cval[DEV_CAP], cl[DEV_CAP], cr[DEV_CAP], fl[DEV_CAP], fr[DEV_CAP];
  const unsigned k = blockIdx.x, tid = threadIdx.x;
  const unsigned c0 = p.half_count[(size_t)k * 2], c1 = p.half_count[(size_t)k * 2 + 1];
  if (c0 + c1 == 0) return;
  // the halves merged: every value of half 0 is below every value of half 1; the first `cap` stay
  const unsigned m0 = c0 < p.cap ? c0 : p.cap, m1 = c1 < p.cap - m0 ? c1 : p.cap - m0, m = m0 + m1;
  for (unsigned i = tid; i < 65536 / 32; i += THREADS) bitmap[i] = 0;
  __syncthreads();
  for (unsigned i = tid; i < m; i += THREADS) {
    const unsigned v = i < m0 ? p.cand[((size_t)k * 2) * p.cap + i] : p.cand[((size_t)k * 2 + 1) * p.cap + (i - m0)];
    cval[i] = v; cl[i] = 0; cr[i] = 0; fl[i] = NO_ROW; fr[i] = NO_ROW;
    atomicOr(&bitmap[v >> 5], 1u << (v & 31));
  }
  __syncthreads();
  if (m == 0) return;
  const Cols c = p.cols[k];
  rows_column(p.trace + (size_t)c.lhs * p.n, p.n, bitmap, cval, m, cl, fl);
  rows_column(p.trace + (size_t)c.rhs * p.n, p.n, bitmap, cval, m, cr, fr);
  __syncthreads();
  for (unsigned i = tid; i < m; i += THREADS) p.entries[(size_t)k * p.cap + i] = Entry{cval[i], cl[i], cr[i], fl[i], fr[i]};
}
}  // namespace pd
