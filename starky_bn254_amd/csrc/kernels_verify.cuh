// HIP kernel of the batch verifier (gfx950), included once by verifier_device.hip.
//
// One work item = (proof, query, tree): the Merkle check of one opened leaf -- hash_or_noop of the leaf, the path of
// two_to_one nodes, the comparison with the cap entry -- and, for the initial oracles, the alpha-reduction of the opened row
// from the words the sponge absorbs anyway.  An item is a chain of dependent permutations (G1ExpStark(128): 210 leaf blocks and
// 13 path nodes for the trace oracle), so it runs on the 16-lane form of the permutation (poseidon_permute_coop16, as
// fri_leaf_hash_coop_kernel and merkle_level_coop_kernel do): lane j < 12 holds state[j], lanes 12..15 mirror lanes 0..3.
// Every lane of a row executes every permutation (DPP broadcasts): an item beyond the batch is masked at its loads and stores
// and never returns early.  blockIdx.y = tree, so the 16 items of a workgroup share their trip counts.
//
// All proofs of one (table, config, degree_bits) share one layout (verifier_core.hpp VerifyLayout): the kernel reads a proof
// only at offsets the host computed from it, inside a slot whose length the host checked, and only canonical words (the host
// parse rejects anything else before a proof is uploaded).
#pragma once
#include "poseidon.cuh"

struct VerifyTreeDev { u32 leaf_off, leaf_len, nsib, cap_off, shift, initial; };
struct VerifyKernelParams {
  const u64* proofs;      // [nproofs][proof_words]
  const u32* indices;     // [nproofs][nqueries]
  const u64* alpha;       // [nproofs][4]: alpha (c0, c1), alpha^8 (c0, c1)
  const VerifyTreeDev* trees;
  unsigned char* ok;      // [nproofs][nqueries][ntrees]: 1 = the Merkle path verifies
  u64* psum;              // [nproofs][nqueries][ninit][2]: P_t of the opened row
  u64 proof_words, query_off, query_stride;
  u32 nproofs, nqueries, ntrees, ninit, lde_bits, cap_mask;
};

__global__ __launch_bounds__(256) void verify_items_kernel(VerifyKernelParams p) {
  const u32 lane64 = threadIdx.x & 63, lane = threadIdx.x & 15, e = lane < 12 ? lane : lane - 12;
  const u32 tree = blockIdx.y;
  const VerifyTreeDev td = p.trees[tree];
  const u64 item = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 4, nitems = (u64)p.nproofs * p.nqueries;
  const bool valid = item < nitems;
  const u32 a = valid ? (u32)(item / p.nqueries) : 0, q = valid ? (u32)(item % p.nqueries) : 0;
  const u64* leaf = p.proofs + (u64)a * p.proof_words + p.query_off + (u64)q * p.query_stride + td.leaf_off;
  const u64* sib = leaf + td.leaf_len;
  u32 index = valid ? ((p.indices[(u64)a * p.nqueries + q] & ((1u << p.lde_bits) - 1u)) >> td.shift) : 0;

  // leaf digest (hash_or_noop, overwrite-mode sponge) and, for an initial oracle, lane j < 8: sum_k v[8k + j] (alpha^8)^k
  const bool reduce = td.initial != 0;
  E2 a8, pw(F(1), F(0)), acc(F(0), F(0));
  if (reduce && valid) a8 = E2(F(p.alpha[(u64)a * 4 + 2]), F(p.alpha[(u64)a * 4 + 3]));
  const bool hashed = td.leaf_len > 4;   // uniform over the workgroup
  u64 st = 0;
  for (u32 c = 0; c < td.leaf_len; c += 8) {
    const bool in = valid && e < 8 && c + e < td.leaf_len;
    const u64 v = in ? leaf[c + e] : 0;
    if (in) st = v;   // a partial last block overwrites only its own elements
    if (reduce) { acc = acc + pw * F(v); pw = pw * a8; }
    if (hashed) st = poseidon_permute_coop16(st, lane);
  }
  if (reduce) {
    // combine the eight lanes with alpha^j; lanes 8..15 carry zero sums
    E2 al(F(0), F(0));
    if (valid) al = E2(F(p.alpha[(u64)a * 4]), F(p.alpha[(u64)a * 4 + 1]));
    E2 t = lane < 8 ? acc * e2_pow(al, lane) : E2(F(0), F(0));
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
      const u64 oa = __shfl_xor((unsigned long long)t.a.v, m, 16), ob = __shfl_xor((unsigned long long)t.b.v, m, 16);
      t = t + E2(F(oa), F(ob));
    }
    if (valid && lane == 0) {
      u64* out = p.psum + ((item * p.ninit) + tree) * 2;
      out[0] = t.a.v; out[1] = t.b.v;
    }
  }
  // the path: the digest sits in lanes 0..3 (and their mirrors); node = two_to_one(left, right), the side by the index bit
  for (u32 s = 0; s < td.nsib; s++) {
    const u64 cur = __shfl((unsigned long long)st, lane & 3, 16);   // every lane: digest word e & 3
    const u64 sw = (valid && e < 8) ? sib[4 * s + (e & 3)] : 0;
    const bool right = (index >> s) & 1;                           // the running digest is the right child
    const u64 v = e < 4 ? (right ? sw : cur) : (e < 8 ? (right ? cur : sw) : 0);
    st = poseidon_permute_coop16(v, lane);
  }
  const u32 ci = (index >> td.nsib) & p.cap_mask;
  const bool eq = !(valid && lane < 4) || st == p.proofs[(u64)a * p.proof_words + td.cap_off + 4 * ci + lane];
  const u64 b = __ballot(eq);
  const bool all = ((b >> (lane64 & 48)) & 0xFFFFu) == 0xFFFFu;
  if (valid && lane == 0) p.ok[item * p.ntrees + tree] = all ? 1 : 0;
}
