/* The reference's call with the trace in host memory, from plain C: G1ExpStark(128), witness generated on the HOST
 * (sbn_generate_trace_g1_exp: 1,676 columns x 2^16 rows, 0.88 GB), then
 *   1. sbn_prover_prove_host_trace on a live prover: the trace crosses PCIe inside the trace commitment;
 *   2. the one-shot sbn_prove with its context cache on: the second call finds the device context of the first.
 *
 *   ./prove_host_trace ios.bin        ios.bin = 128 x 40 little-endian u32 (include/sbn.h)
 *
 * Prints the checksum of the proof (all three proofs must agree); exits non-zero on any failure. */
#include "sbn.h"
#include <stdio.h>
#include <stdlib.h>

static unsigned long long checksum(const sbn_proof* proof) {
  uint64_t sum = 0;
  const uint64_t* w = sbn_proof_words(proof);
  for (size_t i = 0; i < sbn_proof_num_words(proof); i++) sum = sum * 0x100000001b3ULL ^ w[i];
  return (unsigned long long)sum;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s ios.bin\n", argv[0]); return 2; }
  static uint32_t ios[128 * 40];
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(ios, sizeof ios, 1, f) != 1) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  fclose(f);
  if (sbn_abi_version() != SBN_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }
  sbn_air_desc air = {SBN_AIR_G1_EXP, 128};
  sbn_config cfg;
  sbn_standard_fast_config(&cfg);
  const size_t rows = (size_t)512 * 128, n_pi = sbn_air_num_public_inputs(&air);
  uint64_t* trace = malloc(sbn_air_num_columns(&air) * rows * sizeof *trace);
  uint64_t* pi = malloc(n_pi * sizeof *pi);
  if (!trace || !pi) { fprintf(stderr, "out of memory\n"); return 1; }
  int rc = sbn_generate_trace_g1_exp(ios, 128, trace, pi);         /* generate_trace + generate_public_inputs  exp.rs:816-817 */
  sbn_prover* prover = NULL;
  sbn_proof *proof = NULL, *one_shot[2] = {NULL, NULL};
  if (!rc) rc = sbn_prover_create(&air, &cfg, 16, &prover);
  if (!rc) rc = sbn_prover_prove_host_trace(prover, trace, pi, n_pi, &proof);   /* load + prove: prove::<F, C, _, D>(...)  exp.rs:818-825 */
  if (rc) { fprintf(stderr, "failed (%d): %s\n", rc, sbn_last_error()); return 1; }
  sbn_prover_destroy(prover);
  size_t bytes = sbn_proof_serialize(proof, NULL, 0);
  uint8_t* buf = malloc(bytes);
  sbn_proof_serialize(proof, buf, bytes);
  rc = sbn_verify(&air, &cfg, buf, bytes);                         /* verify_stark_proof(...)                  exp.rs:826 */
  if (rc) { fprintf(stderr, "verify failed (%d): %s\n", rc, sbn_last_error()); return 1; }

  uint64_t st[6];
  rc = sbn_prove_cache_configure((uint64_t)16 << 30);              /* keep up to 16 GB of device contexts between sbn_prove calls */
  for (int i = 0; i < 2 && !rc; i++) rc = sbn_prove(&air, &cfg, trace, 16, pi, n_pi, &one_shot[i]);
  if (!rc) rc = sbn_prove_cache_stats(st);
  if (rc) { fprintf(stderr, "one-shot failed (%d): %s\n", rc, sbn_last_error()); return 1; }
  if (checksum(one_shot[0]) != checksum(proof) || checksum(one_shot[1]) != checksum(proof)) { fprintf(stderr, "the one-shot proofs differ\n"); return 1; }
  if (st[0] != 1 || st[1] != 1 || st[3] != 1) { fprintf(stderr, "cache: %llu hits, %llu misses, %llu resident\n", (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[3]); return 1; }
  sbn_prove_cache_configure(0);                                    /* releases the cached context */

  printf("G1ExpStark(128) from a host trace: proof %zu words, checksum %016llx, verified; one-shot cache: %llu hit, %llu miss, %.2f GB context\n",
         sbn_proof_num_words(proof), checksum(proof), (unsigned long long)st[0], (unsigned long long)st[1], (double)st[4] / 1e9);
  sbn_proof_free(proof); sbn_proof_free(one_shot[0]); sbn_proof_free(one_shot[1]);
  free(buf); free(pi); free(trace);
  return 0;
}
