/*
 * sbn.h -- C ABI of the MI355X-native Starky/BN254 prover path (libsbn254.so).
 *
 * Drop-in boundary for the reference's prove()/verify_stark_proof() calls on the G1 / G2 / Fq12 tables:
 *   reference call sites   src/curves/g1/exp.rs:811-826      (G1ExpStark: trace, pi, prove, verify)
 *                          src/curves/g1/muladd.rs:666-678   (G1Stark)
 *                          src/curves/g1/circuit.rs:187-201  (G1ExpStarkyProofGenerator::run_once)
 *   reference signatures   starky 0.1.1 `prove::<F,C,S,D>(stark, &config, trace_poly_values,
 *                          public_inputs, &mut timing)` and `verify_stark_proof(stark, proof, &config)`
 *                          (un-vendored dependency, Cargo.toml:21).
 *
 * Because the AIR's `eval_packed_generic` is generic Rust that cannot cross a C ABI, a table is
 * named by (kind, num_io) and its constraint code lives natively behind this boundary.
 *
 * Conventions: plain pointers and sizes, no exceptions; 0 = success, negative = sbn_status error.
 * All field elements are canonical Goldilocks u64 (< 2^64 - 2^32 + 1), little-endian.
 * Trace wire format = the reference's Vec<PolynomialValues<F>>: COLUMN-MAJOR [num_columns][N]
 * (src/curves/g1/exp.rs:314-317).  Public inputs: flat [num_public_inputs] (exp.rs:320-327).
 *
 * Proof byte layout ("canonical proof words", LE u64 each; the reference never serialises a proof,
 * so this layout is defined here and shared with the test oracle):
 *   header[12] = { magic "SNBPROV1", degree_bits, n_trace_cols, n_perm_zs, n_quotient_polys,
 *                  n_public_inputs, cap_height, rate_bits, n_fri_layers, arity_bits,
 *                  final_poly_len, n_queries }
 *   trace_cap[2^cap_height][4], permutation_zs_cap[..][4] (iff n_perm_zs>0), quotient_polys_cap[..][4]
 *   openings: local_values[n_trace_cols][2], next_values[..][2], permutation_zs[n_perm_zs][2],
 *             permutation_zs_next[..][2], quotient_polys[n_quotient_polys][2]     (ext elem = c0,c1)
 *   fri commit_phase_merkle_caps[n_fri_layers][2^cap_height][4]
 *   per query (n_queries): per initial oracle (trace, [perm_zs], quotient): leaf row values, then
 *             siblings[lde_bits-cap_height][4]; per FRI layer: evals[2^arity_bits][2], siblings[..][4]
 *   final_poly[final_poly_len][2], pow_witness, public_inputs[n_public_inputs]
 */
#ifndef SBN_H
#define SBN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sbn_status {
  SBN_OK = 0,
  SBN_ERR_BAD_ARG = -1,       /* null pointer, unknown air kind, size mismatch */
  SBN_ERR_NON_CANONICAL = -2, /* a field element >= p was supplied */
  SBN_ERR_NO_DEVICE = -3,     /* no HIP device / HIP runtime failure at init */
  SBN_ERR_HIP = -4,           /* a HIP call failed (message via sbn_last_error) */
  SBN_ERR_MALFORMED_PROOF = -5,
  SBN_ERR_VERIFY_FAILED = -6, /* proof rejected (reason via sbn_last_error) */
  SBN_ERR_UNSUPPORTED = -7,   /* e.g. G1_EXP with fewer than 2^16 rows (range_check.rs:26) */
  SBN_ERR_WITNESS = -8        /* trace generation hit a degenerate case (x1==x2 in an affine add) */
} sbn_status;

/* Table kinds.  G1_OP = reference `G1Stark` (src/curves/g1/muladd.rs:462-624);
 * G1_EXP = reference `G1ExpStark` (src/curves/g1/exp.rs:232-742). */
typedef enum sbn_air_kind { SBN_AIR_G1_OP = 1, SBN_AIR_G1_EXP = 2, SBN_AIR_G2_EXP = 3, SBN_AIR_FQ12_EXP = 4, SBN_AIR_FQ_EXP = 5, SBN_AIR_FQ12_EXP_U64 = 6,
                              SBN_AIR_MODULAR = 7, SBN_AIR_FQ12_MUL = 8, SBN_AIR_LOOKUP = 9, SBN_AIR_FLAGS = 10, SBN_AIR_FLAGS_U64 = 11 } sbn_air_kind;
/* G2_EXP = reference `G2ExpStark` (src/curves/g2/exp.rs:248-807): the same machine over Fq2 coordinates.
 * FQ12_EXP = reference `Fq12ExpStark` (src/fields/fq12/exp.rs:223-605): offset * x^e in Fq12 (flat basis of
 * plonky2-bn254 `MyFq12`: coefficient of w^k is c[k] + c[k+6]*i, w^6 = 9 + i), 512 rows per instance, num_io a
 * power of two between 1 and 512.
 * FQ_EXP = reference `FqExpStark` (src/fields/fq/exp.rs:193-582): offset * x^e in the base field Fq, the same
 * square-and-multiply machine over one coefficient (960 columns at num_io = 128), u32 public inputs, u16 range check.
 * FQ12_EXP_U64 = reference `Fq12ExpU64Stark` (src/fields/fq12_u64/exp_u64.rs:243-571): Fq12 exponentiation by a u64
 * exponent, 128 rows per instance, 6-column flags (flags_u64.rs), the exponent is ONE public input (< p).
 * MODULAR = reference `ModularStark` (src/modular/modular.rs:361-537) and FQ12_MUL = reference `Fq12Stark`
 * (src/fields/fq12/mul.rs:355-517): its single-operation test tables for the modular gadget (a * b mod p per row, 812
 * columns) and the Fq12 product (9722 columns); no public inputs, num_io ignored, any power-of-two height >= 256.
 * LOOKUP = reference `MyStark` (src/utils/lookup.rs:136-213), its unit-test table of the lookup argument: 4 columns (inputs,
 * table, permuted inputs, permuted table), two permutation pairs, Merkle leaves are the rows themselves (hash_or_noop); any
 * power-of-two height >= 512, num_io ignored (the reference's own 8-row instance is below the device prover's minimum).
 * FLAGS = reference `FlagStark` (src/utils/flags.rs:379-547), the unit-test table of the exponent-bit flags: num_io inputs
 * of 8 u32 limbs, 512 rows each (the reference uses 16), 17 + 4 * num_io columns, NO permutation pairs -- the one table
 * whose proof carries no permutation-Z commitment (header n_perm_zs = 0).
 * FLAGS_U64 = the `FlagStark` of src/fields/fq12_u64/flags_u64.rs:289-420, the same for the u64-exponent flags: num_io inputs
 * (u64), 128 rows each, 7 + 4 * num_io columns, no rotation pulse, no permutation pairs; num_io >= 4 (512 rows). */

typedef struct sbn_air_desc {
  int32_t kind;    /* sbn_air_kind */
  uint32_t num_io; /* Exp tables: number of instances (rows = 512*num_io; FQ12_EXP_U64: 128*num_io); G1_OP: ignored */
} sbn_air_desc;

/* Mirrors starky `StarkConfig` + plonky2 `FriConfig` (reference: stark.config() ->
 * StarkConfig::standard_fast_config, src/curves/g1/exp.rs:250-253). */
typedef struct sbn_config {
  uint32_t security_bits;      /* 100 */
  uint32_t num_challenges;     /* 2   */
  uint32_t rate_bits;          /* 1   */
  uint32_t cap_height;         /* 4   */
  uint32_t proof_of_work_bits; /* 16  */
  uint32_t fri_arity_bits;     /* 4   (FriReductionStrategy::ConstantArityBits(4, 5)) */
  uint32_t fri_final_poly_bits;/* 5   */
  uint32_t num_query_rounds;   /* 84  */
  /* Not a StarkConfig field: which plonky2 FRI this library speaks (sbn_fri_variant).  SBN_FRI_TIMES_X = the 0.1.x line
   * the reference pins (plonky2 0.1.3 @ 541e127, Cargo.lock:529-531): fri/oracle.rs `prove_openings` multiplies the final
   * polynomial by X (`final_poly.coeffs.insert(0, ZERO)`, mir-protocol/plonky2 PR #436) and fri/verifier.rs
   * `fri_combine_initial` returns `sum * subgroup_x`.  SBN_FRI_PLAIN = the form without that step (the quotients are
   * zero-padded at the end), kept selectable.  0 = SBN_FRI_DEFAULT (= SBN_FRI_TIMES_X), so a zero-initialised field
   * selects the default and not the other protocol.  The dependency is un-vendored, so the default is recalled
   * ([DEP-RECALL]); both forms are tested. */
  uint32_t fri_variant;
} sbn_config;
typedef enum sbn_fri_variant { SBN_FRI_DEFAULT = 0, SBN_FRI_TIMES_X = 1, SBN_FRI_PLAIN = 2 } sbn_fri_variant;

typedef struct sbn_prover sbn_prover; /* device context: buffers sized for one (air, degree_bits) */
typedef struct sbn_proof sbn_proof;   /* host-side proof object (canonical words) */

/* Library / device ------------------------------------------------------------------------------ */
const char* sbn_version(void);
/* Bumped whenever a struct or a function signature of this header changes (3: sbn_config.fri_variant replaces
 * fri_final_poly_times_x, sbn_comm carries struct_size and stream-ordered callbacks; 4: sbn_set_thread_device,
 * sbn_prover_describe, sbn_set_device also selects HIP's current device).  Callers compare with SBN_ABI_VERSION. */
#define SBN_ABI_VERSION 4
int sbn_abi_version(void);
const char* sbn_last_error(void);                    /* thread-local message of the last failure */
int sbn_device_count(void);
/* Device of the provers and transports the calling thread creates afterwards, and the default of threads that never chose one.
 * Also makes it HIP's current device of the calling thread (hipSetDevice), so sbn_set_device(r) followed by
 * sbn_rccl_comm_create puts the staging buffers, the communicator and the prover of rank r on GPU r. */
int sbn_set_device(int device);
/* The same for the calling thread ONLY (the process default stays): for rank threads of one process (sbn_local_comm_create). */
int sbn_set_thread_device(int device);
void sbn_standard_fast_config(sbn_config* out);      /* StarkConfig::standard_fast_config */
/* sbn_standard_fast_config with another blowup at the same conjectured security (rate_bits * num_query_rounds + proof_of_work_bits
 * >= security_bits): rate_bits set and num_query_rounds = ceil((security_bits - proof_of_work_bits) / rate_bits), i.e. 84 / 42 / 28
 * queries at rate_bits 1 / 2 / 3.  rate_bits 3 with 28 queries are the FRI parameters of plonky2's standard_recursion_config: a proof a
 * third the size for a recursive verifier, for four times the LDE rows to hash.  rate_bits = 0 is taken as 1.  The helper only fills
 * the struct: which values the provers and verifiers accept is stated at sbn_prover_create. */
void sbn_config_for_rate(uint32_t rate_bits, sbn_config* out);

/* Table shape (ExpStarkConstants, src/curves/g1/exp.rs:6-34) ----------------------------------- */
size_t sbn_air_num_columns(const sbn_air_desc* air);
size_t sbn_air_num_public_inputs(const sbn_air_desc* air);
size_t sbn_air_num_permutation_zs(const sbn_air_desc* air, const sbn_config* cfg);
size_t sbn_air_num_constraints(const sbn_air_desc* air); /* AIR constraints per point (no perm checks) */

/* Witness generation (host): replaces G1ExpStark::generate_trace / generate_public_inputs
 * (src/curves/g1/exp.rs:290-327) and G1Stark::generate_trace (muladd.rs:481-546).
 * ios: num_io x 40 u32 = x.x[8] x.y[8] offset.x[8] offset.y[8] exp_val[8]  (u32 limbs, LE).
 * trace_out: column-major [num_columns][512*num_io]; pi_out: [56*num_io]. */
int sbn_generate_trace_g1_exp(const uint32_t* ios, size_t num_io, uint64_t* trace_out, uint64_t* pi_out);
/* G2ExpStark::generate_trace / generate_public_inputs (src/curves/g2/exp.rs:307-342).
 * ios: num_io x 72 u32 = x.x.c0 x.x.c1 x.y.c0 x.y.c1 offset.x.c0 offset.x.c1 offset.y.c0 offset.y.c1 exp_val
 * (8 u32 limbs each); trace_out: [num_columns][512*num_io]; pi_out: [104*num_io]. */
int sbn_generate_trace_g2_exp(const uint32_t* ios, size_t num_io, uint64_t* trace_out, uint64_t* pi_out);
/* Fq12ExpStark::generate_trace / generate_public_inputs (src/fields/fq12/exp.rs:283-319).
 * ios: num_io x 200 u32 = x[12] offset[12] (flat-basis coefficients, 8 u32 limbs each) exp_val[8];
 * trace_out: [num_columns][512*num_io]; pi_out: [584*num_io]. */
int sbn_generate_trace_fq12_exp(const uint32_t* ios, size_t num_io, uint64_t* trace_out, uint64_t* pi_out);
/* Fq12ExpU64Stark::generate_trace / generate_public_inputs (src/fields/fq12_u64/exp_u64.rs:283-313).
 * ios: num_io x 194 u32 = x[12] offset[12] (8 u32 limbs each) exp_val (low, high u32; value < 2^64 - 2^32 + 1);
 * trace_out: [num_columns][128*num_io]; pi_out: [577*num_io]. */
int sbn_generate_trace_fq12_exp_u64(const uint32_t* ios, size_t num_io, uint64_t* trace_out, uint64_t* pi_out);
/* FqExpStark::generate_trace / generate_public_inputs (src/fields/fq/exp.rs:248-284).
 * ios: num_io x 24 u32 = x[8] offset[8] exp_val[8]; trace_out: [num_columns][512*num_io]; pi_out: [32*num_io]. */
int sbn_generate_trace_fq_exp(const uint32_t* ios, size_t num_io, uint64_t* trace_out, uint64_t* pi_out);
/* pts: rows x 32 u32 = a.x[8] a.y[8] b.x[8] b.y[8]; trace_out: [num_columns][rows]. */
int sbn_generate_trace_g1_op(const uint32_t* pts, size_t rows, uint64_t* trace_out);
/* ModularStark::generate_trace (modular.rs:383-437) with the operands given: ops: rows x 16 u32 = a[8] b[8] (both < p). */
int sbn_generate_trace_modular(const uint32_t* ops, size_t rows, uint64_t* trace_out);
/* Fq12Stark::generate_trace (fq12/mul.rs:375-419): ops: rows x 192 u32 = x[12] y[12] (flat-basis coefficients < p, 8 u32 limbs each). */
int sbn_generate_trace_fq12_mul(const uint32_t* ops, size_t rows, uint64_t* trace_out);

/* MyStark::generate_trace (lookup.rs:151-166) on caller-given columns: inputs[rows], table[rows] (canonical field elements;
 * every input value must occur in the table) -> [4][rows] = inputs, table, permuted inputs, permuted table (permuted_cols,
 * lookup.rs:60-111). */
int sbn_generate_trace_lookup(const uint64_t* inputs, const uint64_t* table, size_t rows, uint64_t* trace_out);
/* FlagStark::generate_trace (flags.rs:392-440): limbs: num_io x 8 u32; trace_out: [17 + 4 * num_io][512 * num_io]. */
int sbn_generate_trace_flags(const uint32_t* limbs, size_t num_io, uint64_t* trace_out);
/* flags_u64.rs FlagStark::generate_trace (:316-337): exps: num_io x u64; trace_out: [7 + 4 * num_io][128 * num_io]. */
int sbn_generate_trace_flags_u64(const uint64_t* exps, size_t num_io, uint64_t* trace_out);

/* Prover ---------------------------------------------------------------------------------------- */
/* Accepted (anything else: SBN_ERR_UNSUPPORTED, checked before a device is looked for): num_challenges = 2, rate_bits 1 or 3
 * (2 is refused: the transforms and the Merkle kernels run at it through sbn_commit_values only), cap_height 1..8, fri_arity_bits
 * 1..4, num_query_rounds 1..512, proof_of_work_bits 0..32, any fri_final_poly_bits, fri_variant 0..2; degree_bits >= 9 with
 * degree_bits + rate_bits <= 23, the largest LDE being 2^23 points: 9..22 at rate_bits 1, 9..20 at rate_bits 3 (the Exp tables: the
 * height their num_io fixes, G1 / G2 / FQ_EXP from 2^16 rows).  sbn_verifier_create accepts the same range.  Every value of
 * that range is proved on the device and compared word for word with the CPU oracle under the same config
 * (tests/test_config_matrix_gpu.py at rate_bits 1: each field at both ends of its range except 32 proof-of-work bits, LookupStark
 * at every height up to 2^22 rows; tests/test_rate_gpu.py at rate_bits 3).  At rate_bits r the quotient is evaluated on the coset of
 * 2n points, every 2^(r-1)-th row of the LDE, as starky does (the section on rate_bits).  fri_arity_bits = 1: a FRI leaf is two extension values = four words, which is its own digest
 * (plonky2 hash_or_noop), as the rows of a matrix of at most four columns are. */
int sbn_prover_create(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, sbn_prover** out);
/* How a context stores the coset LDEs of its trace and Z matrices between the commitment and the queries.
 * SBN_LDE_FULL: whole, [cols][n << rate_bits] each (what sbn_prover_create does).
 * SBN_LDE_COMPACT (rate_bits > 1): a matrix of more than 4 columns keeps only the rows the quotient reads, [cols][2n]; the LDE of a
 * column chunk lives in a small ring between its transform and the leaf sponge, and the rows a query opens are evaluated again
 * from the coefficients.  Same proof words; device memory per wide column falls from (2 + 2^rate_bits) n to 4 n words.  Matrices of
 * at most 4 columns (their rows are their own digests) stay whole in both modes. */
enum { SBN_LDE_FULL = 0, SBN_LDE_COMPACT = 1 };
typedef struct sbn_prover_options { uint32_t struct_size; uint32_t lde_storage; } sbn_prover_options;
/* sbn_prover_create with options; opt == NULL or lde_storage = SBN_LDE_FULL is exactly sbn_prover_create.  Checked before a device
 * is looked for, in this order: struct_size != sizeof the struct or an unknown lde_storage: SBN_ERR_BAD_ARG; then the refusals of
 * sbn_prover_create, and SBN_LDE_COMPACT with rate_bits 1: SBN_ERR_UNSUPPORTED (the quotient's domain is the whole LDE there,
 * qn = m, so nothing would be dropped), and SBN_LDE_COMPACT for a table with more than 4 trace columns and 1..4 Z columns (no
 * table has that shape; its quotient would need two row strides): SBN_ERR_UNSUPPORTED.  sbn_prover_describe reports
 * lde=full|compact, the ring depth and its bytes.
 * Known defect, in both storage modes and older than this option: a batch prover with three contexts in
 * flight has returned wrong proofs for units after a context's first; one and two contexts in flight have not.  A guarded batch
 * prover (sbn_batch_prover_set_guard) turns that defect from a wrong result with status 0 into SBN_ERR_VERIFY_FAILED naming the unit. */
int sbn_prover_create_with(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, const sbn_prover_options* opt, sbn_prover** out);
/* Device bytes sbn_prover_create_with allocates at creation (dev_bytes of sbn_prover_describe right after it), computed without a
 * device from the list of buffers the creation itself allocates from; the same argument checks.  Outside the plan, allocated by
 * the first call that needs them: 8 bytes of device memory for the canonical-form scan of sbn_prover_prove_host_trace (its upload
 * ring is pinned host memory, 64 MiB).  The row-major loads (sbn_prover_load_trace_rows) share that ring and allocate nothing more:
 * their device staging is carved from the LDE buffer, which is in the plan. */
int sbn_prover_memory_plan(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, const sbn_prover_options* opt, uint64_t* bytes_out);
void sbn_prover_destroy(sbn_prover* p);
/* Host -> device copy of the trace (PCIe-inclusive path). */
int sbn_prover_load_trace(sbn_prover* p, const uint64_t* trace_col_major, const uint64_t* public_inputs, size_t n_pi);
/* Trace already resident in HBM (device pointer, same layout); copied device-to-device. */
int sbn_prover_load_trace_device(sbn_prover* p, const uint64_t* d_trace_col_major, const uint64_t* public_inputs, size_t n_pi);
/* prove() on the loaded trace; may be called repeatedly (the loaded trace is preserved). */
int sbn_prover_prove(sbn_prover* p, sbn_proof** out);
/* load + prove in one call: the trace crosses PCIe in the commit pipeline's own column chunks while earlier chunks are
 * transformed and absorbed.  Same proof words as sbn_prover_load_trace followed by sbn_prover_prove.  On success the
 * trace is resident as after load_trace (prove can be repeated, read_trace returns it).  On any failure NO trace is
 * loaded.  The caller's matrix is only read (it may be a read-only mapping) and is not needed after the call returns; it
 * is staged through at most 64 MiB of pinned host memory per prover, allocated on the first call.  The canonical-form
 * check runs on the device, chunk by chunk behind the copies: a word >= p gives SBN_ERR_NON_CANONICAL naming the smallest
 * such index, as load_trace does, after the trace commitment instead of in front of it.  Single-GPU provers only; the
 * trace_commit stage time includes the upload. */
int sbn_prover_prove_host_trace(sbn_prover* p, const uint64_t* trace_col_major, const uint64_t* public_inputs, size_t n_pi, sbn_proof** out);
/* The same for a trace held as one allocation per column, the reference's `Vec<PolynomialValues<F>>` (prove(stark, &config, trace,
 * ...), src/curves/g1/circuit.rs:187-201): column c of the trace is columns[c][0 .. n), n = 2^degree_bits.  No flat copy is made:
 * the upload gathers from the columns into its pinned ring (csrc/host_columns.hpp).  The columns need 8-byte alignment only, two
 * entries may be the same pointer, and the memory is only read.
 * flags = 0: exactly the call above on the flattened matrix -- same proof words, same refusal, same message ("trace word %zu is
 * not canonical" with the index c * n + row, smallest first).
 * flags = SBN_TRACE_REDUCE: the words may be any 64-bit representatives.  A trace word >= p becomes w - p on the device, behind the
 * upload, where the scan would have run (csrc/kernels_load.cuh reduce_words_kernel; one subtraction suffices, 2^64 - 1 - p < p), and
 * public inputs >= p are reduced on the host.  *reduced_out (optional) receives the number of trace words changed (0 without the
 * flag).  Afterwards the trace is resident in canonical form: read_trace returns the reduced words.
 * Refused before any device work, in this order: p or out null, n_columns other than the table's column count, columns[c] null or
 * not 8-byte aligned (the message names c), an unknown flag bit (all SBN_ERR_BAD_ARG), the public-input checks of the call above,
 * a split prover (SBN_ERR_UNSUPPORTED).  A failing call leaves no trace loaded, the streams idle and the ring free. */
#define SBN_TRACE_REDUCE 1u   /* flags bit 0: a word >= p is taken mod p on the device instead of refused */
int sbn_prover_prove_host_columns(sbn_prover* p, const uint64_t* const* columns, size_t n_columns, uint32_t flags,
                                  const uint64_t* public_inputs, size_t n_pi, uint64_t* reduced_out, sbn_proof** out);
/* ROW-major traces: what the reference's generators hold in front of their `transpose` (src/curves/g1/exp.rs:255-298 and the other
 * generate_trace functions build `rows` row by row, transpose, and only then append the derived columns).  The library transposes
 * on the device (csrc/kernels_load.cuh) and, in main-row mode, writes the derived columns itself.
 * Exactly one of flat / row_ptrs is set: flat = one allocation, row r at flat[r * row_stride .. + n_cols), row_stride >= n_cols
 * (`Vec<[F; N]>`: row_stride = N); row_ptrs = one allocation per row, row_ptrs[r][0 .. n_cols) (`Vec<Vec<F>>`; row_stride is
 * ignored).  8-byte alignment suffices; the memory is only read, and the words between n_cols and row_stride are never read.
 * n_rows = 2^degree_bits.  n_cols selects the mode:
 *   whole-row mode, n_cols = the table's column count, any table: the call transposes and checks, nothing else; the shape-constant
 *     columns are compared as after sbn_prover_load_trace.
 *   main-row mode, n_cols = sbn_air_num_main_columns, the five Exp tables: the rows hold the main columns only, and the columns
 *     [num_main, num_columns) -- periodic pulse, io pulses, table column, range-check columns -- are written by the kernels of the
 *     device witness (host twin: by the code the host generators end with).  G1_EXP / G2_EXP / FQ_EXP on the device: 2^16 .. 2^20
 *     rows, as sbn_prover_generate_trace: every height these tables have (num_io <= 2,048).  FQ12_EXP,
 *     FQ12_EXP_U64: any size.
 * flags: 0 or SBN_TRACE_REDUCE, as for sbn_prover_prove_host_columns (words and public inputs >= p are taken mod p; *reduced_out,
 * optional, receives the number of trace words changed).
 * Refused in this order, before any device work where a device is involved:
 *   1. a null argument or struct_size != sizeof the struct; 2. both or neither of flat / row_ptrs; 3. n_rows != 2^degree_bits (the
 *   calls without a prover: no power of two, or not the height the table's num_io fixes); 4. n_cols neither of the two counts, or
 *   row_stride < n_cols; 5. flat or a row pointer null or not 8-byte aligned (the message names the row); 6. an unknown flag bit
 *   -- all SBN_ERR_BAD_ARG; 7. the public-input checks of sbn_prover_load_trace; 8. main-row mode on a table or height it does not
 *   cover (the main-column count of another table included): SBN_ERR_UNSUPPORTED; 9. a split prover: SBN_ERR_UNSUPPORTED.
 * Data errors are found on the device, inside the transposition: a word >= p without the reduce flag gives SBN_ERR_NON_CANONICAL,
 * "... row r, column c ..." being the first such word in row-major order; in main-row mode a word >= 2^16 (after the reduction)
 * in a range-checked main column gives SBN_ERR_WITNESS, named the same way.  A failing call leaves NO trace loaded, the streams
 * idle and the ring free. */
typedef struct sbn_host_rows {
  uint32_t struct_size, reserved;
  const uint64_t* flat; size_t row_stride;
  const uint64_t* const* row_ptrs;
  size_t n_rows, n_cols;
} sbn_host_rows;
/* Columns of a row in front of the reference's `transpose`: G1_EXP 398, G2_EXP 782, FQ_EXP 158, FQ12_EXP 1742, FQ12_EXP_U64 1734
 * (num_io does not enter); 0 for a table that is no Exp table. */
size_t sbn_air_num_main_columns(const sbn_air_desc* air);
/* Both modes on the host pool (SBN_HOST_THREADS), no device: trace_col_major_out[num_columns][n_rows] is the trace a prover would
 * hold after sbn_prover_load_trace_rows.  The no-GPU fallback and the CPU-testable twin.  There are no public inputs here, so refusal
 * 7 does not apply; main-row mode of the u16 tables takes any height from 2^16 rows. */
int sbn_trace_from_rows_host(const sbn_air_desc* air, const sbn_host_rows* rows, uint32_t flags, uint64_t* trace_col_major_out, uint64_t* reduced_out);
/* Rows in host memory -> the prover's trace buffer: pieces of whole rows cross PCIe through the pinned ring and the copy stream of
 * sbn_prover_prove_host_trace, packed to n_cols words per row, and piece k + 1 is copied and sent while piece k is transposed.
 * Afterwards the prover is loaded exactly as after sbn_prover_load_trace: sbn_prover_read_trace returns the full column-major
 * trace, sbn_prover_prove, sbn_prover_check_trace and sbn_prover_explain_rows work.  The staging of the pieces in flight and the
 * scratch of the derived columns are carved from the context's LDE buffer (resident transforms of the shape-constant columns are
 * dropped when the carving reaches them), so the call allocates no device memory beyond the 8 bytes and the pinned ring named at
 * sbn_prover_memory_plan. */
int sbn_prover_load_trace_rows(sbn_prover* p, const sbn_host_rows* rows, uint32_t flags, const uint64_t* public_inputs, size_t n_pi, uint64_t* reduced_out);
/* The same for rows already in HBM (a caller's own row-generating kernel): row r at d_rows + r * row_stride, 2^degree_bits rows.
 * The same transposition kernel, no PCIe traffic.  d_rows must not overlap the prover's buffers. */
int sbn_prover_load_trace_rows_device(sbn_prover* p, const uint64_t* d_rows, size_t row_stride, size_t n_cols, uint32_t flags,
                                      const uint64_t* public_inputs, size_t n_pi, uint64_t* reduced_out);
/* sbn_prover_load_trace_rows followed by sbn_prover_prove in one call (the commitment cannot start before the last row is in, so
 * this is load, then the ordinary proof, not the streaming commitment of sbn_prover_prove_host_trace). */
int sbn_prover_prove_host_rows(sbn_prover* p, const sbn_host_rows* rows, uint32_t flags, const uint64_t* public_inputs, size_t n_pi,
                               uint64_t* reduced_out, sbn_proof** out);
/* Per-stage device times (ms, HIP events on the prover's stream) of the last prove():
 * names via sbn_prover_stage_name(i); returns the number of stages written. */
int sbn_prover_stage_times(const sbn_prover* p, float* ms_out, int cap);
const char* sbn_prover_stage_name(int i);
/* Parity hook: the two Jacobian curve chains of every G1ExpStark (E = 1) / G2ExpStark (E = 2) instance as the device witness
 * generator consumes them ([num_io][257][3][E][4] u64 each, Montgomery form; csrc/bn254w.cuh exp_chains).  form 0 = the library's
 * choice (eight instances per AVX-512 IFMA register when the CPU has it), 1 = one instance at a time, 2 = IFMA or
 * SBN_ERR_UNSUPPORTED.  The forms write the same words. */
int sbn_host_curve_chains(int E, const uint32_t* ios, size_t num_io, uint64_t* ja_out, uint64_t* jb_out, int form);
/* The SBN_* environment switches this prover was created under, resolved, as one line of key=value pairs (csrc/settings.hpp:
 * the environment is read once, at creation; experiment switches need SBN_EXPERIMENTAL=1 and are listed under ignored=[...]
 * otherwise; a value that is not understood makes sbn_prover_create fail with SBN_ERR_BAD_ARG). */
int sbn_prover_describe(const sbn_prover* p, char* out, size_t cap);
/* The same check without a prover or a device: SBN_OK and the resolved switches of the calling process, or SBN_ERR_BAD_ARG. */
int sbn_settings_check(char* out, size_t cap);
/* Raw device pointer of the loaded trace buffer (for callers that fill it on-device).  Words written through it count from the
 * next sbn_prover_load_trace_device on this pointer: prove() may reuse what it derived from the trace it was last told about. */
uint64_t* sbn_prover_trace_device_ptr(sbn_prover* p);
/* The shape-constant columns [*first_out, *end_out) of a table: functions of the row, the height and num_io alone (the Exp tables'
 * periodic pulse, io-pulse counter, io-pulse witness / pulse pairs and range-check table column; 0, 0 for every other table).  A
 * single-GPU prover with whole LDEs keeps their coefficients and LDE between proofs and transforms them once: every load compares
 * those columns of the trace with the generators' words on the device (a valid witness may differ there: such a trace is proved as
 * before, and so is the one after it), sbn_prover_generate_trace* writes them itself.  SBN_FIXED_COLUMNS=0 transforms them in every
 * proof.  Same proof words either way; sbn_prover_describe reports the switch, the range the context keeps and the columns the
 * last prove() left untransformed (fixed_columns, fixed_columns_range, fixed_columns_skipped).  No device involved. */
int sbn_fixed_columns_range(const sbn_air_desc* air, uint32_t* first_out, uint32_t* end_out);
/* Building block: that comparison alone.  block = the columns above of a trace of 2^degree_bits rows, column-major, host memory;
 * *match_out = 1 when every word is the generators', else 0. */
int sbn_fixed_columns_check(const sbn_air_desc* air, uint32_t degree_bits, const uint64_t* block, int* match_out);
/* Witness generation ON THE DEVICE, straight into the prover's trace buffer: G1ExpStark / G2ExpStark / Fq12ExpStark / FqExpStark
 * ::generate_trace + generate_public_inputs (src/curves/g1/exp.rs:255-327, src/curves/g2/exp.rs:271-342,
 * src/fields/fq12/exp.rs:283-319) without the trace ever crossing PCIe.  Same `ios` layout and the same resulting trace /
 * public inputs, bit for bit, as sbn_generate_trace_{g1,g2,fq12}_exp; afterwards the prover is loaded and
 * sbn_prover_prove can run.  pi_out (optional): [num_public_inputs].  G1_EXP / G2_EXP / FQ_EXP: 2^16 .. 2^20 rows, 128 .. 2,048 instances (the
 * reference pads to any power of two >= 128 instances, src/curves/g1/circuit.rs:273-277; 2,048 is the largest num_io an Exp
 * table is created with: at 4,096 the 4 num_io pulse columns alone are 275 GB of trace); FQ12_EXP, FQ12_EXP_U64: any size.  A call that fails, for whatever reason
 * (a coordinate >= p, a degenerate instance, a non-canonical exponent), leaves NO trace loaded: sbn_prover_prove then fails
 * with SBN_ERR_BAD_ARG until a trace is generated or loaded again. */
int sbn_prover_generate_trace(sbn_prover* p, const uint32_t* ios, size_t num_io, uint64_t* pi_out);
/* Chained instance lists: the call shape of the reference's *_msm tests (test_g1_msm, src/curves/g1/circuit.rs:459-509, and
 * test_g2_msm, test_fq12_msm, test_fq12_u64_msm), where offset[0] is a fixed start value and offset[k+1] is the output of
 * instance k, so that the last output is start + sum e_k x_k on the curves and start * prod x_k^e_k in the fields.
 * kind: one of the five Exp tables (sbn_air_kind).  terms: [count][T] u32, an instance row of the table's `ios` without its
 * offset words (x, then exp_val): T = 24 (G1_EXP), 40 (G2_EXP), 16 (FQ_EXP), 104 (FQ12_EXP), 98 (FQ12_EXP_U64).  start: the offset
 * words of instance 0 (16, 32, 8, 96, 96 u32).  ios_out: [count][40 | 72 | 24 | 200 | 194] u32, the explicit list in the layout
 * the generators above and sbn_prover_generate_trace take: offset[0] = start, offset[k+1] = offset[k] + e_k x_k (curves) or
 * offset[k] * x_k^e_k (fields, 0^0 = 1), every value canonical and affine.  final_out (optional): the last output, in the word
 * shape of start.  Any count >= 1; the terms run on the host pool (SBN_HOST_THREADS).
 * Refused: a coordinate, coefficient or exponent that the generators refuse (>= p: SBN_ERR_BAD_ARG; a FQ12_EXP_U64 exponent that is
 * not a canonical field element: SBN_ERR_NON_CANONICAL); on the curves a start or an x_k that is not on the table's curve
 * (y^2 = x^3 + 3, the twist y^2 = x^3 + 3/(9+i); points off the prime-order subgroup of the twist are fine): SBN_ERR_BAD_ARG
 * naming the instance, because the running sum is independent of its bracketing only inside a group.  The arithmetic that derives
 * the offsets is complete (identity terms, equal and opposite operands), so SBN_ERR_WITNESS means one of two things only: some
 * offset (or the last output) is the point at infinity and has no affine form, or the table's own walk of the explicit list is
 * degenerate (an addition of the chain B[t+1] = B[t] + bit_t 2^t x meets B[t] = +-2^t x), which the generators refuse as well. */
int sbn_chain_instances(int32_t kind, const uint32_t* terms, size_t count, const uint32_t* start, uint32_t* ios_out, uint32_t* final_out);
/* sbn_prover_generate_trace on the list sbn_chain_instances derives from (terms, start): same tables, sizes and failure rule (a
 * failing call leaves NO trace loaded), and on success the same loaded trace and public inputs, word for word.  ios_out
 * (optional): that list, [num_io][words per instance].  Where the chains of the table run on the device (G1_EXP / G2_EXP under
 * SBN_TRACEGEN_DEVICE_CHAIN=1 or 2, FQ12_EXP / FQ12_EXP_U64 unless SBN_FQ12_HOST_CHAIN=1) the offsets are built there too and
 * the instance list never visits the host between the terms and the witness kernels; elsewhere it is derived on the host pool. */
int sbn_prover_generate_trace_chained(sbn_prover* p, const uint32_t* terms, size_t num_io, const uint32_t* start, uint64_t* pi_out, uint32_t* ios_out);
/* Device -> host copy of the loaded trace, column-major [num_columns][N] (tests, debugging). */
int sbn_prover_read_trace(sbn_prover* p, uint64_t* trace_out);

/* Trace check: which rows of a trace break a constraint -------------------------------------------- */
/* What starky 0.1.1 prover.rs `check_constraints` does inside prove() in a debug build ([DEP-RECALL]):
 * every constraint of the table is evaluated on the TRACE domain H (row i against row i + 1 mod N, L_first = [i == 0],
 * L_last = [i == N - 1], the permutation product Z computed as prove() computes it) and the rows on which one is non-zero are
 * reported.  prove() itself accepts any canonical matrix and returns a proof that sbn_verify then rejects with a reason about a
 * quotient opening; this names the row.
 * A DEBUGGING AID FOR HONEST MISTAKES, NOT A SOUNDNESS STATEMENT: the constraints of a row are folded with powers of two
 * challenges as in the quotient stage, so a broken row escapes one accumulator with probability of about
 * (number of constraints) / 2^64.  The challenges come from the host transcript after it has observed a fixed tag, `seed`, the
 * table kind, num_io, degree_bits and the public inputs: the permutation sets first (tables with Z columns only), then the two
 * alphas, the order of prove().  The same seed gives the same report from the device form and from the host form.
 * GRANULARITY of this report: segment and row.  sbn_explain_rows_host / sbn_prover_explain_rows below name the constraint BLOCKS a
 * row breaks (the emissions of the regrouped evaluator, csrc/air.cuh).
 * The segments are the four of the quotient stage: 0 = AIR head (public inputs, transitions, flags, gadgets; everything of the
 * non-Exp tables), 1 = AIR tail of the Exp tables (io pulses, range check), 2 / 3 = the permutation checks of the Z columns
 * [0, z_split) / [z_split, num_zs).  A wrong cell of a permuted column shows in segment 2 or 3 on row N - 1 only: Z is the
 * running product, so only its closing row can break.  WHICH values and rows are behind such a failure is the answer of
 * sbn_explain_permutations_host / sbn_prover_explain_permutations below: the exact multiset difference of the pair's columns. */
typedef struct sbn_trace_report {
  uint32_t struct_size;          /* caller sets sizeof(sbn_trace_report) */
  uint32_t num_segments;         /* 4 */
  uint64_t rows;                 /* N */
  uint64_t failing_rows;         /* rows on which any segment is non-zero */
  uint64_t first_failing_row;    /* UINT64_MAX when failing_rows == 0 */
  uint64_t seg_failing_rows[4];
  uint64_t seg_first_row[4];     /* UINT64_MAX when that segment is clean */
  uint32_t num_zs, z_split;      /* segment 2 = Z columns [0, z_split), segment 3 = [z_split, num_zs) */
} sbn_trace_report;
/* The loaded trace of a single-GPU prover, checked on the device (csrc/trace_check.hip: the constraint kernels of the quotient
 * stage pointed at the trace values, then one reduction).  row_flags_out (optional): [N] bytes, bit s of byte i set when either
 * accumulator of segment s is non-zero on row i.  SBN_OK = the check ran, the verdict is in the report.  SBN_ERR_BAD_ARG: a null
 * argument, a wrong struct_size, no trace loaded (also after a failed sbn_prover_generate_trace); SBN_ERR_UNSUPPORTED: the
 * context of a split prover with world > 1.  The trace stays loaded and untouched (only per-proof scratch is overwritten):
 * sbn_prover_prove gives the same words before and after. */
int sbn_prover_check_trace(sbn_prover* p, uint64_t seed, sbn_trace_report* report, uint8_t* row_flags_out);
/* Device times of the last sbn_prover_check_trace (ms, HIP events): permutation Z, constraint kernels (with the tables of H and
 * the upload of the alpha powers), reduction, download of the report block; returns the number written. */
int sbn_prover_check_times(const sbn_prover* p, float* ms_out, int cap);
/* The same check on host threads (SBN_HOST_THREADS), no device looked for: the same report and the same flags for the same
 * seed.  Tables and heights as sbn_prover_create accepts them (SBN_ERR_BAD_ARG for an unknown table, SBN_ERR_UNSUPPORTED for a
 * height it does not prove); a word >= p: SBN_ERR_NON_CANONICAL naming the smallest such index, as sbn_prover_load_trace. */
int sbn_check_trace_host(const sbn_air_desc* air, const uint64_t* trace_col_major, uint32_t degree_bits,
                         const uint64_t* public_inputs, size_t n_pi, uint64_t seed,
                         sbn_trace_report* report, uint8_t* row_flags_out);
const char* sbn_trace_segment_name(int s);   /* "air_head", "air_tail", "perm_lo", "perm_hi"; "" otherwise */

/* Explain: which constraint BLOCKS a failing row breaks ------------------------------------------------ */
/* The regrouped evaluator (csrc/air.cuh) does not fold constraints one by one: it EMITS either one constraint or a gadget's
 * local sum over `count` consecutive constraints with the filter factored out.  The sequence of emissions depends on the table
 * (kind, num_io) only and is in the emission order of the reference's eval_packed_generic; every emission is one block.  A
 * recording form of the consumer (csrc/air_record.cuh; the forms the prover and the verifier run are untouched) reduces the
 * contribution of each emission alone under both challenges and flags the block when either is non-zero.
 * A BLOCK IS THE GRANULARITY: inside a merged block (a gadget: up to 792 constraints; the public-input binding: num_pi
 * constraints; a transition case; the flags) the factored sums cannot separate constraints.  The same disclaimer as for the
 * trace check: a debugging aid, a broken block escapes with probability of about count / 2^64.
 * Sections (sbn_constraint_block.section, names from sbn_constraint_section_name):
 *    0 output_pulse_sum            is_final - sum of the output pulses (Exp and Flag tables)
 *    1 public_inputs               the public-input binding of the Exp tables, num_pi constraints in one block
 *    2 transition_double, 3 transition_add, 4 transition_hold
 *                                  the three cases of the state transition of the Exp tables (square / multiply / hold in
 *                                  the square-and-multiply tables FQ_EXP, FQ12_EXP, FQ12_EXP_U64)
 *    5 flags, 10 flags_repeat      eval_flags and its second emission after the gadgets (one block each)
 *    6 gadget_add, 7 gadget_double the curve gadgets (G1_OP, G1_EXP, G2_EXP), one block each
 *    8 gadget_sq, 9 gadget_mul     the field gadgets (FQ_EXP, FQ12_EXP, FQ12_EXP_U64; MODULAR and FQ12_MUL have gadget_mul only)
 *   11 rotation_pulse              the five constraints of the periodic pulse, instance = 0..4
 *   12 io_pulse                    the counter's two constraints (no instance), then two per pulse position, instance = position
 *   13 range_check_recomposition   split range check: target = lo + 256 hi, instance = range-checked column k
 *   14 range_check_lookup          the two constraints of every lookup pair, one block each, instance = range-checked column k
 *                                  (a split range check has a lo and a hi pair per column)
 *   15 range_table                 the three constraints of the range table column
 *   16 lookup                      the two lookup constraints of the LOOKUP table */
typedef struct sbn_constraint_block {
  uint32_t first, count;     /* constraints [first, first + count) of the table's AIR stream, in the emission order of
                                eval_packed_generic: 0 = the first constraint emitted (its weight is alpha^(n-1)) */
  uint32_t segment;          /* 0 = air_head, 1 = air_tail: the segments of sbn_trace_report */
  uint32_t section;          /* what the block is, see above */
  uint32_t instance;         /* index inside the section where it has one (io pulse i, range-checked column k), else UINT32_MAX */
  uint32_t col_first, col_count; /* the most specific span of trace columns the block is about (0, 0 where there is none) */
} sbn_constraint_block;
/* The block table of a table, no device: recorded by running the recording consumer once over a zero row, so it cannot drift
 * from the evaluator.  Writes min(B, cap) entries (out may be null) and returns B; 0 for an unknown table.  The blocks are in
 * order, partition [0, sbn_air_num_constraints), and the head / tail boundary of the Exp tables is a block boundary. */
size_t sbn_air_constraint_blocks(const sbn_air_desc* air, sbn_constraint_block* out, size_t cap);
const char* sbn_constraint_section_name(int section);   /* "" for a value that is no section */
/* The trace columns whose permutation Z column z checks (lhs against rhs), z < sbn_air_num_permutation_zs. */
int sbn_air_permutation_pair(const sbn_air_desc* air, size_t z, uint32_t* lhs_col, uint32_t* rhs_col);
/* rows[n_rows]: any rows of the trace.  block_flags_out: [n_rows][(B + 7) / 8] bytes, bit b of row r's entry = block b is non-zero
 * on rows[r] (row i against row i + 1 mod N, the selectors of the trace domain, the challenges of sbn_check_trace_host for the
 * same seed).  z_flags_out (optional; tables with Z columns): [n_rows][(num_zs + 7) / 8], bit z = the first-row constraint or the
 * transition of Z column z is non-zero on that row, Z computed as prove() computes it.  Host threads, no device looked for;
 * argument checks, canonical-form refusal, tables and heights as sbn_check_trace_host; a row >= N: SBN_ERR_BAD_ARG. */
int sbn_explain_rows_host(const sbn_air_desc* air, const uint64_t* trace_col_major, uint32_t degree_bits, const uint64_t* public_inputs,
                          size_t n_pi, uint64_t seed, const uint64_t* rows, size_t n_rows, uint8_t* block_flags_out, uint8_t* z_flags_out);
typedef struct sbn_block_stat { uint64_t failing_rows, first_row; } sbn_block_stat;   /* first_row = UINT64_MAX when clean */
/* The same over EVERY row, summed: block_stats_out[B], z_stats_out[num_zs] (optional).  The summary a systematically wrong column
 * needs: "gadget_add [181, 346) fails on 65,024 rows, first on row 1". */
int sbn_explain_trace_host(const sbn_air_desc* air, const uint64_t* trace_col_major, uint32_t degree_bits, const uint64_t* public_inputs,
                           size_t n_pi, uint64_t seed, sbn_block_stat* block_stats_out, sbn_block_stat* z_stats_out);
/* The same two on the loaded trace of a single-GPU prover (csrc/trace_explain.hip: one thread per row runs the evaluator through
 * the recording consumer; a wave ballots every block and one lane adds the count), bit for bit what the host forms give for the
 * same seed.  SBN_ERR_BAD_ARG: a null argument, a row >= N, no trace loaded; SBN_ERR_UNSUPPORTED: the context of a split prover
 * with world > 1.  Only per-proof scratch is overwritten: sbn_prover_prove gives the same words before and after. */
int sbn_prover_explain_rows(sbn_prover* p, uint64_t seed, const uint64_t* rows, size_t n_rows, uint8_t* block_flags_out, uint8_t* z_flags_out);
int sbn_prover_explain_trace(sbn_prover* p, uint64_t seed, sbn_block_stat* block_stats_out, sbn_block_stat* z_stats_out);
/* Device times of the last explain call (ms, HIP events): permutation Z, explain kernels (with the tables of H and the upload of
 * the alpha powers), reduction / download; returns the number written. */
int sbn_prover_explain_times(const sbn_prover* p, float* ms_out, int cap);

/* Explain: the values and rows behind a failing permutation pair --------------------------------------- */
/* Z column z checks the MULTISET of trace column lhs_z against that of column rhs_z (sbn_air_permutation_pair); the running
 * product hides where they differ.  These calls compare the two columns of every chosen pair directly, as multisets of canonical
 * 64-bit words: exact, no challenge, no seed, and the trace need not satisfy the AIR -- only the pair structure of the table is
 * used.  Per pair, exact whatever per_pair is: differing_values = distinct values v with count_lhs(v) != count_rhs(v);
 * excess_lhs = sum of max(count_lhs - count_rhs, 0), excess_rhs the same the other way; entries = min(differing_values,
 * per_pair).  The differing values are listed SMALLEST first, ascending, at most per_pair of them; first_row_* is the smallest
 * row that holds the value in that column, UINT64_MAX when the count is 0.  A table without Z columns gives nothing to write. */
typedef struct sbn_perm_pair_stat { uint64_t differing_values, excess_lhs, excess_rhs, entries; } sbn_perm_pair_stat;
typedef struct sbn_perm_diff_entry { uint64_t value, count_lhs, count_rhs, first_row_lhs, first_row_rhs; } sbn_perm_diff_entry;
/* Host threads (SBN_HOST_THREADS; csrc/perm_diff.hpp: values below 2^16 in a signed histogram, the others sorted), one pair per
 * task, no device looked for.  zs == NULL: all pairs (n_zs ignored), output index = z; else output index k is pair zs[k]
 * (z >= num_zs: SBN_ERR_BAD_ARG).  stats_out: [n_out]; entries_out: [n_out][per_pair], may be NULL when per_pair == 0; of pair
 * k's per_pair slots the first stats_out[k].entries are written.  Null arguments, tables and heights, and the canonical-form
 * refusal (SBN_ERR_NON_CANONICAL naming the smallest index) as sbn_explain_rows_host. */
int sbn_explain_permutations_host(const sbn_air_desc* air, const uint64_t* trace_col_major, uint32_t degree_bits,
                                  const uint32_t* zs, size_t n_zs, size_t per_pair,
                                  sbn_perm_pair_stat* stats_out, sbn_perm_diff_entry* entries_out);
/* The same bytes for the loaded trace of a single-GPU prover (csrc/perm_diff.hip, csrc/kernels_permdiff.cuh): two workgroups per
 * pair hold signed 32-bit histograms of half of [0, 2^16) each in 128 KiB of LDS, a second kernel re-reads the columns of the
 * pairs that differ for counts and first rows.  A pair ends on one of three routes, all exact: BINS, every cell below 2^16 (the
 * kernels alone); LIST, the cells >= 2^16 of the launch fitted a bounded list (4,096 cells) that the host diffs behind the binned
 * values; DOWNLOAD, the list overflowed -- LookupStark at large heights always -- or per_pair > 1,024 and more binned values
 * differ: the two columns come back and the host routine diffs them.  sbn_prover_describe reports the pairs of the last call by
 * route as perm_diff_routes=bins:list:download.  SBN_ERR_BAD_ARG: a null argument, z >= num_zs, no trace loaded;
 * SBN_ERR_UNSUPPORTED: the context of a split prover with world > 1.  Only per-proof scratch is overwritten: sbn_prover_prove
 * gives the same words before and after. */
int sbn_prover_explain_permutations(sbn_prover* p, const uint32_t* zs, size_t n_zs, size_t per_pair,
                                    sbn_perm_pair_stat* stats_out, sbn_perm_diff_entry* entries_out);
/* Times of the last sbn_prover_explain_permutations (ms): histogram kernel, rows pass (HIP events), download + host merge (host
 * clock); returns the number written. */
int sbn_prover_explain_permutation_times(const sbn_prover* p, float* ms_out, int cap);

/* Name the cells: a loaded trace against its canonical witness ----------------------------------------- */
/* A block is the finest unit the explain calls above reach.  For the five Exp tables the library knows more: the witness is a
 * function of the instance list, and the instance list sits in the public inputs.  The CANONICAL WITNESS of a list is the trace the
 * five Exp generators of sbn_generate_trace_* write for it -- bit for bit what sbn_prover_generate_trace produces.  These calls
 * compare a trace with it word by word: exact, no challenge, no seed, deterministic, and every count is exact whatever cells_cap is.
 *   cells, main_cells       the differing cells over all columns, and those of them in columns [0, sbn_air_num_main_columns)
 *   rows, columns           the rows and the columns that hold at least one differing cell
 *   first_row, first_column the smallest (row, column), row first, over the main columns; over the derived columns when no main
 *                           cell differs; UINT64_MAX when none does
 *   listed                  entries written to cells_out = min(cells, cells_cap): ascending (row, column) over the MAIN columns, and
 *                           only once those are exhausted the same order over the derived columns.  Main columns come first because
 *                           the chains make every later row depend on earlier ones: the first main cell is the cause, while a sorted
 *                           range-check column may differ on much earlier rows as a consequence.
 *   pi_words, first_pi_word the loaded public-input words that differ from the public inputs the instances determine (in practice
 *                           wrong outputs; with a given `ios` also input words); UINT64_MAX when none does
 * column_cells_out, column_first_row_out (both optional): [sbn_air_num_columns] words, the differing cells of each column and its
 * first differing row (all ones when it has none).  cells_cap: 0 .. 65536, 0 asks for the statistics only (cells_out may be NULL). */
typedef struct sbn_witness_diff {
  uint32_t struct_size;          /* caller sets sizeof(sbn_witness_diff) */
  uint32_t reserved;
  uint64_t cells, main_cells, rows, columns;
  uint64_t first_row, first_column;
  uint64_t listed;
  uint64_t pi_words, first_pi_word;
} sbn_witness_diff;
typedef struct sbn_witness_cell { uint64_t row, column, got, want; } sbn_witness_cell;
/* The instance list the public inputs of an Exp table carry: the inverse of the tables' generate_public_inputs, on the host.  Per
 * instance the public inputs are x, offset, exponent, output; limbs are u32 on the curves and in FQ_EXP, 16-bit in the Fq12 tables,
 * the FQ12_EXP_U64 exponent is one word.  ios_out: [num_io] rows in the layout sbn_generate_trace_* takes; outputs_out (optional):
 * [num_io] values in the word shape of x.  SBN_ERR_BAD_ARG: a null argument, a kind that is no Exp table, n_pi that is not num_io
 * instances, or a limb out of its range, naming the public-input index. */
int sbn_instances_from_public_inputs(int32_t kind, const uint64_t* public_inputs, size_t n_pi, size_t num_io,
                                     uint32_t* ios_out, uint32_t* outputs_out);
/* The loaded trace of a single-GPU prover against the canonical witness of `ios` (csrc/witness_diff.hip,
 * csrc/kernels_witdiff.cuh).  ios == NULL: the instances are taken from the loaded public inputs; a given ios is compared as given.
 * The witness is generated on the device into the coefficient buffer, which is idle between proofs; one kernel compares the two
 * matrices, a second lists the cells of the chosen rows.  Refusals, in this order, the argument checks before a device is looked for:
 *   1. SBN_ERR_BAD_ARG: a null p or report, a wrong struct_size, cells_cap > 65536, cells_out NULL with a cap, num_io not the table's;
 *   2. SBN_ERR_BAD_ARG: no trace loaded;  3. SBN_ERR_UNSUPPORTED: a table that is no Exp table (no instance list in its public
 *   inputs);  4. SBN_ERR_UNSUPPORTED: the context of a split prover;  5. SBN_ERR_UNSUPPORTED: a height the device witness does not
 *   cover (G1 / G2 / FQ_EXP below 2^16 rows: no such table);  6. what the generator says about the list (a value
 *   >= p, a non-canonical exponent, SBN_ERR_WITNESS), behind "no canonical witness: ".
 * SBN_OK = the diff ran; whether anything differs is in the report.  On EVERY path the loaded trace, its public inputs and the
 * loaded state come out as they went in -- also after a refused list: sbn_prover_prove gives the same words before and after. */
int sbn_prover_diff_witness(sbn_prover* p, const uint32_t* ios, size_t num_io, sbn_witness_diff* report,
                            uint64_t* column_cells_out, uint64_t* column_first_row_out,
                            sbn_witness_cell* cells_out, size_t cells_cap);
/* Times of the last sbn_prover_diff_witness (ms): the device witness, the compare kernel (HIP events), listing + downloads (host
 * clock); returns the number written. */
int sbn_prover_diff_witness_times(const sbn_prover* p, float* ms_out, int cap);
/* The host twin, no device looked for: the host generator runs on the host pool (SBN_HOST_THREADS) into a temporary of the trace's
 * size and the matrices are compared in tiles of 64 x 64.  The same report, arrays and list.  Any height the host generators take,
 * as the device form.  Refusals as above without 2, 4 and 5; degree_bits or n_pi that do not match the table:
 * SBN_ERR_BAD_ARG. */
int sbn_diff_witness_host(const sbn_air_desc* air, const uint64_t* trace_col_major, uint32_t degree_bits,
                          const uint64_t* public_inputs, size_t n_pi, const uint32_t* ios, size_t num_io,
                          sbn_witness_diff* report, uint64_t* column_cells_out, uint64_t* column_first_row_out,
                          sbn_witness_cell* cells_out, size_t cells_cap);

/* One-shot convenience with the reference's argument list:
 * prove(stark, &config, trace_poly_values, public_inputs) (src/curves/g1/exp.rs:818-825): a device context, then
 * sbn_prover_prove_host_trace.  The context is created and destroyed per call unless sbn_prove_cache_configure keeps it. */
int sbn_prove(const sbn_air_desc* air, const sbn_config* cfg, const uint64_t* trace_col_major, uint32_t degree_bits,
              const uint64_t* public_inputs, size_t n_pi, sbn_proof** out);

/* sbn_prove with the argument list of sbn_prover_prove_host_columns: the same context cache, key and statistics. */
int sbn_prove_columns(const sbn_air_desc* air, const sbn_config* cfg, const uint64_t* const* columns, size_t n_columns,
                      uint32_t degree_bits, uint32_t flags, const uint64_t* public_inputs, size_t n_pi, sbn_proof** out);
/* sbn_prove for a row-major trace (sbn_prover_prove_host_rows; degree_bits = log2 of rows->n_rows): the same cache, key and
 * statistics.  The refusals 1 .. 8 of the list at sbn_host_rows run before a device is looked for. */
int sbn_prove_rows(const sbn_air_desc* air, const sbn_config* cfg, const sbn_host_rows* rows, uint32_t flags, const uint64_t* public_inputs,
                   size_t n_pi, sbn_proof** out);

/* sbn_prove keeps the device contexts it creates, keyed by (device, kind, num_io, degree_bits, every sbn_config field),
 * up to budget_bytes of device memory, least recently used evicted first.  0 (the default) = create and destroy per
 * call, as before; setting 0 also destroys what is cached.  Thread-safe.  A context is handed to one call at a time: a
 * concurrent call for the same key works on a temporary context of its own.  A context larger than the whole budget is
 * never kept, and neither is one whose call failed.  A cached context keeps the SBN_* switches it was created under (they
 * are read when a context is created, see sbn_prover_describe); configure 0 and the budget again to have them read anew.
 * Nothing is released at process exit: call this with 0 before unloading the library or resetting the device. */
int sbn_prove_cache_configure(uint64_t budget_bytes);
/* out[0..5] = hits, misses, evictions, contexts resident, bytes resident, budget. */
int sbn_prove_cache_stats(uint64_t out[6]);

/* Batch mode (BASELINE config "batch of independent proofs"): `inflight` prover contexts on the current GPU with one
 * host thread each.  Every unit is one instance list of the table (`num_io` instances, `ios_words_per_unit` u32 words,
 * layouts as for sbn_generate_trace_*): its witness is generated on the device and proved; proofs_out[count] receives
 * the proofs in unit order (all freed and an error returned if any unit fails).  The reference counterpart is the loop
 * of `G1ExpStarkyProofGenerator::run_once` calls over chunks of 128 instances (src/curves/g1/circuit.rs:161-202). */
typedef struct sbn_batch_prover sbn_batch_prover;
int sbn_batch_prover_create(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, uint32_t inflight, sbn_batch_prover** out);
/* The same with the options of sbn_prover_create_with for every context of the batch (NULL: as above). */
int sbn_batch_prover_create_with(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, uint32_t inflight, const sbn_prover_options* opt,
                                 sbn_batch_prover** out);
int sbn_batch_prover_prove_ios(sbn_batch_prover* b, const uint32_t* ios, size_t ios_words_per_unit, size_t num_io, size_t count, sbn_proof** proofs_out);
/* `count` units whose traces are in host memory, one allocation per column: columns[u * n_columns + c] is column c of unit u,
 * public_inputs[u] its n_pi public inputs (public_inputs may be null when n_pi is 0), flags as for sbn_prover_prove_host_columns.
 * Any table kind.  Each context's thread takes the next unit and uploads on the context's own copy stream, so one unit's PCIe time
 * runs beside the other contexts' kernels.  proofs_out[count] in unit order, each the proof of sbn_prover_prove_host_columns on
 * that unit.  On a failure: the status of the failing unit with the smallest index, its message behind "unit %zu: ", every
 * proofs_out entry null, and the batch prover usable. */
int sbn_batch_prover_prove_host_columns(sbn_batch_prover* b, const uint64_t* const* columns /* [count][n_columns] */, size_t n_columns,
                                        uint32_t flags, const uint64_t* const* public_inputs /* [count] */, size_t n_pi, size_t count,
                                        sbn_proof** proofs_out);
void sbn_batch_prover_destroy(sbn_batch_prover* b);

/* Verified proving: no proof leaves a guarded context unless it verifies ------------------------------ */
/* The reference never uses a proof it has not verified: G1ExpStarkyProofGenerator::run_once (src/curves/g1/circuit.rs:187-201) calls
 * prove(...) and, on the next line, verify_stark_proof(stark, inner_proof.clone(), &inner_config).unwrap(); the G2, Fq, Fq12 and
 * Fq12-u64 generators do the same.  A guard joins the two halves inside the library.  THE PROMISE of a guarded context: a proof it
 * returns has passed the verifier the caller's consumer will run.
 * With a guard set, every call that returns an sbn_proof from the context -- sbn_prover_prove, sbn_prover_prove_host_trace,
 * sbn_prover_prove_host_columns, sbn_prover_prove_host_rows, every sbn_batch_prover_prove_* call, and sbn_prove / sbn_prove_columns /
 * sbn_prove_rows under sbn_prove_set_guard -- verifies the assembled WORDS, the array sbn_proof_serialize would write (not the device
 * buffers they came from), before it returns.
 *   SBN_GUARD_HOST    sbn_verify on the calling thread.
 *   SBN_GUARD_DEVICE  a device verifier of batch 1 (sbn_verifier_create) that the context owns: created by the first guarded proof,
 *                     on the context's device, for the context's (air, cfg, degree_bits); destroyed with the context; kept when the
 *                     mode goes back to SBN_GUARD_OFF.  Its device bytes are outside sbn_prover_memory_plan (as the 8 bytes of the
 *                     canonical-form scan are); sbn_prover_describe reports them as guard_bytes, the stats as out[3], and the
 *                     one-shot context cache counts them against its budget.
 * A proof that verifies: the words are those of the unguarded call; the trace stays loaded, sbn_prover_prove can be repeated.
 * A proof that does not: SBN_ERR_VERIFY_FAILED, sbn_last_error() = the verifier's own reason (the same text in both modes, the one
 * sbn_verify leaves), *out null, and the trace STAYS LOADED -- also after the load-and-prove calls, which otherwise leave none behind
 * a failure -- so that sbn_prover_check_trace, sbn_prover_explain_* and sbn_prover_diff_witness can name the cause.  There is no retry:
 * a unit that fails is reported, and the stats count it.  The batch calls keep their failure rule (every proof slot null, the batch
 * prover usable): the status and the message of the failing unit with the smallest index, behind "unit %zu: ".  In a batch every
 * context checks its own proof on its own worker thread with its own verifier; no verifier is shared, no lock is taken, and the other
 * contexts keep proving meanwhile.  The guard enqueues nothing on the prover's streams: the device verifier has its own.
 * Refused before any device is looked for, in this order: a null handle, then an unknown mode: SBN_ERR_BAD_ARG; the context of a
 * split prover, whatever its world size and whatever the mode: SBN_ERR_UNSUPPORTED (the ranks would have to agree on the verdict).
 * Setting the mode a context already has changes nothing.  With SBN_GUARD_OFF, the default, every call is exactly the unguarded one. */
enum { SBN_GUARD_OFF = 0, SBN_GUARD_DEVICE = 1, SBN_GUARD_HOST = 2 };
int sbn_prover_set_guard(sbn_prover* p, uint32_t mode);
int sbn_batch_prover_set_guard(sbn_batch_prover* b, uint32_t mode);   /* every context of the batch */
/* The one-shot calls sbn_prove / sbn_prove_columns / sbn_prove_rows, process-wide, as sbn_prove_cache_configure: the context of a
 * call, cached or fresh, is given this mode before it proves.  A refused mode leaves the setting as it was. */
int sbn_prove_set_guard(uint32_t mode);
/* out[0..3] = proofs checked, proofs rejected, nanoseconds spent checking (host clock, the lazy creation of the device verifier
 * included), device bytes of the guard (0 until a device guard has checked its first proof).  Plain counters of the context: read
 * them between calls, not while another thread proves on it. */
int sbn_prover_guard_stats(const sbn_prover* p, uint64_t out[4]);
int sbn_batch_prover_guard_stats(const sbn_batch_prover* b, uint64_t out[4]);   /* summed over its contexts */

/* Long chained lists ------------------------------------------------------------------------------- */
/* An MSM / multi-exponentiation of ANY length as proofs of one table: the chained list of sbn_chain_instances cut into units of
 * num_io instances, the last unit padded as the reference's g1_exp_circuit pads a short list (src/curves/g1/circuit.rs:273-277,
 * 303: resized with copies of the LAST input, only outputs[..n] used).  "These units prove this MSM" means: every unit proof
 * verifies (sbn_verify / sbn_verifier_verify) AND sbn_msm_check_links accepts their public inputs; the reference states the
 * second half with `connect` calls inside its circuit (circuit.rs:480-483). */
size_t sbn_msm_num_units(size_t count, size_t num_io);   /* ceil(count / num_io); 0 when either is 0 */
/* The padded, unit-cut list, host pool, no device.  kind, terms, start, final_out and the refusals as sbn_chain_instances (the
 * refusals name the GLOBAL instance index); ios_out: [units * num_io][words per instance]: rows [0, count) are what
 * sbn_chain_instances writes, rows [count, units * num_io) are copies of row count - 1 (x, offset and exponent), final_out
 * (optional) is the output of instance count - 1.  count == 0 or num_io == 0: SBN_ERR_BAD_ARG.  num_io is not checked against any
 * table (this only shapes a list); a single padded unit (count < num_io) is a legal call. */
int sbn_msm_instances(int32_t kind, const uint32_t* terms, size_t count, size_t num_io, const uint32_t* start, uint32_t* ios_out, uint32_t* final_out);
/* Proves the units of that list on the contexts of a batch prover (its table's num_io): proofs_out[units] in unit order, final_out
 * (optional) and ios_out (optional) as sbn_msm_instances.  Proofs, public inputs and ios_out are word for word what
 * sbn_batch_prover_prove_ios gives on the list of sbn_msm_instances.  Failure rule as prove_ios: the status and message of the first
 * failing unit (or of the checks of the whole list, naming the global instance), every proof freed, proofs_out all null; the batch
 * prover stays usable.  The list is derived once on the host pool (sbn_msm_instances) in every placement of the table's chains, so
 * every unit's start is known before the first unit is taken and no context waits for another; the units then go through the
 * explicit-list path of sbn_batch_prover_prove_ios. */
int sbn_batch_prover_prove_msm(sbn_batch_prover* b, const uint32_t* terms, size_t count, const uint32_t* start, sbn_proof** proofs_out,
                               uint32_t* final_out, uint32_t* ios_out);
/* The link check on the public inputs of the unit proofs (host, no device): public_inputs[u] = the [num_pi] public inputs of unit
 * u of the table (kind, num_io).  Checked, in instance order: units == sbn_msm_num_units(count, num_io); the offset of global
 * instance 0 equals start; offset[g + 1] == output[g] for every g < count - 1, across unit boundaries; every pad instance equals
 * instance count - 1 in x, offset, exponent and output; with terms (optional, [count][T] as sbn_chain_instances), x and exponent of
 * every real instance equal the caller's.  SBN_OK and final_out (optional) = the output of instance count - 1 in the word shape of
 * start, or SBN_ERR_VERIFY_FAILED with sbn_last_error naming the first global instance and field that breaks.
 * It does NOT verify any proof: that is sbn_verify or sbn_verifier_verify on each unit. */
int sbn_msm_check_links(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count,
                        const uint32_t* terms, const uint32_t* start, uint32_t* final_out);

/* Scalar multiplications ----------------------------------------------------------------------------- */
/* The INDEPENDENT batch: every instance of a G1_EXP / G2_EXP list carries the same offset and the caller wants e_k x_k itself, not
 * offset + e_k x_k.  The reference uses it in g2_mul_by_cofactor_circuit (src/curves/g2/circuit.rs:335-367: x = point, offset = the
 * G2 generator, exp_val = 2p - r, result = output + (-generator): cofactor clearing) and wherever G1ExpOutputGenerator /
 * G2ExpOutputGenerator (src/curves/g1/circuit.rs:111-123) run on independent inputs; the offset exists only because the table
 * cannot hold the point at infinity.  One definition for every entry point below, E = 1 (G1_EXP) or 2 (G2_EXP):
 *   points   [count][16E] u32: the x words of an `ios` row (x.c0 [x.c1] y.c0 [y.c1], eight little-endian u32 limbs each);
 *   scalars  [scalar_count][8] u32, scalar_count = count, or 1 for ONE scalar shared by every instance.  256-bit integers, NEVER
 *            reduced mod r (the twist's group has order r (2p - r): cofactor clearing depends on it);
 *   offset   [16E] u32, or NULL = the curve's generator (sbn_curve_generator), as the reference uses.
 * With units = sbn_msm_num_units(count, num_io) the explicit list has units * num_io rows: row g < count is (points[g], offset,
 * scalar[g]), row g >= count a copy of row count - 1 (the reference's resize rule, as sbn_msm_instances).  Per real instance
 * product[g] = output[g] + (-offset) by the COMPLETE addition: output = offset (e = 0, or e a multiple of the point's order) is the
 * point at infinity, which is not an error (infinity_out[g] = 1, the product words zero); output = -offset cannot happen, because
 * it needs e x = -2 offset, which the doubling branch handles; e x = -offset makes the OUTPUT infinite, which the table cannot
 * hold: SBN_ERR_WITNESS.  products_out: [count][16E] u32, infinity_out: [count] bytes, ios_out: [units * num_io][40 | 72] u32; every
 * output pointer is optional.
 * Refused, in this order: SBN_ERR_UNSUPPORTED for a kind other than the two curve tables (a field table needs none of this: its
 * offset is multiplicative and one is always legal); SBN_ERR_BAD_ARG for a null argument, count = 0, scalar_count outside
 * {1, count}, a coordinate >= p, an offset or a point that is not on the table's curve (naming the instance; the rule of
 * sbn_chain_instances: output - offset = e x only inside a group; points off the prime-order subgroup of the twist are fine and
 * are the normal input of cofactor clearing); SBN_ERR_WITNESS when the table's own walk of an instance is degenerate (B[t] = +-2^t x
 * at a set bit, e.g. x = +-offset with an odd scalar), naming the FIRST such instance: the remedy is another offset. */
int sbn_curve_generator(int32_t kind, uint32_t* out);   /* (1, 2) on G1, ark_bn254's G2Affine::generator() on the twist: [16E] u32 */
int sbn_g2_cofactor(uint32_t out[8]);                   /* 2p - r = 21888242871839275222246405745257275088844257914179612981679871602714643921549 */
/* The explicit list and the products on the host pool, no device (e_k x_k as sbn_chain_instances derives its terms, then the
 * table's-walk check of the list).  num_io is not checked against any table. */
int sbn_scalar_mul_instances(int32_t kind, const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t count, size_t num_io,
                             const uint32_t* offset, uint32_t* ios_out, uint32_t* products_out, uint8_t* infinity_out);
/* One unit (count = num_io) on a prover of the table: on success the loaded trace and the public inputs are, word for word, those
 * of sbn_prover_generate_trace on the list of sbn_scalar_mul_instances; sizes and the failure rule as there (a failing call leaves
 * NO trace loaded).  Where the table's chains run on the device (SBN_TRACEGEN_DEVICE_CHAIN = 1 or 2) the list is expanded there
 * from the points, the scalars and the offset (24 / 40 words per instance go up instead of 40 / 72) and the products are
 * computed there from the instance outputs; a degenerate instance is then named by the host walk on the error path.  Elsewhere
 * the list is derived on the host pool and takes the explicit path. */
int sbn_prover_generate_trace_scalar_muls(sbn_prover* p, const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t num_io,
                                          const uint32_t* offset, uint64_t* pi_out, uint32_t* products_out, uint8_t* infinity_out, uint32_t* ios_out);
/* Any count, as units of the batch prover's table (units as sbn_batch_prover_prove_msm): proofs_out[units] in unit order, word for
 * word what sbn_batch_prover_prove_ios gives on the list of sbn_scalar_mul_instances.  A refused list leaves the batch prover
 * usable and every proofs_out entry null. */
int sbn_batch_prover_prove_scalar_muls(sbn_batch_prover* b, const uint32_t* points, const uint32_t* scalars, size_t scalar_count, size_t count,
                                       const uint32_t* offset, sbn_proof** proofs_out, uint32_t* products_out, uint8_t* infinity_out, uint32_t* ios_out);
/* The twin of sbn_msm_check_links, on the public inputs of the unit proofs (host, no device; it verifies NO proof).
 * SBN_ERR_VERIFY_FAILED naming the instance and the field for: a wrong unit count; an x or exponent that differs from the caller's;
 * an offset that differs from the call's; a pad row that differs from instance count - 1 in x, offset, exponent or output; an output
 * limb out of range; an output that is not a point of the curve.  On success the products and flags are recomputed on the host. */
int sbn_scalar_mul_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, const uint32_t* points,
                         const uint32_t* scalars, size_t scalar_count, const uint32_t* offset, uint32_t* products_out, uint8_t* infinity_out);
/* Cofactor clearing on the twist: the two calls above for G2_EXP with the generator as offset and the shared scalar 2p - r
 * (g2/circuit.rs:335-367).  A batch prover of any other table: SBN_ERR_BAD_ARG. */
int sbn_batch_prover_prove_mul_by_cofactor(sbn_batch_prover* b, const uint32_t* points, size_t count, sbn_proof** proofs_out, uint32_t* cleared_out,
                                           uint8_t* infinity_out, uint32_t* ios_out);
int sbn_mul_by_cofactor_check(size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, const uint32_t* points,
                              uint32_t* cleared_out, uint8_t* infinity_out);

/* Batches of short MSMs -------------------------------------------------------------------------------- */
/* SEGMENTED chained lists packed into shared units.  The reference's g1_exp_circuit (src/curves/g1/circuit.rs:262-304) takes any list
 * of inputs and the caller wires the offsets: some inputs continue a chain, others start a new one.  The everyday workload looks
 * like that -- one public-key aggregation per signature, one product of a few x_k^e_k per pairing check: many short sums, not one
 * long MSM.  One sbn_batch_prover_prove_msm call per sum pads every sum to a whole unit: a thousand 10-term G1 sums are 1,000 unit
 * proofs (the sum of ceil(len_s / num_io)) where their 10,000 instances fit 79 units (ceil of the sum of len_s over num_io).  The
 * two shapes above are the ends of this one: sbn_msm_instances is one segment, sbn_scalar_mul_instances is segments of length 1
 * with a shared start.  One definition for every entry point below; kind is one of the five Exp tables and T (words per term: 24 /
 * 40 / 16 / 104 / 98), W (words per offset value: 16 / 32 / 8 / 96 / 96) and the words per `ios` row are as in sbn_chain_instances:
 *   terms    [M][T] u32: the instances of all segments, one after the other;
 *   lengths  [segments] u64: every length >= 1, their sum is M; head(s) = the global index of the first instance of segment s;
 *   starts   [start_count][W] u32, start_count = segments (one start per segment) or 1 for ONE start shared by all; NULL = the
 *            generator (sbn_curve_generator) on a curve table and one on a field table (start_count is then not read).
 * With units = sbn_msm_num_units(M, num_io) the explicit list has units * num_io rows.  Row g < M: offset[g] = start_s when g =
 * head(s), otherwise the output of instance g - 1 (offset + e x on the curves, offset * x^e in the fields, 0^0 = 1); row g >= M is a
 * copy of row M - 1 in x, offset and exponent (the reference's resize rule, as sbn_msm_instances).  Segments may straddle unit
 * boundaries.  Per segment: finals_out [segments][W] = the output of its last instance; on the two curve tables also sums_out
 * [segments][W] and infinity_out [segments] = final_s + (-start_s) by the COMPLETE addition, as sbn_scalar_mul_instances (a sum at
 * infinity is not an error: flag 1, words zero).  On a field table sums_out / infinity_out must be NULL: with the default start the
 * final is the product.  Every output pointer is optional.
 * Refused, in this order, each naming the GLOBAL instance and its segment: SBN_ERR_UNSUPPORTED for a kind that is no Exp table;
 * SBN_ERR_BAD_ARG for a null argument, segments = 0, a zero length, start_count outside {1, segments}, num_io = 0, sums_out on a field
 * table, a coordinate or coefficient >= p, a start or an x off the table's curve; SBN_ERR_NON_CANONICAL for a FQ12_EXP_U64 exponent
 * that is no canonical field element; SBN_ERR_WITNESS when an offset or a final inside a segment is the point at infinity; then
 * SBN_ERR_WITNESS when the table's own walk of an instance is degenerate.  The same partial sum in another segment with another
 * start is fine. */
/* The explicit list, the finals and the sums on the host pool, no device: the terms in parallel, one pass of complete additions
 * (products) per segment, one batched inversion for the affine forms, then the table's-walk check of the list.  num_io is not
 * checked against any table (this only shapes a list). */
int sbn_msm_batch_instances(int32_t kind, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts, size_t start_count,
                            size_t num_io, uint32_t* ios_out, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out);
/* One unit on a prover of the table: M <= the table's num_io (SBN_ERR_BAD_ARG otherwise), the rest of the unit is padded.  On success
 * the loaded trace, the public inputs and ios_out ([num_io][words per instance]) are, word for word, those of
 * sbn_prover_generate_trace on the list of sbn_msm_batch_instances; a failing call leaves NO trace loaded.  Where the table's chains
 * run on the device (G1_EXP / G2_EXP under SBN_TRACEGEN_DEVICE_CHAIN = 1 or 2; FQ12_EXP / FQ12_EXP_U64 unless SBN_FQ12_HOST_CHAIN)
 * the offsets are built there: on the curves a segmented prefix scan over the terms (a lane adds its partner only inside its own
 * segment), in Fq12 one workgroup per segment walking its own running product; the pads take the offset of instance M - 1; the
 * derived list, the finals and the sums come back with the instance outputs, and an instance the device refuses is named by the host
 * derivation on the error path.  FQ_EXP and the host-chain placements derive on the host pool and take the explicit path.  The
 * words are the same in every placement. */
int sbn_prover_generate_trace_msm_batch(sbn_prover* p, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts,
                                        size_t start_count, uint64_t* pi_out, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out,
                                        uint32_t* ios_out);
/* Any M, as units of the batch prover's table: proofs_out[units] in unit order, word for word what sbn_batch_prover_prove_ios
 * gives on the list of sbn_msm_batch_instances, which is derived once on the host pool (every unit's first offset is known before
 * the first unit is taken, so no context waits for another).  Failure rule as sbn_batch_prover_prove_msm: every proof freed,
 * proofs_out all null, the batch prover usable. */
int sbn_batch_prover_prove_msm_batch(sbn_batch_prover* b, const uint32_t* terms, const uint64_t* lengths, size_t segments, const uint32_t* starts,
                                     size_t start_count, sbn_proof** proofs_out, uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out,
                                     uint32_t* ios_out);
/* The twin of sbn_msm_check_links, on the public inputs of the unit proofs (host, no device; it verifies NO proof).  Checked, in
 * instance order: units == sbn_msm_num_units(M, num_io); the offset of every head equals the start of its segment; offset[g + 1] ==
 * output[g] inside a segment, across unit boundaries; every pad instance equals instance M - 1 in x, offset, exponent and output;
 * with terms (optional), x and exponent of every real instance are the caller's; every output limb is in range.  On the curves
 * every output must be a point of the curve (as sbn_scalar_mul_check) and the sums and flags are recomputed on the host.  SBN_OK
 * and finals_out / sums_out / infinity_out (optional, as above), or SBN_ERR_VERIFY_FAILED with sbn_last_error naming the first global
 * instance, its segment and the field that breaks. */
int sbn_msm_batch_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, const uint64_t* lengths, size_t segments,
                        const uint32_t* terms /*optional*/, const uint32_t* starts, size_t start_count, uint32_t* finals_out, uint32_t* sums_out,
                        uint8_t* infinity_out);

/* Complete sums ---------------------------------------------------------------------------------------- */
/* Batches of short MSMs on G1_EXP / G2_EXP in which the LIBRARY picks the start of every segment, so that no valid curve input is
 * refused and the caller gets the sums e_k x_k back.  The Exp tables add with incomplete affine formulas: a list is refused when
 * an addition of the table's walk meets B[t] = +-2^t x, or when an offset or a final is the point at infinity, and "the remedy is
 * another start" (above).  With the generator as the default start the everyday inputs fail: m G + r H with odd m, sk G, a list that
 * holds -G.  Here the starts come from a fixed table of SBN_START_CANDIDATES points of the table's curve with no chosen relation to
 * the generator (sbn_start_candidate).  G1: x = 2, 3, 4, ... in ascending order, kept where x^3 + 3 is a non-zero square mod p, y the
 * smaller root as an integer, the first eight.  Twist: x = k + i (c0 = k, c1 = 1), k = 0, 1, 2, ..., kept where x^3 + 3 / (9 + i) is a
 * non-zero square in Fq2, y the root whose (c1, c0) integer pair is lexicographically smaller, the first eight; these need not lie in
 * the order-r subgroup (an offset need not).  One definition for every entry point below; kind, terms, lengths, T, W and the units
 * are as in "Batches of short MSMs":
 *   term_infinity  [M] bytes or NULL: a term with term_infinity[g] != 0 is the point at infinity, the identity of an aggregation.
 *                  Its words in `terms` are NOT read or validated; the effective term is (generator, exponent 0), an instance whose
 *                  walk has no addition and whose product is the identity;
 *   terms_out      [M][T] u32: the effective terms;
 *   starts_out     [segments][W] u32 and choice_out [segments] bytes: the start of segment s is candidate choice[s], the SMALLEST
 *                  j < SBN_START_CANDIDATES for which the segment, started from candidate j, has no bad event: an offset or a final
 *                  at infinity, or an addition of the table's walk with B = +-A.  With S_{g-1} the sum of the segment's terms
 *                  before instance g, the bad starts are (+-2^t - k) x_g - S_{g-1} over the set bits t of e_g (k = the value of the
 *                  bits below t) and -S_g: they depend on the segment's own terms only, so the choice of a segment is a pure
 *                  function of its terms and no segment moves another.
 * On success ios_out, finals_out, sums_out and infinity_out are, word for word, what sbn_msm_batch_instances(kind, terms_out,
 * lengths, segments, starts_out, segments, num_io, ...) returns, and that call succeeds (pads copy row M - 1, offset included); so
 * sbn_msm_batch_check(..., terms = terms_out, starts = starts_out, start_count = segments) checks the unit proofs unchanged.  A
 * segment whose sum is the point at infinity is not an error (an all-masked segment is one: flag 1, sum words zero, final = start).
 * Every output pointer is optional.
 * Refused, in this order: SBN_ERR_UNSUPPORTED for a kind that is no Exp table, and for the three field tables (their offset one is
 * always legal, nothing there is incomplete); the SBN_ERR_BAD_ARG refusals of sbn_msm_batch_instances for the arguments (null terms
 * or lengths, segments = 0, a zero length, num_io = 0) and for the values of the terms that are not masked (a coordinate >= p, an x
 * off the table's curve), with the same wording, naming the instance and its segment; SBN_ERR_WITNESS when all eight candidates fail
 * for some segment, naming the smallest such segment, the count of such segments and the instance at which candidate 7 failed.
 * Eight independent points must each hit a bad set of a few hundred points per instance among about 2^254: honest inputs cannot exhaust
 * the table; inputs crafted from the published candidates can, and their remedy is sbn_msm_batch_instances with starts of the
 * caller's own. */
#define SBN_START_CANDIDATES 8
int sbn_start_candidate(int32_t kind, uint32_t j, uint32_t* out /* [16E] */);   /* refusals as sbn_curve_generator; j >= 8: SBN_ERR_BAD_ARG */
/* The derivation on the host pool, no device: the terms and their prefix sums once; candidate 0 on every segment, ALL failing
 * segments collected in one pass (a per-instance status of the table's walk), only those re-derived with the next candidate.
 * num_io is not checked against any table. */
int sbn_msm_batch_instances_complete(int32_t kind, const uint32_t* terms, const uint8_t* term_infinity /* [M] or NULL */, const uint64_t* lengths,
                                     size_t segments, size_t num_io, uint32_t* ios_out, uint32_t* terms_out /* [M][T] */,
                                     uint32_t* starts_out /* [segments][W] */, uint8_t* choice_out /* [segments] */, uint32_t* finals_out,
                                     uint32_t* sums_out, uint8_t* infinity_out);
/* One unit on a prover of the table, M <= num_io: on success the loaded trace, the public inputs and ios_out are those of
 * sbn_prover_generate_trace on the list above; a failing call leaves NO trace loaded.  Where the table's chains run on the device
 * (SBN_TRACEGEN_DEVICE_CHAIN = 1 or 2) the derivation runs there too, on the segmented path of sbn_prover_generate_trace_msm_batch:
 * the start of segment s is candidate choice[s] (an index per segment goes up, not start words), every choice 0 at first; behind
 * the scan and the rebase of the B chains a kernel writes a status word per segment that has a bad event, the host reads the
 * status words back, moves the failing segments to their next candidate and launches start, scan, rebase and status again -- at
 * most eight rounds, and a second one only when a segment failed.  The terms e_k x_k, their partial sums and the A chains enter no
 * start and are computed once.  With every choice 0 the call is the explicit call plus the status kernel and one readback.  The
 * kernels of the explicit-start calls are unchanged (they keep their single error word).  Placement 0 derives on the host pool
 * and takes the explicit path, and a list that exhausts the candidates is worded by the host derivation.  The words are the same
 * in every placement. */
int sbn_prover_generate_trace_msm_batch_complete(sbn_prover* p, const uint32_t* terms, const uint8_t* term_infinity, const uint64_t* lengths,
                                                 size_t segments, uint64_t* pi_out, uint32_t* terms_out, uint32_t* starts_out, uint8_t* choice_out,
                                                 uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out, uint32_t* ios_out);
/* Any M, as units of the batch prover's table: the list is derived once on the host pool, then the units go through the unit loop
 * of sbn_batch_prover_prove_ios.  Failure rule as sbn_batch_prover_prove_msm_batch; guards apply as to every sbn_batch_prover_prove_*
 * call. */
int sbn_batch_prover_prove_msm_batch_complete(sbn_batch_prover* b, const uint32_t* terms, const uint8_t* term_infinity, const uint64_t* lengths,
                                              size_t segments, sbn_proof** proofs_out, uint32_t* terms_out, uint32_t* starts_out, uint8_t* choice_out,
                                              uint32_t* finals_out, uint32_t* sums_out, uint8_t* infinity_out, uint32_t* ios_out);

/* Field powers --------------------------------------------------------------------------------------- */
/* Powers and POWER TOWERS on the three field Exp tables FQ_EXP, FQ12_EXP and FQ12_EXP_U64: the caller wants x^e itself.  A field
 * table needs no offset trick (its offset is multiplicative: every instance here carries offset = 1, word 0 = 1 and the rest 0), but
 * one call shape cannot be said as a list of independent or offset-chained instances: a TOWER, `depth` >= 1 consecutive instances
 * where level 0 has x = base and level l has x = the OUTPUT of level l - 1.  Every level carries the tower's exponent e, so level l
 * outputs base^(e^(l+1)).  FQ12_EXP_U64 exists for this: the BN parameter x = 4965661367192848881 fits a u64 (sbn_bn_x) and the hard
 * part of the final exponentiation starts from f^x, f^(x^2), f^(x^3): one tower of depth 3.  depth = 1 is a batch of independent
 * powers (inverses with e = p - 2, Legendre symbols with (p - 1) / 2, square roots with (p + 1) / 4 in FQ_EXP).
 * One definition for every entry point below, W = 8 (FQ_EXP) or 96 (the Fq12 tables: twelve flat-basis coefficients) u32 words per
 * field element, as in `ios`:
 *   bases  [count][W] u32: the level-0 x of every tower;
 *   exps   [exp_count][8] u32 ([exp_count][2], low word first, for FQ12_EXP_U64), exp_count = count (one exponent per tower), or 1
 *          for ONE exponent shared by every tower; 256-bit integers as they are, never reduced;
 *   depth  common to the towers of a call; the count * depth instances are laid out tower-major (instance g = tower * depth + level).
 * With M = count * depth and units = sbn_msm_num_units(M, num_io) the explicit list has units * num_io rows: row g < M is (x of its
 * level, one, the tower's exponent), row g >= M a copy of row M - 1 (the reference's resize rule, as sbn_msm_instances).  Towers may
 * straddle unit boundaries.  powers_out: [count][depth][W] u32 (the output of every real instance), ios_out: [units * num_io][24 |
 * 200 | 194] u32; both optional.  A zero base and a zero exponent are legal and the table defines the result (x^0 = 1, also for
 * x = 0; 0^e = 0 for e > 0).
 * Refused, in this order: SBN_ERR_UNSUPPORTED for a curve table or a kind that is no Exp table (a curve table takes the scalar
 * multiplications above); SBN_ERR_BAD_ARG for a null argument, count = 0, depth = 0, num_io = 0 or exp_count outside {1, count};
 * then, tower by tower and as the table's own generator refuses an instance, SBN_ERR_BAD_ARG for a base with a coefficient >= p
 * and SBN_ERR_NON_CANONICAL for a u64 exponent that is no canonical field element (>= 2^64 - 2^32 + 1), naming the tower. */
int sbn_bn_x(uint32_t out[2]);   /* the BN parameter x = 4965661367192848881 = 0x44E992B44A6909F1, low word first */
/* The explicit list and the powers on the host pool, no device: towers side by side, the levels of a tower one after the other.
 * num_io is not checked against any table (this only shapes a list). */
int sbn_power_instances(int32_t kind, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count, size_t depth, size_t num_io,
                        uint32_t* ios_out, uint32_t* powers_out);
/* One unit on a prover of the table: count * depth <= the table's num_io (SBN_ERR_BAD_ARG otherwise), the rest of the unit is padded.
 * On success the loaded trace, the public inputs and ios_out ([num_io][words per instance]) are, word for word, those of
 * sbn_prover_generate_trace on the list of sbn_power_instances; sizes and the failure rule as there (a failing call leaves NO trace
 * loaded).  On the Fq12 tables, whose chains run on the device, one workgroup per tower walks its levels there: it writes the output
 * of a level into the x words of the next instance and runs that level's chain, with no host round trip between levels; the pads are
 * filled on the device from the last real instance, and the derived list and the powers come back in the download of the instance
 * outputs.  FQ_EXP (chains on the host pool) and an Fq12 prover created under SBN_FQ12_HOST_CHAIN walk the towers on the host pool and
 * take the explicit path.  The words are the same in every placement. */
int sbn_prover_generate_trace_powers(sbn_prover* p, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count, size_t depth,
                                     uint64_t* pi_out, uint32_t* powers_out, uint32_t* ios_out);
/* Any count, as units of the batch prover's table (units as above): proofs_out[units] in unit order, word for word what
 * sbn_batch_prover_prove_ios gives on the list of sbn_power_instances, which is derived once (every unit's first x is known before
 * the first unit is taken, so no context waits for another).  Failure rule as sbn_batch_prover_prove_msm: a refused list leaves the
 * batch prover usable and every proofs_out entry null. */
int sbn_batch_prover_prove_powers(sbn_batch_prover* b, const uint32_t* bases, const uint32_t* exps, size_t exp_count, size_t count, size_t depth,
                                  sbn_proof** proofs_out, uint32_t* powers_out, uint32_t* ios_out);
/* The twin of sbn_msm_check_links, on the public inputs of the unit proofs (host, no device; it verifies NO proof): what a circuit
 * states with `connect` calls.  Checked, in instance order: units == sbn_msm_num_units(count * depth, num_io); every offset is one;
 * every exponent is the caller's; x of level 0 equals the tower's base; x of level l equals the output of level l - 1, across unit
 * boundaries; every output limb is in range (16 bits in the Fq12 tables, 32 in FQ_EXP) and every output coefficient is < p; every
 * pad instance equals instance count * depth - 1 in x, offset, exponent and output.  SBN_OK and powers_out (optional,
 * [count][depth][W]) = the outputs, or SBN_ERR_VERIFY_FAILED with sbn_last_error naming the first global instance and the field
 * (x, offset, exponent, output) that breaks. */
int sbn_power_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units, size_t count, size_t depth,
                    const uint32_t* bases, const uint32_t* exps, size_t exp_count, uint32_t* powers_out);

/* Field programs ------------------------------------------------------------------------------------- */
/* The general form of the linked lists above, on the three field Exp tables FQ_EXP, FQ12_EXP and FQ12_EXP_U64 (an instance is
 * output = offset * x^e): a PROGRAM is a list of instances whose x and offset are each a literal or the OUTPUT of an earlier
 * instance.  A chained list is the program offset[k+1] = output[k], a tower the program x[l] = output[l-1]; with general links the
 * same table states a product of two earlier results (x = a, offset = b, e = 1), a Frobenius map (e = p), an exponent longer than
 * the exponent field by Horner (acc = acc^(2^B) * x^limb), and a check f * f_inv = 1 by reading the output.  Curve tables are out
 * of scope: a curve output is offset + e x, so an output used as x drags its start along.
 * One definition for every entry point below.  W = 8 (FQ_EXP) or 96 (the Fq12 tables) u32 words per field element and ew = 8 u32
 * words per exponent (2, low word first, for FQ12_EXP_U64), the word shapes of `ios` and of the field powers:
 *   nodes  [count]: node g is instance g of the list.  x and offset are an index into `values` (a literal), or SBN_NODE_OUTPUT | j,
 *          the output of node j, j < g; offset may also be SBN_NODE_ONE, the field's one.  exp is an index into `exps`.
 *   values [n_values][W] u32, exps [n_exps][ew] u32: exponents are used as they are, never reduced.
 * A literal and an earlier output may each be used any number of times, in either position, and the same node may supply both x
 * and offset of one node.  With units = sbn_msm_num_units(count, num_io) the explicit list has units * num_io rows: row g < count is
 * (x, offset, exponent of node g) with every link resolved to its words, row g >= count a copy of row count - 1 (the resize rule,
 * as sbn_msm_instances).  Links may cross unit boundaries.  Outputs follow the table's own walk: 0^0 = 1, and a zero base or a zero
 * offset are legal.  outs_out: [count][W] u32, ios_out: [units * num_io][24 | 200 | 194] u32; both optional.
 * Refused, in this order:
 *   1. SBN_ERR_UNSUPPORTED for a curve table or a kind that is no Exp table;
 *   2. SBN_ERR_BAD_ARG for a null nodes, values or exps, count = 0 or num_io = 0, and count, n_values or n_exps of 2^31 - 1 or more;
 *   3. node by node, naming the node and the field, SBN_ERR_BAD_ARG for a link with j >= g, then a literal index >= n_values, then
 *      SBN_NODE_ONE as x, then an exponent index >= n_exps;
 *   4. for the literals, then the exponents, THAT SOME NODE USES, in index order: SBN_ERR_BAD_ARG for a coefficient >= p and
 *      SBN_ERR_NON_CANONICAL for a u64 exponent that is no canonical field element (>= 2^64 - 2^32 + 1).
 * An unused literal is not read, and no call adds a value refusal that sbn_prover_generate_trace would not make on the explicit list. */
typedef struct sbn_program_node { uint32_t x, offset, exp; } sbn_program_node;
#define SBN_NODE_OUTPUT 0x80000000u  /* x / offset = SBN_NODE_OUTPUT | j : the output of node j, j < this node's index */
#define SBN_NODE_ONE    0x7fffffffu  /* offset only: the field's one */
/* The schedule of a program, which drives the host pool and the device alike: level_out[g] (optional, [count]) = 0 for a node
 * without links, otherwise 1 + the largest level of the nodes it links to; *depth_out (optional) = 1 + the largest level.  The nodes
 * of one level are independent.  Structure only: refuses a null nodes, count = 0 or >= 2^31 - 1, a link with j >= g and
 * SBN_NODE_ONE as x (SBN_ERR_BAD_ARG, naming the node and the field). */
int sbn_program_levels(const sbn_program_node* nodes, size_t count, uint32_t* level_out, uint32_t* depth_out);
/* The explicit list and the outputs on the host pool, no device: level by level, the nodes of a level side by side.  num_io is not
 * checked against any table (this only shapes a list). */
int sbn_program_instances(int32_t kind, const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values,
                          const uint32_t* exps, size_t n_exps, size_t num_io, uint32_t* ios_out, uint32_t* outs_out);
/* One unit on a prover of the table: count <= the table's num_io (SBN_ERR_BAD_ARG otherwise, after refusals 1 and 2), the rest of
 * the unit is padded.  On success the loaded trace, the public inputs and ios_out ([num_io][words per instance]) are, word for word,
 * those of sbn_prover_generate_trace on the list of sbn_program_instances; sizes and the failure rule as there (a failing call
 * leaves NO trace loaded).  On the Fq12 tables, whose chains run on the device, the host uploads the list with the literals, ones
 * and exponents in place and the node table; one launch per level runs one workgroup per node of that level, which reads a linked
 * operand from the outputs an EARLIER launch wrote, stores its words into its own row of the list and walks the chain.  Links cross
 * kernel boundaries only: no launch reads what it stored.  The pads are filled on the device and the derived list and the outputs
 * come back in the one download of the instance outputs.  FQ_EXP (chains on the host pool) and an Fq12 prover created under
 * SBN_FQ12_HOST_CHAIN derive on the host pool and take the explicit path.  The words are the same in every placement. */
int sbn_prover_generate_trace_program(sbn_prover* p, const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values,
                                      const uint32_t* exps, size_t n_exps, uint64_t* pi_out, uint32_t* outs_out, uint32_t* ios_out);
/* Any count, as units of the batch prover's table (units as above): proofs_out[units] in unit order, word for word what
 * sbn_batch_prover_prove_ios gives on the list of sbn_program_instances, which is derived once on the host pool (so no context
 * waits for another).  Failure rule as sbn_batch_prover_prove_powers: a refused list leaves the batch prover usable and every
 * proofs_out entry null; guards apply as to every sbn_batch_prover_prove_* call. */
int sbn_batch_prover_prove_program(sbn_batch_prover* b, const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values,
                                   const uint32_t* exps, size_t n_exps, sbn_proof** proofs_out, uint32_t* outs_out, uint32_t* ios_out);
/* The twin of sbn_power_check, on the public inputs of the unit proofs (host, no device; it verifies NO proof): what a circuit
 * states with `connect` calls.  After refusals 1 to 3 and a null public_inputs (SBN_ERR_BAD_ARG) it checks, in instance order:
 * units == sbn_msm_num_units(count, num_io); x and offset of a literal node equal the caller's words (SBN_NODE_ONE: one); x or
 * offset of a linked node equals the OUTPUT public inputs of node j, across unit boundaries; the exponent is the caller's; every
 * output limb is in range (16 bits in the Fq12 tables, 32 in FQ_EXP) and every output coefficient is < p; every pad instance equals
 * instance count - 1 in x, offset, exponent and output.  SBN_OK and outs_out (optional, [count][W]) = the outputs, or
 * SBN_ERR_VERIFY_FAILED with sbn_last_error naming the first instance, the field (x, offset, exponent, output) and, for a link, the
 * node it should equal. */
int sbn_program_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units,
                      const sbn_program_node* nodes, size_t count, const uint32_t* values, size_t n_values,
                      const uint32_t* exps, size_t n_exps, uint32_t* outs_out);

/* Mapped links and the final exponentiation ---------------------------------------------------------- */
/* On the Fq12 tables a link of a field program may carry a FROBENIUS MAP: the operand is frob(output of node j, m) = (output of
 * node j)^(p^m), m in 0 .. 11.  The map is linear, so a consuming circuit computes it natively on the public inputs it connects,
 * and a program need not spend an instance with exponent p (which the u64 table cannot even state) on it.  In the flat basis of
 * the tables (the coefficient of w^k is a_k = c[k] + c[k+6] i, w^6 = xi = 9 + i) coefficient k of frob(f, m) is
 * conj^m(a_k) * G[m][k] with G[m][k] = xi^(k (p^m - 1) / 6) in Fq2 (csrc/fq12_frobenius_consts.hpp, written by
 * tools/gen_fq12_frobenius.py).  m = 0 is the identity, m = 6 the conjugate (G[6][k] = (-1)^k), and p^12 is the identity: maps
 * compose by adding mod 12.
 * The two host helpers (no device): sbn_fq12_frobenius, and sbn_fq12_inverse (f^-1 = fbar / (f fbar) with fbar the product of
 * frob(f, 1 .. 11) and one inversion in Fq).  Both refuse a null pointer, m > 11 and a coefficient >= p, and the inverse refuses
 * zero, with SBN_ERR_BAD_ARG.  in and out may be the same array. */
int sbn_fq12_frobenius(const uint32_t in[96], uint32_t m, uint32_t out[96]);
int sbn_fq12_inverse(const uint32_t in[96], uint32_t out[96]);
/* A mapped program is a field program whose nodes carry a fourth word:
 *   maps: bits 0..7 = the map of x, bits 8..15 = the map of offset, each 0 .. 11; bits 16..31 zero.
 * Each sbn_program_m_* call takes the arguments and gives the outputs of its twin above, and every statement made there holds
 * with these changes:
 *   - A node's operand with map m is frob(output of node j, m).  The explicit list holds the MAPPED words in the x / offset fields
 *     of the row; pads copy row count - 1 as before; the schedule is unchanged (a map adds no level).
 *   - With every maps == 0 each call gives, word for word, what its twin gives: list, outputs, trace, public inputs, proofs.
 *   - Refusal 3 grows: node by node, after the existing checks of that node and naming the node and the field,
 *     SBN_ERR_BAD_ARG for bits 16..31 set, then SBN_ERR_BAD_ARG for a map above 11, then SBN_ERR_BAD_ARG for a non-zero map on an
 *     operand that is no link (a literal or SBN_NODE_ONE: the caller maps a literal itself, sbn_fq12_frobenius), then, on FQ_EXP,
 *     SBN_ERR_UNSUPPORTED for any non-zero map (the map is an Fq12 notion; sbn_program_m_levels knows no table and skips this one).
 *   - sbn_program_m_check is the `connect` calls of a consuming circuit: a mapped operand must equal frob(OUTPUT public inputs of
 *     node j, m), computed natively by the check, across unit boundaries; everything else as in sbn_program_check.  A failure names
 *     the instance, the field, the node it should equal and the map ("... differs from frob_m of the output of node j").
 *   - sbn_prover_generate_trace_program_m, where the chains run on the device: in front of the launch of every level that has a
 *     mapped operand a small launch (one workgroup per mapped operand) reads the output an EARLIER level wrote, applies the map and
 *     stores the mapped words into the x / offset words of the node's own row; the level launch then loads that operand as it
 *     loads a literal.  Links still cross kernel boundaries only.  FQ_EXP and an Fq12 prover created under SBN_FQ12_HOST_CHAIN
 *     derive on the host pool.  The words are the same in every placement.
 *
 * THE FINAL EXPONENTIATION f -> f^((p^12 - 1) / r) of a BN254 pairing is 16 nodes on FQ12_EXP_U64; every exponent is 1, the BN
 * parameter x (sbn_bn_x) or one of 2, 6, 12, 18, 30, 36.  The literals are f, conj(f) = frob(f, 6) and f_inv = f^-1
 * (sbn_fq12_inverse); node n below is "output = offset * x^e", frob_m(n) a mapped link, conj = frob_6, e the easy-part result:
 *    0   f * f_inv^1                  must equal one: the check that f_inv is the inverse
 *    1   conj(f) * f_inv^1            = f^(p^6 - 1)
 *    2   frob_2(n1) * n1^1            = e = f^((p^6 - 1)(p^2 + 1)), the easy part
 *    3   1 * e^x      4   1 * n3^x      5   1 * n4^x        fx, fx2, fx3
 *    6   frob_1(e) * frob_2(e)^1      7   n6 * frob_3(e)^1  y0
 *    8   n3 * frob_1(n4)^1            fx * frob(fx2)
 *    9   n5 * frob_1(n5)^1            fx3 * frob(fx3)
 *   10   n7 * conj(e)^2
 *   11   n10 * frob_2(n4)^6
 *   12   n11 * frob_7(n3)^12          frob_7 = conj o frob_1
 *   13   n12 * conj(n8)^18
 *   14   n13 * conj(n4)^30
 *   15   n14 * conj(n9)^36            = f^((p^12 - 1) / r), the result
 * since (p^4 - p^2 + 1) / r = l0 + l1 p + l2 p^2 + p^3 with l2 = 6x^2 + 1, l1 = -36x^3 - 18x^2 - 12x + 1,
 * l0 = -36x^3 - 30x^2 - 18x - 2, and the inverse of an easy-part result is its conjugate.  One unit of Fq12ExpU64Stark(16). */
typedef struct sbn_program_node_m { uint32_t x, offset, exp, maps; } sbn_program_node_m;
#define SBN_FINAL_EXP_NODES 16
int sbn_program_m_levels(const sbn_program_node_m* nodes, size_t count, uint32_t* level_out, uint32_t* depth_out);
int sbn_program_m_instances(int32_t kind, const sbn_program_node_m* nodes, size_t count, const uint32_t* values, size_t n_values,
                            const uint32_t* exps, size_t n_exps, size_t num_io, uint32_t* ios_out, uint32_t* outs_out);
int sbn_prover_generate_trace_program_m(sbn_prover* p, const sbn_program_node_m* nodes, size_t count, const uint32_t* values, size_t n_values,
                                        const uint32_t* exps, size_t n_exps, uint64_t* pi_out, uint32_t* outs_out, uint32_t* ios_out);
int sbn_batch_prover_prove_program_m(sbn_batch_prover* b, const sbn_program_node_m* nodes, size_t count, const uint32_t* values, size_t n_values,
                                     const uint32_t* exps, size_t n_exps, sbn_proof** proofs_out, uint32_t* outs_out, uint32_t* ios_out);
int sbn_program_m_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units,
                        const sbn_program_node_m* nodes, size_t count, const uint32_t* values, size_t n_values,
                        const uint32_t* exps, size_t n_exps, uint32_t* outs_out);

/* Curve programs ------------------------------------------------------------------------------------- */
/* What the field programs above are to the field tables, on the curve tables G1_EXP and G2_EXP (an instance is output = offset +
 * e x): a program is a list of instances whose x and offset are each a literal point or the OUTPUT of an earlier instance.  A
 * curve output is no bare product: it carries the start it was accumulated from, so an output used as x drags a multiple of the
 * start along.  The library does the bookkeeping: beside every output it keeps the BLIND the output carries, a function of the
 * start, the exponents and the shape of the program alone, and hands back the VALUE output + (-blind) the caller means.  With it
 * the tables state a multiple of a result, e2 (e1 P) (the subgroup check r (h P) = O of a point just cleared of its cofactor, a
 * scalar applied to the sum of an MSM), a combination a S1 + b S2 of two earlier results (the random linear combination of a batch
 * verification, C - y G of a KZG opening, the merge of MSM segments derived side by side) and any DAG of such sums.
 * One definition for every entry point below.  E = 1 (G1_EXP) or 2 (G2_EXP), W = 16E u32 words per point (x.c0 [x.c1] y.c0 [y.c1],
 * eight words each, as in `ios`):
 *   nodes  [count] sbn_program_node: node g is instance g of the list.  x is an index into `points` or SBN_NODE_OUTPUT | j, j < g;
 *          offset is an index into `points`, SBN_NODE_OUTPUT | j, or SBN_NODE_START, the start the library picks; exp is an index
 *          into `exps`.  SBN_NODE_ONE is illegal in both fields.
 *   points [n_points][W] u32, exps [n_exps][8] u32: 256-bit exponents, used as they are, never reduced.
 * out_g = offset_g + e_g x_g as points, and every output is carried as out_g = v_g + T_g, the value and the blind:
 *     operand               v      T
 *     literal point P       P      O
 *     SBN_NODE_START        O      S
 *     SBN_NODE_OUTPUT | j   v_j    T_j
 *   v_g = v_off + e_g v_x,  T_g = T_off + e_g T_x.  A value may be the point at infinity; a node with no SBN_NODE_START anywhere
 *   under it has T = O and value = out.
 * S = sbn_start_candidate(kind, choice) with ONE choice for the whole program (a blind is a function of S, so two starts in one
 * program would need a blind per start and node): the smallest j < SBN_START_CANDIDATES for which no node has a bad event of the
 * complete sums -- an offset or an output at infinity, or an addition of the table's walk with B = +-A.  The events at a node
 * whose operands hold no start are the caller's: no candidate mends them.
 * Returned (every output pointer optional): *choice_out; outs_out [count][W], the table outputs; values_out [count][W] with
 * infinity_out [count] bytes, values[g] = out_g + (-T_g) by the complete addition (a value at infinity is no error: flag 1, words
 * zero); ios_out [units * num_io][2W + 8], the explicit list with every link resolved, units = sbn_msm_num_units(count, num_io),
 * rows >= count copies of row count - 1.  Links may cross units.
 * Refused, in this order:
 *   1. SBN_ERR_UNSUPPORTED for any kind but G1_EXP / G2_EXP;
 *   2. SBN_ERR_BAD_ARG for a null nodes, points or exps, count = 0 or num_io = 0, and count, n_points or n_exps of 2^31 - 1 or more;
 *   3. node by node, naming the node and the field, SBN_ERR_BAD_ARG for a link with j >= g, then a literal index >= n_points, then
 *      SBN_NODE_ONE, then SBN_NODE_START as x, then an exponent index >= n_exps;
 *   4. for the literals THAT SOME NODE USES, in index order: SBN_ERR_BAD_ARG for a coordinate >= p, then (again in index order) for
 *      a point off the table's curve.  An unused literal is not read;
 *   5. SBN_ERR_WITNESS when all eight candidates fail, naming the first node at which candidate 7 failed and, when that node holds
 *      no start, that no candidate can mend it. */
#define SBN_NODE_START 0x7ffffffeu  /* offset only (curve programs): the start the library picks */
/* The derivation on the host pool, no device: level by level (sbn_program_levels), the nodes of a level side by side, the blinds
 * beside the outputs; candidate 0 first, after a bad event the whole program again from the next candidate; then the table's own
 * walk of the list.  num_io is not checked against any table. */
int sbn_curve_program_instances(int32_t kind, const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points,
                                const uint32_t* exps, size_t n_exps, size_t num_io, uint32_t* ios_out, uint32_t* outs_out,
                                uint32_t* values_out, uint8_t* infinity_out, uint8_t* choice_out);
/* One unit on a prover of the table: count <= the table's num_io (SBN_ERR_BAD_ARG otherwise, after refusals 1 and 2), the rest of
 * the unit is padded.  On success the loaded trace, the public inputs and ios_out ([num_io][2W + 8]) are, word for word, those of
 * sbn_prover_generate_trace on the list of sbn_curve_program_instances; a failing call leaves NO trace loaded.  Where the table's
 * chains run on the device (SBN_TRACEGEN_DEVICE_CHAIN = 1 or 2) the links are resolved there from candidate 0: one launch per level
 * walks the chains of that level's nodes (one lane or one wave per node), reading a linked operand from the affine outputs an
 * EARLIER launch left, and a status kernel behind it writes those affine outputs and ONE status word when a node of the level has
 * a bad event.  The host derives the blinds meanwhile, reads the word after the last level and uploads the negated blinds; the
 * values are computed on the device and come back with the outputs and the derived list.  A bad event sends the call to the host
 * derivation, which walks the candidates, and to the explicit path; so does placement 0.  The words are the same in every placement. */
int sbn_prover_generate_trace_curve_program(sbn_prover* p, const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points,
                                            const uint32_t* exps, size_t n_exps, uint64_t* pi_out, uint32_t* outs_out, uint32_t* values_out,
                                            uint8_t* infinity_out, uint8_t* choice_out, uint32_t* ios_out);
/* Any count, as units of the batch prover's table: proofs_out[units] in unit order, word for word what sbn_batch_prover_prove_ios
 * gives on the list of sbn_curve_program_instances, which is derived once on the host pool.  Failure rule and guards as
 * sbn_batch_prover_prove_program. */
int sbn_batch_prover_prove_curve_program(sbn_batch_prover* b, const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points,
                                         const uint32_t* exps, size_t n_exps, sbn_proof** proofs_out, uint32_t* outs_out, uint32_t* values_out,
                                         uint8_t* infinity_out, uint8_t* choice_out, uint32_t* ios_out);
/* The check on the public inputs of the unit proofs (host, no device; it verifies NO proof).  After refusals 1 to 3, a null
 * public_inputs and choice >= SBN_START_CANDIDATES (SBN_ERR_BAD_ARG) it checks units == sbn_msm_num_units(count, num_io) and then,
 * in instance order: x and offset of a literal operand equal the caller's words; an SBN_NODE_START offset equals candidate
 * `choice`; a linked x or offset equals the OUTPUT public inputs of node j, across unit boundaries; the exponent is the caller's;
 * every output limb is in range, every output coordinate < p and every output a point of the curve; every pad instance equals
 * instance count - 1.  Then the blinds are recomputed from `choice` and the exponents alone: outs_out (optional) = the outputs,
 * values_out / infinity_out (optional) = out + (-T).  SBN_ERR_VERIFY_FAILED with sbn_last_error naming the first instance, the field
 * (x, offset, exponent, output) and, for a link, the node it should equal. */
int sbn_curve_program_check(int32_t kind, size_t num_io, const uint64_t* const* public_inputs, size_t units,
                            const sbn_program_node* nodes, size_t count, const uint32_t* points, size_t n_points,
                            const uint32_t* exps, size_t n_exps, uint32_t choice, uint32_t* outs_out, uint32_t* values_out,
                            uint8_t* infinity_out);

/* One oversized trace split over the GPUs of a node (BASELINE config "Single Fq12 exponentiation proof, trace height
 * 2^18, 8xMI355X with RCCL FRI fold"; reference workload src/fields/fq12/exp.rs:638-696).  One rank per GPU (one process
 * each, or the threads of one process with sbn_local_comm_create); every rank calls the same functions with the same
 * arguments and receives the same proof.  Work and the derived matrices (coefficients, LDE, Z, Merkle trees) are sharded:
 * COLUMNS for iNTT / LDE / Z / openings / the FRI batch combination, dealt round-robin in blocks of 64 (rank r owns the
 * column blocks r, r + world, ...); LDE ROWS for leaf hashing, Merkle subtrees, constraint evaluation and query answers
 * (rank s owns the rows whose Merkle leaf index has top log2(world) bits = s: complete cap subtrees).  The trace VALUES
 * are resident on every rank (generated there by sbn_split_prover_generate_trace, or loaded).  Exchange steps: one
 * all-to-all per column block and plane (columns -> rows), pipelined -- while block k travels, block k + 1 is transformed
 * and the blocks k - 1 of all ranks are absorbed by the leaf sponge -- and small all-gathers (caps, quotient values,
 * openings, FRI partial sums, query rows).  The collectives come with the sbn_comm: the transports of this library
 * (sbn_rccl_comm_create: RCCL send / recv over xGMI; sbn_local_comm_create: the ranks are threads of one process), or the
 * caller's own (torch.distributed in starky_bn254_amd/split.py; a host-staged backend for tests).
 * world must be 1, 2, 4, 8 or 16 (<= 2^cap_height).
 * rate_bits = 1 only: with rate_bits > 1 sbn_split_exchange_bytes and sbn_split_prover_create return SBN_ERR_UNSUPPORTED for every
 * world, 1 included (the exchange plans deal the rows of a 2n-point LDE, which is then also the quotient's domain). */
typedef struct sbn_comm {
  uint32_t struct_size;      /* sizeof(sbn_comm) of the caller's header (ABI check) */
  uint32_t reserved;
  void* ctx;                 /* passed back to the callbacks */
  uint32_t rank, world;
  void* send_buf;            /* device memory, >= send_bytes of sbn_split_exchange_bytes */
  void* recv_buf;            /* device memory, >= recv_bytes; holds this rank's row-sharded LDE matrices during a proof */
  uint64_t send_bytes, recv_bytes;
  /* Block d = send_buf[send_off[d] .. +send_len[d]) goes to rank d; the block from rank s lands at
   * recv_buf[recv_off[s] .. +recv_len[s]).  Arrays of `world` entries, bytes; zero-length blocks are skipped (rank d's
   * recv_len[s] equals rank s's send_len[d]); blocks sent to different ranks may be the same region (an all-gather); a
   * rank may send a block to itself.  STREAM-ORDERED: `stream` is a hipStream_t of the device that owns the buffers; the
   * send blocks are read after everything enqueued on it before the call, and work enqueued on it after the call sees
   * the received blocks complete and may overwrite the send blocks.  The call itself may return early (RCCL) or block
   * (a host-staged transport synchronises the stream itself).  The arrays are only valid during the call.  0 = ok. */
  int (*all_to_all)(void* ctx, void* stream, const uint64_t* send_off, const uint64_t* send_len, const uint64_t* recv_off, const uint64_t* recv_len);
  /* Host memory, blocking: every rank contributes `bytes` at send; recv = [world][bytes] in rank order. */
  int (*all_gather_host)(void* ctx, const void* send, void* recv, uint64_t bytes);
} sbn_comm;
typedef struct sbn_split_prover sbn_split_prover;
/* Staging sizes a rank needs for (air, degree_bits) in a world of `world` ranks. */
int sbn_split_exchange_bytes(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, uint32_t world, uint64_t* send_bytes, uint64_t* recv_bytes);
int sbn_split_prover_create(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, const sbn_comm* comm, sbn_split_prover** out);
void sbn_split_prover_destroy(sbn_split_prover* p);
/* As sbn_prover_generate_trace / sbn_prover_load_trace: the full trace values on this rank. */
int sbn_split_prover_generate_trace(sbn_split_prover* p, const uint32_t* ios, size_t num_io, uint64_t* pi_out);
int sbn_split_prover_load_trace(sbn_split_prover* p, const uint64_t* trace_col_major, const uint64_t* public_inputs, size_t n_pi);
/* The proof of the whole trace, on every rank, word for word the proof sbn_prover_prove gives on one GPU. */
int sbn_split_prover_prove(sbn_split_prover* p, sbn_proof** out);
int sbn_split_prover_stage_times(const sbn_split_prover* p, float* ms_out, int cap);
/* sbn_prover_set_guard on this rank's context: a null handle or an unknown mode SBN_ERR_BAD_ARG, otherwise SBN_ERR_UNSUPPORTED for
 * every mode and every world size, 1 included (verify what sbn_split_prover_prove returns with sbn_verify or a sbn_verifier). */
int sbn_split_prover_set_guard(sbn_split_prover* p, uint32_t mode);
/* sbn_prover_check_trace on this rank's loaded trace, world = 1 only: with more ranks the Z columns and the rows are shared out
 * and this returns SBN_ERR_UNSUPPORTED (every rank holds the whole trace: check it with sbn_check_trace_host or on a single-GPU
 * prover). */
int sbn_split_prover_check_trace(sbn_split_prover* p, uint64_t seed, sbn_trace_report* report, uint8_t* row_flags_out);
/* sbn_prover_explain_rows / sbn_prover_explain_trace on this rank's loaded trace, world = 1 only, as the check. */
int sbn_split_prover_explain_rows(sbn_split_prover* p, uint64_t seed, const uint64_t* rows, size_t n_rows, uint8_t* block_flags_out, uint8_t* z_flags_out);
int sbn_split_prover_explain_trace(sbn_split_prover* p, uint64_t seed, sbn_block_stat* block_stats_out, sbn_block_stat* z_stats_out);

/* Transports that fill an sbn_comm: starky_bn254_amd/csrc/transport.hip ---------------------- */
/* RCCL over xGMI, one process per GPU, no Python: librccl is loaded at run time (SBN_RCCL_LIB overrides the name), so the
 * library itself has no link-time dependency on it.  Rank 0 calls sbn_rccl_unique_id and hands the 128 bytes to the other
 * ranks by whatever means the caller has (a file, a socket, MPI); then every rank calls sbn_rccl_comm_create with the
 * staging sizes of sbn_split_exchange_bytes (the transport allocates send_buf / recv_buf on the current device).
 * all_to_all = ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd on the given stream; all_gather_host = ncclAllGather on
 * a small device buffer + copies. */
int sbn_rccl_unique_id(uint8_t id_out[128]);
int sbn_rccl_comm_create(const uint8_t id[128], uint32_t rank, uint32_t world, uint64_t send_bytes, uint64_t recv_bytes, sbn_comm* out);
void sbn_rccl_comm_destroy(sbn_comm* comm);
/* The ranks are threads of ONE process: rank r on devices[r] (null: all ranks on the current device -- how the parity tests
 * run 8 and 16 ranks on a one-GPU box).  Blocks are pulled with stream-ordered device-to-device copies (peer copies over
 * xGMI between different devices); the ranks meet at host barriers, so every rank must be inside the same library call
 * on its own thread.  A failing rank calls sbn_local_comm_abort, which releases the others with an error. */
typedef struct sbn_local_group sbn_local_group;
int sbn_local_comm_create(uint32_t world, const int* devices, uint64_t send_bytes, uint64_t recv_bytes, sbn_comm* comms_out, sbn_local_group** out);
void sbn_local_comm_abort(sbn_local_group* g);
void sbn_local_comm_destroy(sbn_local_group* g);
/* A pattern exchange through `comm` (uneven blocks, self blocks, an all-gather, the host all-gather), checked on the
 * device: every rank calls it (with the device of its staging buffers current); 0 = the transport moved every byte where it
 * belongs. */
int sbn_comm_selftest(const sbn_comm* comm);

/* Proof object ---------------------------------------------------------------------------------- */
size_t sbn_proof_num_words(const sbn_proof* proof);
const uint64_t* sbn_proof_words(const sbn_proof* proof);
/* Writes the canonical LE byte stream; returns bytes needed (call with cap=0 to size). */
size_t sbn_proof_serialize(const sbn_proof* proof, uint8_t* buf, size_t cap);
uint32_t sbn_proof_degree_bits(const sbn_proof* proof); /* StarkProof::recover_degree_bits, exp.rs:829 */
void sbn_proof_free(sbn_proof* proof);

/* Verifier: verify_stark_proof(stark, proof, &config) (src/curves/g1/exp.rs:826). */
int sbn_verify(const sbn_air_desc* air, const sbn_config* cfg, const uint8_t* proof_bytes, size_t len);

/* Batch verifier: the same verification with the Merkle hashing and the reduction of the opened rows on the device, for up to
 * max_batch proofs of one (table, config, degree_bits) per call (csrc/verifier_device.hip).  It frees host cores; whether it is
 * also faster than sbn_verify on as many host threads as the caller has is recorded in DESIGN.md section 7.
 * config_supported() and the table / degree_bits checks run before a device is looked for (as sbn_prover_create);
 * 1 <= max_batch <= 65536; no device: SBN_ERR_NO_DEVICE (no fallback: sbn_verify is the host verifier).  The verifier owns
 * max_batch proof-sized slots of device memory, a stream and 16 MiB of pinned staging; the caller's memory is only read. */
typedef struct sbn_verifier sbn_verifier;
int sbn_verifier_create(const sbn_air_desc* air, const sbn_config* cfg, uint32_t degree_bits, uint32_t max_batch, sbn_verifier** out);
/* 1 <= count <= max_batch.  Returns SBN_OK when the call ran; status_out[i] is what sbn_verify(air, cfg, proofs[i], lens[i])
 * returns, and sbn_verifier_reason(v, i) is the message sbn_last_error() would hold after it ("" when accepted), until the
 * next call.  A call-level failure (null argument, count out of range: SBN_ERR_BAD_ARG; a HIP failure: SBN_ERR_HIP) leaves
 * status_out untouched.  A proof that names another degree_bits than the verifier's gets its verdict from the host path.
 * One thread at a time per verifier. */
int sbn_verifier_verify(sbn_verifier* v, const uint8_t* const* proofs, const size_t* lens, size_t count, int32_t* status_out);
const char* sbn_verifier_reason(const sbn_verifier* v, size_t i);
/* Device times of the last call (ms, HIP events on the verifier's stream): upload, kernels, download; returns the number written. */
int sbn_verifier_stage_times(const sbn_verifier* v, float* ms_out, int cap);
void sbn_verifier_destroy(sbn_verifier* v);

/* Building blocks exposed for parity tests and benchmarks (device in/out unless noted) --------- */
/* PolynomialBatch::from_values on a host column-major matrix: Merkle cap (2^cap_height x 4 words),
 * optionally coefficients [ncols][n] and LDE [ncols][n<<rate_bits] (natural order) back to host.
 * rate_bits 1..3 with n << rate_bits <= 2^23, n a power of two >= 512, cap_height 1..8 (the range of sbn_config); otherwise
 * SBN_ERR_UNSUPPORTED.  Runs the transform plan and the kernels a prover of n rows and this rate_bits runs. */
int sbn_commit_values(const uint64_t* cols, size_t ncols, size_t n, uint32_t rate_bits, uint32_t cap_height,
                      uint64_t* cap_out, uint64_t* coeffs_out, uint64_t* lde_out);
/* The twin of sbn_commit_values for SBN_LDE_COMPACT: rows of the coset LDE at rate_bits, computed from the values by the compact
 * mode's own kernels (values -> coefficients through the transform plan of a prover of this height, then the evaluation at the
 * opened points).  leaf_indices[k] < 2^(degree_bits + rate_bits) is a Merkle leaf index, i.e. LDE row bitrev(leaf index), as the
 * query indices of a proof are (SBN_ERR_BAD_ARG beyond); 1 <= count <= 65536 (SBN_ERR_BAD_ARG otherwise); rows_out: [count][ncols].  rate_bits 1..3, degree_bits >= 9,
 * degree_bits + rate_bits <= 23, otherwise SBN_ERR_UNSUPPORTED.  Host in/out. */
int sbn_lde_rows(const uint64_t* values_col_major, size_t ncols, uint32_t degree_bits, uint32_t rate_bits, const uint32_t* leaf_indices, size_t count,
                 uint64_t* rows_out);
/* Poseidon permutation of `count` independent width-12 states on the device (host in/out). */
int sbn_poseidon_permute_batch(uint64_t* states, size_t count);
/* The same permutation through the 16-lane cooperative form that the narrow Merkle levels, the FRI leaves and the device verifier
 * run (csrc/poseidon.cuh poseidon_permute_coop16): one group of 16 lanes per state, `count` passed to the kernel as it is, so counts
 * that are no multiple of 4 (groups per wave) or 16 (groups per workgroup) run partly filled waves and workgroups.  A null pointer
 * (SBN_ERR_BAD_ARG) and a word >= p (SBN_ERR_NON_CANONICAL) are refused before a device is looked for.  Host in/out. */
int sbn_poseidon_permute_coop_batch(uint64_t* states, size_t count);
/* out[i] = a[i] * b[i] in the Goldilocks field with the DEVICE multiply of every kernel (csrc/gl.cuh: 13-instruction weak product +
 * canonicalisation; mode 0), or the weak product of the transform passes canonicalised afterwards (mode 1).  a, b: any 64-bit
 * values (non-canonical representatives included: the kernels' intermediate values are); out canonical.  Host in/out. */
int sbn_field_mul_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, int mode);
/* The BN254 base-field helpers of the witness generators (csrc/bn254w.cuh, csrc/kernels_tracegen.cuh) on `count` elements of four
 * little-endian u64 words in standard form.  op 0: a*b through the Montgomery product (to_m, mmul, from_m); 1: a+b; 2: a-b;
 * 3: a^-1 (device: Fermat, host: binary extended GCD); 4: a^-1 by Montgomery's trick over consecutive groups of 8 (count % 8 == 0);
 * 5: (c0 + c1 i)^-1 in Fq2 through the norm, c0 from a and c1 from b, out [count][2][4].  on_device = 0 runs the host build of
 * the same functions (no device needed).  SBN_ERR_NON_CANONICAL for an input >= p, SBN_ERR_BAD_ARG for a zero to invert.
 * Parity tests only; host in/out. */
int sbn_bn254_fq_batch(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, int on_device);
/* Index of the first word >= p (the Goldilocks modulus) among words[0 .. count), or count when every word is canonical: the scan
 * sbn_prover_prove_host_trace runs behind each chunk it uploads (csrc/kernels_load.cuh first_non_canonical_kernel), host in/out.
 * on_device = 0 runs a host loop and needs no device. */
int sbn_first_non_canonical(const uint64_t* words, size_t count, int on_device, uint64_t* index_out);
/* out[0 .. len) = the flat words [word0, word0 + len) of the column-major matrix [n_columns][n] whose column c is
 * columns[c][0 .. n): the copy sbn_prover_prove_host_columns makes into each piece of its upload ring (csrc/host_columns.hpp).
 * SBN_ERR_BAD_ARG when word0 + len > n_columns * n or a column pointer is null or not 8-byte aligned.  Host only. */
int sbn_gather_columns(const uint64_t* const* columns, size_t n_columns, size_t n, size_t word0, size_t len, uint64_t* out);
/* In place: every word >= p becomes w - p; *reduced_out (optional) = the number of words changed.  The kernel
 * SBN_TRACE_REDUCE runs behind each chunk it uploads (csrc/kernels_load.cuh reduce_words_kernel), host in/out; on_device = 0 runs a
 * host loop and needs no device. */
int sbn_reduce_words(uint64_t* words, size_t count, int on_device, uint64_t* reduced_out);
/* The host permutation behind the Fiat-Shamir transcript of prove()/verify() (plonky2 Challenger's
 * PoseidonPermutation): sparse partial rounds, or the plain definition when use_definition != 0.  Host only. */
int sbn_poseidon_permute_host(uint64_t* states, size_t count, int use_definition);
/* The table's AIR constraints (eval_packed_generic of the table, e.g. src/curves/g1/exp.rs:331-495; no permutation checks)
 * folded into the num_challenges = 2 accumulators acc_j = sum_t c_t alpha_j^(n-1-t) on ONE row pair over the base field:
 * the regrouped evaluator the quotient kernel runs, on the host.  local_row / next_row: [num_columns]; z_last = x - g^-1,
 * l_first / l_last = the Lagrange selectors at the point (starky ConstraintConsumer).  Host only. */
int sbn_eval_constraints_host(const sbn_air_desc* air, const uint64_t* local_row, const uint64_t* next_row, const uint64_t* public_inputs,
                              size_t n_pi, const uint64_t* alphas, uint64_t z_last, uint64_t l_first, uint64_t l_last, uint64_t* acc_out);

#ifdef __cplusplus
}
#endif
#endif /* SBN_H */
