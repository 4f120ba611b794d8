//! Raw declarations of include/sbn.h (one line per entry point the shim uses).
#![allow(non_camel_case_types)]
use std::os::raw::c_char;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct sbn_air_desc {
    pub kind: i32,
    pub num_io: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct sbn_config {
    pub security_bits: u32,
    pub num_challenges: u32,
    pub rate_bits: u32,
    pub cap_height: u32,
    pub proof_of_work_bits: u32,
    pub fri_arity_bits: u32,
    pub fri_final_poly_bits: u32,
    pub num_query_rounds: u32,
    /// sbn_fri_variant: 0 = default (= 1), 1 = plonky2 0.1.x FRI (final polynomial multiplied by X, PR #436), 2 = later upstream
    pub fri_variant: u32,
}

/// sbn_prover_options.lde_storage
pub const SBN_LDE_FULL: u32 = 0;
pub const SBN_LDE_COMPACT: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct sbn_prover_options {
    pub struct_size: u32,
    pub lde_storage: u32,
}

/// include/sbn.h `sbn_program_node` ("Field programs"): x / offset an index into `values`, or `SBN_NODE_OUTPUT | j` for the output of
/// node j (j below the node's own index); offset may be `SBN_NODE_ONE`; exp an index into `exps`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct sbn_program_node {
    pub x: u32,
    pub offset: u32,
    pub exp: u32,
}
pub const SBN_NODE_OUTPUT: u32 = 0x8000_0000;
pub const SBN_NODE_ONE: u32 = 0x7fff_ffff;
/// include/sbn.h "Curve programs": offset only, the start the library picks (one per program)
pub const SBN_NODE_START: u32 = 0x7fff_fffe;

/// the modes of sbn_prover_set_guard / sbn_batch_prover_set_guard / sbn_prove_set_guard
pub const SBN_GUARD_OFF: u32 = 0;
pub const SBN_GUARD_DEVICE: u32 = 1;
pub const SBN_GUARD_HOST: u32 = 2;

#[repr(C)]
pub struct sbn_prover {
    _opaque: [u8; 0],
}
#[repr(C)]
pub struct sbn_proof {
    _opaque: [u8; 0],
}
#[repr(C)]
pub struct sbn_batch_prover {
    _opaque: [u8; 0],
}
#[repr(C)]
pub struct sbn_verifier {
    _opaque: [u8; 0],
}

/// include/sbn.h `sbn_trace_report`: what sbn_prover_check_trace found, by segment (0 = AIR head, 1 = AIR tail of the Exp tables,
/// 2 / 3 = the permutation checks of the Z columns below / from `z_split`); `u64::MAX` = no such row.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct sbn_trace_report {
    pub struct_size: u32,
    pub num_segments: u32,
    pub rows: u64,
    pub failing_rows: u64,
    pub first_failing_row: u64,
    pub seg_failing_rows: [u64; 4],
    pub seg_first_row: [u64; 4],
    pub num_zs: u32,
    pub z_split: u32,
}

/// include/sbn.h `sbn_constraint_block`: one emission of the regrouped evaluator, constraints `[first, first + count)` of the AIR stream.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct sbn_constraint_block {
    pub first: u32,
    pub count: u32,
    pub segment: u32,
    pub section: u32,
    pub instance: u32,
    pub col_first: u32,
    pub col_count: u32,
}

/// include/sbn.h `sbn_block_stat`: rows on which a block (or a Z column) is non-zero, and the first of them (`u64::MAX`: none).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct sbn_block_stat {
    pub failing_rows: u64,
    pub first_row: u64,
}

/// include/sbn.h `sbn_witness_diff`: the loaded trace against the canonical witness of its instance list (`u64::MAX` = none).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct sbn_witness_diff {
    pub struct_size: u32,
    pub reserved: u32,
    pub cells: u64,
    pub main_cells: u64,
    pub rows: u64,
    pub columns: u64,
    pub first_row: u64,
    pub first_column: u64,
    pub listed: u64,
    pub pi_words: u64,
    pub first_pi_word: u64,
}

/// include/sbn.h `sbn_witness_cell`: one differing cell, the loaded word and the canonical one.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct sbn_witness_cell {
    pub row: u64,
    pub column: u64,
    pub got: u64,
    pub want: u64,
}

pub const SBN_AIR_G1_OP: i32 = 1;
pub const SBN_AIR_G1_EXP: i32 = 2;
pub const SBN_AIR_G2_EXP: i32 = 3;
pub const SBN_AIR_FQ12_EXP: i32 = 4;
pub const SBN_AIR_FQ_EXP: i32 = 5;
pub const SBN_AIR_FQ12_EXP_U64: i32 = 6;
/// the reference's single-operation test tables (`ModularStark`, `Fq12Stark`)
pub const SBN_AIR_MODULAR: i32 = 7;
pub const SBN_AIR_FQ12_MUL: i32 = 8;
/// the reference's unit-test tables `MyStark` (lookup.rs) and `FlagStark` (flags.rs)
pub const SBN_AIR_LOOKUP: i32 = 9;
pub const SBN_AIR_FLAGS: i32 = 10;
pub const SBN_AIR_FLAGS_U64: i32 = 11;

extern "C" {
    pub fn sbn_abi_version() -> i32;
    pub fn sbn_last_error() -> *const c_char;
    pub fn sbn_set_device(device: i32) -> i32;
    pub fn sbn_set_thread_device(device: i32) -> i32;
    pub fn sbn_device_count() -> i32;
    pub fn sbn_standard_fast_config(out: *mut sbn_config);
    /// standard_fast_config at another blowup and the same conjectured security: 84 / 42 / 28 queries at rate_bits 1 / 2 / 3
    pub fn sbn_config_for_rate(rate_bits: u32, out: *mut sbn_config);
    pub fn sbn_air_num_columns(air: *const sbn_air_desc) -> usize;
    pub fn sbn_air_num_public_inputs(air: *const sbn_air_desc) -> usize;

    pub fn sbn_prover_create(air: *const sbn_air_desc, cfg: *const sbn_config, degree_bits: u32, out: *mut *mut sbn_prover) -> i32;
    pub fn sbn_prover_create_with(air: *const sbn_air_desc, cfg: *const sbn_config, degree_bits: u32, opt: *const sbn_prover_options, out: *mut *mut sbn_prover) -> i32;
    pub fn sbn_prover_memory_plan(air: *const sbn_air_desc, cfg: *const sbn_config, degree_bits: u32, opt: *const sbn_prover_options, bytes_out: *mut u64) -> i32;
    pub fn sbn_prover_destroy(p: *mut sbn_prover);
    pub fn sbn_prover_load_trace(p: *mut sbn_prover, trace_col_major: *const u64, public_inputs: *const u64, n_pi: usize) -> i32;
    pub fn sbn_prover_generate_trace(p: *mut sbn_prover, ios: *const u32, num_io: usize, pi_out: *mut u64) -> i32;
    pub fn sbn_chain_instances(kind: i32, terms: *const u32, count: usize, start: *const u32, ios_out: *mut u32, final_out: *mut u32) -> i32;
    pub fn sbn_prover_generate_trace_chained(p: *mut sbn_prover, terms: *const u32, num_io: usize, start: *const u32, pi_out: *mut u64, ios_out: *mut u32) -> i32;
    pub fn sbn_prover_prove(p: *mut sbn_prover, out: *mut *mut sbn_proof) -> i32;
    pub fn sbn_prover_prove_host_trace(p: *mut sbn_prover, trace_col_major: *const u64, public_inputs: *const u64, n_pi: usize, out: *mut *mut sbn_proof) -> i32;
    pub fn sbn_prover_prove_host_columns(p: *mut sbn_prover, columns: *const *const u64, n_columns: usize, flags: u32, public_inputs: *const u64, n_pi: usize, reduced_out: *mut u64, out: *mut *mut sbn_proof) -> i32;
    pub fn sbn_prove_columns(air: *const sbn_air_desc, cfg: *const sbn_config, columns: *const *const u64, n_columns: usize, degree_bits: u32, flags: u32, public_inputs: *const u64, n_pi: usize, out: *mut *mut sbn_proof) -> i32;
    pub fn sbn_batch_prover_prove_host_columns(b: *mut sbn_batch_prover, columns: *const *const u64, n_columns: usize, flags: u32, public_inputs: *const *const u64, n_pi: usize, count: usize, proofs_out: *mut *mut sbn_proof) -> i32;
    pub fn sbn_gather_columns(columns: *const *const u64, n_columns: usize, n: usize, word0: usize, len: usize, out: *mut u64) -> i32;
    pub fn sbn_reduce_words(words: *mut u64, count: usize, on_device: i32, reduced_out: *mut u64) -> i32;
    pub fn sbn_prove_cache_configure(budget_bytes: u64) -> i32;
    pub fn sbn_prove_cache_stats(out: *mut u64) -> i32;
    pub fn sbn_first_non_canonical(words: *const u64, count: usize, on_device: i32, index_out: *mut u64) -> i32;
    pub fn sbn_prover_check_trace(p: *mut sbn_prover, seed: u64, report: *mut sbn_trace_report, row_flags_out: *mut u8) -> i32;
    pub fn sbn_trace_segment_name(s: i32) -> *const c_char;
    pub fn sbn_air_num_permutation_zs(air: *const sbn_air_desc, cfg: *const sbn_config) -> usize;
    pub fn sbn_air_constraint_blocks(air: *const sbn_air_desc, out: *mut sbn_constraint_block, cap: usize) -> usize;
    pub fn sbn_constraint_section_name(section: i32) -> *const c_char;
    pub fn sbn_air_permutation_pair(air: *const sbn_air_desc, z: usize, lhs_col: *mut u32, rhs_col: *mut u32) -> i32;
    pub fn sbn_explain_rows_host(air: *const sbn_air_desc, trace_col_major: *const u64, degree_bits: u32, public_inputs: *const u64, n_pi: usize, seed: u64, rows: *const u64, n_rows: usize, block_flags_out: *mut u8, z_flags_out: *mut u8) -> i32;
    pub fn sbn_explain_trace_host(air: *const sbn_air_desc, trace_col_major: *const u64, degree_bits: u32, public_inputs: *const u64, n_pi: usize, seed: u64, block_stats_out: *mut sbn_block_stat, z_stats_out: *mut sbn_block_stat) -> i32;
    pub fn sbn_prover_explain_rows(p: *mut sbn_prover, seed: u64, rows: *const u64, n_rows: usize, block_flags_out: *mut u8, z_flags_out: *mut u8) -> i32;
    pub fn sbn_prover_explain_trace(p: *mut sbn_prover, seed: u64, block_stats_out: *mut sbn_block_stat, z_stats_out: *mut sbn_block_stat) -> i32;
    pub fn sbn_prover_explain_times(p: *const sbn_prover, ms_out: *mut f32, cap: i32) -> i32;
    pub fn sbn_instances_from_public_inputs(kind: i32, public_inputs: *const u64, n_pi: usize, num_io: usize, ios_out: *mut u32, outputs_out: *mut u32) -> i32;
    pub fn sbn_prover_diff_witness(p: *mut sbn_prover, ios: *const u32, num_io: usize, report: *mut sbn_witness_diff, column_cells_out: *mut u64, column_first_row_out: *mut u64, cells_out: *mut sbn_witness_cell, cells_cap: usize) -> i32;
    pub fn sbn_prover_diff_witness_times(p: *const sbn_prover, ms_out: *mut f32, cap: i32) -> i32;
    pub fn sbn_diff_witness_host(air: *const sbn_air_desc, trace_col_major: *const u64, degree_bits: u32, public_inputs: *const u64, n_pi: usize, ios: *const u32, num_io: usize, report: *mut sbn_witness_diff, column_cells_out: *mut u64, column_first_row_out: *mut u64, cells_out: *mut sbn_witness_cell, cells_cap: usize) -> i32;
    pub fn sbn_prover_stage_times(p: *const sbn_prover, ms_out: *mut f32, cap: i32) -> i32;
    pub fn sbn_prover_stage_name(i: i32) -> *const c_char;
    pub fn sbn_prover_describe(p: *const sbn_prover, out: *mut c_char, cap: usize) -> i32;
    pub fn sbn_settings_check(out: *mut c_char, cap: usize) -> i32;

    pub fn sbn_batch_prover_create(air: *const sbn_air_desc, cfg: *const sbn_config, degree_bits: u32, inflight: u32, out: *mut *mut sbn_batch_prover) -> i32;
    pub fn sbn_batch_prover_create_with(air: *const sbn_air_desc, cfg: *const sbn_config, degree_bits: u32, inflight: u32, opt: *const sbn_prover_options, out: *mut *mut sbn_batch_prover) -> i32;
    pub fn sbn_lde_rows(values_col_major: *const u64, ncols: usize, degree_bits: u32, rate_bits: u32, leaf_indices: *const u32, count: usize, rows_out: *mut u64) -> i32;
    pub fn sbn_batch_prover_prove_ios(b: *mut sbn_batch_prover, ios: *const u32, ios_words_per_unit: usize, num_io: usize, count: usize, proofs_out: *mut *mut sbn_proof) -> i32;
    pub fn sbn_batch_prover_destroy(b: *mut sbn_batch_prover);
    /// verified proving (include/sbn.h): mode = SBN_GUARD_OFF / SBN_GUARD_DEVICE / SBN_GUARD_HOST
    pub fn sbn_prover_set_guard(p: *mut sbn_prover, mode: u32) -> i32;
    pub fn sbn_batch_prover_set_guard(b: *mut sbn_batch_prover, mode: u32) -> i32;
    pub fn sbn_prove_set_guard(mode: u32) -> i32;
    pub fn sbn_prover_guard_stats(p: *const sbn_prover, out: *mut u64) -> i32;
    pub fn sbn_batch_prover_guard_stats(b: *const sbn_batch_prover, out: *mut u64) -> i32;
    pub fn sbn_msm_num_units(count: usize, num_io: usize) -> usize;
    pub fn sbn_msm_instances(kind: i32, terms: *const u32, count: usize, num_io: usize, start: *const u32, ios_out: *mut u32, final_out: *mut u32) -> i32;
    pub fn sbn_batch_prover_prove_msm(b: *mut sbn_batch_prover, terms: *const u32, count: usize, start: *const u32, proofs_out: *mut *mut sbn_proof, final_out: *mut u32, ios_out: *mut u32) -> i32;
    pub fn sbn_msm_check_links(kind: i32, num_io: usize, public_inputs: *const *const u64, units: usize, count: usize, terms: *const u32, start: *const u32, final_out: *mut u32) -> i32;
    pub fn sbn_curve_generator(kind: i32, out: *mut u32) -> i32;
    pub fn sbn_g2_cofactor(out: *mut u32) -> i32;
    pub fn sbn_scalar_mul_instances(kind: i32, points: *const u32, scalars: *const u32, scalar_count: usize, count: usize, num_io: usize, offset: *const u32, ios_out: *mut u32, products_out: *mut u32, infinity_out: *mut u8) -> i32;
    pub fn sbn_prover_generate_trace_scalar_muls(p: *mut sbn_prover, points: *const u32, scalars: *const u32, scalar_count: usize, num_io: usize, offset: *const u32, pi_out: *mut u64, products_out: *mut u32, infinity_out: *mut u8, ios_out: *mut u32) -> i32;
    pub fn sbn_batch_prover_prove_scalar_muls(b: *mut sbn_batch_prover, points: *const u32, scalars: *const u32, scalar_count: usize, count: usize, offset: *const u32, proofs_out: *mut *mut sbn_proof, products_out: *mut u32, infinity_out: *mut u8, ios_out: *mut u32) -> i32;
    pub fn sbn_scalar_mul_check(kind: i32, num_io: usize, public_inputs: *const *const u64, units: usize, count: usize, points: *const u32, scalars: *const u32, scalar_count: usize, offset: *const u32, products_out: *mut u32, infinity_out: *mut u8) -> i32;
    pub fn sbn_batch_prover_prove_mul_by_cofactor(b: *mut sbn_batch_prover, points: *const u32, count: usize, proofs_out: *mut *mut sbn_proof, cleared_out: *mut u32, infinity_out: *mut u8, ios_out: *mut u32) -> i32;
    pub fn sbn_mul_by_cofactor_check(num_io: usize, public_inputs: *const *const u64, units: usize, count: usize, points: *const u32, cleared_out: *mut u32, infinity_out: *mut u8) -> i32;
    pub fn sbn_bn_x(out: *mut u32) -> i32;
    pub fn sbn_power_instances(kind: i32, bases: *const u32, exps: *const u32, exp_count: usize, count: usize, depth: usize, num_io: usize, ios_out: *mut u32, powers_out: *mut u32) -> i32;
    pub fn sbn_prover_generate_trace_powers(p: *mut sbn_prover, bases: *const u32, exps: *const u32, exp_count: usize, count: usize, depth: usize, pi_out: *mut u64, powers_out: *mut u32, ios_out: *mut u32) -> i32;
    pub fn sbn_batch_prover_prove_powers(b: *mut sbn_batch_prover, bases: *const u32, exps: *const u32, exp_count: usize, count: usize, depth: usize, proofs_out: *mut *mut sbn_proof, powers_out: *mut u32, ios_out: *mut u32) -> i32;
    pub fn sbn_power_check(kind: i32, num_io: usize, public_inputs: *const *const u64, units: usize, count: usize, depth: usize, bases: *const u32, exps: *const u32, exp_count: usize, powers_out: *mut u32) -> i32;
    pub fn sbn_program_levels(nodes: *const sbn_program_node, count: usize, level_out: *mut u32, depth_out: *mut u32) -> i32;
    pub fn sbn_program_instances(kind: i32, nodes: *const sbn_program_node, count: usize, values: *const u32, n_values: usize, exps: *const u32, n_exps: usize, num_io: usize, ios_out: *mut u32, outs_out: *mut u32) -> i32;
    pub fn sbn_prover_generate_trace_program(p: *mut sbn_prover, nodes: *const sbn_program_node, count: usize, values: *const u32, n_values: usize, exps: *const u32, n_exps: usize, pi_out: *mut u64, outs_out: *mut u32, ios_out: *mut u32) -> i32;
    pub fn sbn_batch_prover_prove_program(b: *mut sbn_batch_prover, nodes: *const sbn_program_node, count: usize, values: *const u32, n_values: usize, exps: *const u32, n_exps: usize, proofs_out: *mut *mut sbn_proof, outs_out: *mut u32, ios_out: *mut u32) -> i32;
    pub fn sbn_program_check(kind: i32, num_io: usize, public_inputs: *const *const u64, units: usize, nodes: *const sbn_program_node, count: usize, values: *const u32, n_values: usize, exps: *const u32, n_exps: usize, outs_out: *mut u32) -> i32;
    pub fn sbn_curve_program_instances(kind: i32, nodes: *const sbn_program_node, count: usize, points: *const u32, n_points: usize, exps: *const u32, n_exps: usize, num_io: usize, ios_out: *mut u32, outs_out: *mut u32, values_out: *mut u32, infinity_out: *mut u8, choice_out: *mut u8) -> i32;
    pub fn sbn_prover_generate_trace_curve_program(p: *mut sbn_prover, nodes: *const sbn_program_node, count: usize, points: *const u32, n_points: usize, exps: *const u32, n_exps: usize, pi_out: *mut u64, outs_out: *mut u32, values_out: *mut u32, infinity_out: *mut u8, choice_out: *mut u8, ios_out: *mut u32) -> i32;
    pub fn sbn_batch_prover_prove_curve_program(b: *mut sbn_batch_prover, nodes: *const sbn_program_node, count: usize, points: *const u32, n_points: usize, exps: *const u32, n_exps: usize, proofs_out: *mut *mut sbn_proof, outs_out: *mut u32, values_out: *mut u32, infinity_out: *mut u8, choice_out: *mut u8, ios_out: *mut u32) -> i32;
    pub fn sbn_curve_program_check(kind: i32, num_io: usize, public_inputs: *const *const u64, units: usize, nodes: *const sbn_program_node, count: usize, points: *const u32, n_points: usize, exps: *const u32, n_exps: usize, choice: u32, outs_out: *mut u32, values_out: *mut u32, infinity_out: *mut u8) -> i32;

    pub fn sbn_proof_num_words(p: *const sbn_proof) -> usize;
    pub fn sbn_proof_words(p: *const sbn_proof) -> *const u64;
    pub fn sbn_proof_free(p: *mut sbn_proof);
    pub fn sbn_verify(air: *const sbn_air_desc, cfg: *const sbn_config, bytes: *const u8, len: usize) -> i32;

    pub fn sbn_verifier_create(air: *const sbn_air_desc, cfg: *const sbn_config, degree_bits: u32, max_batch: u32, out: *mut *mut sbn_verifier) -> i32;
    pub fn sbn_verifier_verify(v: *mut sbn_verifier, proofs: *const *const u8, lens: *const usize, count: usize, status_out: *mut i32) -> i32;
    pub fn sbn_verifier_reason(v: *const sbn_verifier, i: usize) -> *const c_char;
    pub fn sbn_verifier_stage_times(v: *const sbn_verifier, ms_out: *mut f32, cap: i32) -> i32;
    pub fn sbn_verifier_destroy(v: *mut sbn_verifier);
}
