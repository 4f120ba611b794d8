"""Host-side mirror of the reference's operator interface for the G1 prover path.

Names follow the reference (src/curves/g1/exp.rs:232-328, :811-826):
    stark = G1ExpStark(num_io);  config = stark.config()
    trace = stark.generate_trace(inputs);  pi = stark.generate_public_inputs(inputs)
    proof = prove(stark, config, trace, pi);  verify_stark_proof(stark, proof, config)
Errors surface as SbnError (the reference returns anyhow::Result and callers unwrap).
"""
import collections
import ctypes as C
import os
import numpy as np

AIR_G1_OP = 1
AIR_MODULAR = 7
AIR_FQ12_MUL = 8
AIR_LOOKUP = 9
AIR_FLAGS = 10
AIR_FLAGS_U64 = 11
AIR_G1_EXP = 2
AIR_G2_EXP = 3
AIR_FQ12_EXP = 4
AIR_FQ_EXP = 5
AIR_FQ12_EXP_U64 = 6

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# every symbol include/sbn.h declares
EXPORTS = [
    "sbn_version", "sbn_last_error", "sbn_device_count", "sbn_set_device", "sbn_set_thread_device", "sbn_standard_fast_config", "sbn_config_for_rate",
    "sbn_air_num_columns", "sbn_air_num_public_inputs", "sbn_air_num_permutation_zs", "sbn_air_num_constraints",
    "sbn_generate_trace_g1_exp", "sbn_generate_trace_g2_exp", "sbn_generate_trace_fq12_exp", "sbn_generate_trace_fq_exp", "sbn_generate_trace_fq12_exp_u64",
    "sbn_generate_trace_g1_op", "sbn_generate_trace_modular", "sbn_generate_trace_fq12_mul", "sbn_generate_trace_lookup", "sbn_generate_trace_flags", "sbn_generate_trace_flags_u64",
    "sbn_prover_create", "sbn_prover_destroy", "sbn_prover_load_trace", "sbn_prover_load_trace_device",
    "sbn_prover_prove", "sbn_prover_prove_host_trace", "sbn_prover_stage_times", "sbn_prover_stage_name", "sbn_prover_describe", "sbn_settings_check", "sbn_prover_trace_device_ptr",
    "sbn_prover_generate_trace", "sbn_prover_read_trace", "sbn_chain_instances", "sbn_prover_generate_trace_chained",
    "sbn_prover_check_trace", "sbn_prover_check_times", "sbn_check_trace_host", "sbn_trace_segment_name",
    "sbn_air_constraint_blocks", "sbn_constraint_section_name", "sbn_air_permutation_pair", "sbn_explain_rows_host", "sbn_explain_trace_host",
    "sbn_prover_explain_rows", "sbn_prover_explain_trace", "sbn_prover_explain_times", "sbn_split_prover_explain_rows", "sbn_split_prover_explain_trace",
    "sbn_explain_permutations_host", "sbn_prover_explain_permutations", "sbn_prover_explain_permutation_times",
    "sbn_instances_from_public_inputs", "sbn_prover_diff_witness", "sbn_prover_diff_witness_times", "sbn_diff_witness_host",
    "sbn_batch_prover_create", "sbn_batch_prover_prove_ios", "sbn_batch_prover_destroy",
    "sbn_msm_num_units", "sbn_msm_instances", "sbn_batch_prover_prove_msm", "sbn_msm_check_links",
    "sbn_curve_generator", "sbn_g2_cofactor", "sbn_scalar_mul_instances", "sbn_prover_generate_trace_scalar_muls",
    "sbn_batch_prover_prove_scalar_muls", "sbn_scalar_mul_check", "sbn_batch_prover_prove_mul_by_cofactor", "sbn_mul_by_cofactor_check",
    "sbn_msm_batch_instances", "sbn_prover_generate_trace_msm_batch", "sbn_batch_prover_prove_msm_batch", "sbn_msm_batch_check",
    "sbn_start_candidate", "sbn_msm_batch_instances_complete", "sbn_prover_generate_trace_msm_batch_complete", "sbn_batch_prover_prove_msm_batch_complete",
    "sbn_bn_x", "sbn_power_instances", "sbn_prover_generate_trace_powers", "sbn_batch_prover_prove_powers", "sbn_power_check",
    "sbn_program_levels", "sbn_program_instances", "sbn_prover_generate_trace_program", "sbn_batch_prover_prove_program", "sbn_program_check",
    "sbn_fq12_frobenius", "sbn_fq12_inverse",
    "sbn_program_m_levels", "sbn_program_m_instances", "sbn_prover_generate_trace_program_m", "sbn_batch_prover_prove_program_m", "sbn_program_m_check",
    "sbn_curve_program_instances", "sbn_prover_generate_trace_curve_program", "sbn_batch_prover_prove_curve_program", "sbn_curve_program_check",
    "sbn_prove", "sbn_prove_cache_configure", "sbn_prove_cache_stats", "sbn_first_non_canonical", "sbn_proof_num_words", "sbn_proof_words", "sbn_proof_serialize", "sbn_proof_degree_bits",
    "sbn_proof_free", "sbn_verify", "sbn_commit_values", "sbn_poseidon_permute_batch", "sbn_poseidon_permute_coop_batch", "sbn_poseidon_permute_host", "sbn_field_mul_batch", "sbn_bn254_fq_batch",
    "sbn_eval_constraints_host", "sbn_host_curve_chains", "sbn_split_exchange_bytes", "sbn_split_prover_create", "sbn_split_prover_destroy", "sbn_split_prover_generate_trace",
    "sbn_split_prover_load_trace", "sbn_split_prover_prove", "sbn_split_prover_stage_times", "sbn_split_prover_check_trace",
    "sbn_abi_version", "sbn_rccl_unique_id", "sbn_rccl_comm_create", "sbn_rccl_comm_destroy",
    "sbn_local_comm_create", "sbn_local_comm_abort", "sbn_local_comm_destroy", "sbn_comm_selftest",
    "sbn_verifier_create", "sbn_verifier_verify", "sbn_verifier_reason", "sbn_verifier_stage_times", "sbn_verifier_destroy",
    "sbn_prover_create_with", "sbn_batch_prover_create_with", "sbn_prover_memory_plan", "sbn_lde_rows",
    "sbn_prover_prove_host_columns", "sbn_prove_columns", "sbn_batch_prover_prove_host_columns", "sbn_gather_columns", "sbn_reduce_words",
    "sbn_fixed_columns_range", "sbn_fixed_columns_check",
    "sbn_air_num_main_columns", "sbn_trace_from_rows_host", "sbn_prover_load_trace_rows", "sbn_prover_load_trace_rows_device", "sbn_prover_prove_host_rows", "sbn_prove_rows",
    "sbn_prover_set_guard", "sbn_batch_prover_set_guard", "sbn_prove_set_guard", "sbn_prover_guard_stats", "sbn_batch_prover_guard_stats", "sbn_split_prover_set_guard",
]


class SbnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sbn error {code}: {msg}")
        self.code = code
        self.reason = msg   # sbn_last_error() as it was: behind code -6 the verifier's own reason


class _AirDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("num_io", C.c_uint32)]


class _Config(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("security_bits", "num_challenges", "rate_bits", "cap_height",
                                            "proof_of_work_bits", "fri_arity_bits", "fri_final_poly_bits", "num_query_rounds",
                                            "fri_variant")]


FRI_DEFAULT, FRI_TIMES_X, FRI_PLAIN = 0, 1, 2   # sbn_fri_variant (include/sbn.h)


class _ProverOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("lde_storage", C.c_uint32)]


LDE_STORAGE = {"full": 0, "compact": 1}   # SBN_LDE_FULL, SBN_LDE_COMPACT


def _prover_options(lde):
    """The sbn_prover_options of an `lde=` argument: None stands for no options at all, a name for its mode, an integer for itself
    (so that a caller can hand the library a mode it does not know)."""
    if lde is None:
        return None
    if isinstance(lde, str):
        if lde not in LDE_STORAGE:
            raise ValueError(f"lde must be one of {sorted(LDE_STORAGE)}, not {lde!r}")
        lde = LDE_STORAGE[lde]
    return _ProverOptions(C.sizeof(_ProverOptions), int(lde))


def _opt_ref(opt):
    return C.byref(opt) if opt is not None else None


class _HostRows(C.Structure):
    """sbn_host_rows (include/sbn.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("flat", C.c_void_p), ("row_stride", C.c_size_t), ("row_ptrs", C.c_void_p),
                ("n_rows", C.c_size_t), ("n_cols", C.c_size_t)]


class _TraceReport(C.Structure):
    """sbn_trace_report (include/sbn.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("num_segments", C.c_uint32), ("rows", C.c_uint64), ("failing_rows", C.c_uint64),
                ("first_failing_row", C.c_uint64), ("seg_failing_rows", C.c_uint64 * 4), ("seg_first_row", C.c_uint64 * 4),
                ("num_zs", C.c_uint32), ("z_split", C.c_uint32)]


class _WitnessDiff(C.Structure):
    """sbn_witness_diff (include/sbn.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(n, C.c_uint64) for n in (
        "cells", "main_cells", "rows", "columns", "first_row", "first_column", "listed", "pi_words", "first_pi_word")]


class _ConstraintBlock(C.Structure):
    """sbn_constraint_block (include/sbn.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("first", "count", "segment", "section", "instance", "col_first", "col_count")]


class _BlockStat(C.Structure):
    """sbn_block_stat (include/sbn.h)."""
    _fields_ = [("failing_rows", C.c_uint64), ("first_row", C.c_uint64)]


def lib_path():
    """The in-tree HIP library; SBN_LIB selects another build of the same ABI (A/B measurements)."""
    return os.environ.get("SBN_LIB") or os.path.join(_HERE, "libsbn254.so")


def lib():
    """Loads libsbn254.so; raises if the HIP extension has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise SbnError(-100, f"{p} is missing: build it with `make -C starky_bn254_amd/csrc` (there is no CPU fallback)")
        L = C.CDLL(p)
        vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
        L.sbn_version.restype = C.c_char_p
        L.sbn_last_error.restype = C.c_char_p
        L.sbn_prover_stage_name.restype = C.c_char_p
        L.sbn_prover_stage_name.argtypes = [C.c_int]
        for f in ("sbn_air_num_columns", "sbn_air_num_public_inputs", "sbn_air_num_constraints"):
            getattr(L, f).restype = sz
            getattr(L, f).argtypes = [C.POINTER(_AirDesc)]
        L.sbn_air_num_permutation_zs.restype = sz
        L.sbn_air_num_permutation_zs.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config)]
        L.sbn_standard_fast_config.argtypes = [C.POINTER(_Config)]
        L.sbn_config_for_rate.argtypes = [u32, C.POINTER(_Config)]
        L.sbn_config_for_rate.restype = None
        L.sbn_generate_trace_g1_exp.argtypes = [vp, sz, vp, vp]
        L.sbn_generate_trace_g2_exp.argtypes = [vp, sz, vp, vp]
        L.sbn_generate_trace_fq12_exp.argtypes = [vp, sz, vp, vp]
        L.sbn_generate_trace_fq_exp.argtypes = [vp, sz, vp, vp]
        L.sbn_generate_trace_fq12_exp_u64.argtypes = [vp, sz, vp, vp]
        L.sbn_generate_trace_g1_op.argtypes = [vp, sz, vp]
        L.sbn_generate_trace_modular.argtypes = [vp, sz, vp]
        L.sbn_generate_trace_fq12_mul.argtypes = [vp, sz, vp]
        L.sbn_generate_trace_lookup.argtypes = [vp, vp, sz, vp]
        L.sbn_generate_trace_flags.argtypes = [vp, sz, vp]
        L.sbn_generate_trace_flags_u64.argtypes = [vp, sz, vp]
        L.sbn_prover_create.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config), u32, C.POINTER(vp)]
        if hasattr(L, "sbn_prover_create_with"):   # (an older build named by SBN_LIB for an A/B lacks the four: full contexts still work with it)
            L.sbn_prover_create_with.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config), u32, C.POINTER(_ProverOptions), C.POINTER(vp)]
            L.sbn_batch_prover_create_with.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config), u32, u32, C.POINTER(_ProverOptions), C.POINTER(vp)]
            L.sbn_prover_memory_plan.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config), u32, C.POINTER(_ProverOptions), C.POINTER(C.c_uint64)]
            L.sbn_lde_rows.argtypes = [vp, sz, u32, u32, vp, sz, vp]
        L.sbn_prover_destroy.argtypes = [vp]
        L.sbn_prover_load_trace.argtypes = [vp, vp, vp, sz]
        L.sbn_prover_load_trace_device.argtypes = [vp, vp, vp, sz]
        L.sbn_prover_prove.argtypes = [vp, C.POINTER(vp)]
        L.sbn_prover_prove_host_trace.argtypes = [vp, vp, vp, sz, C.POINTER(vp)]
        if hasattr(L, "sbn_prover_prove_host_columns"):   # (absent from an older build named by SBN_LIB for an A/B)
            L.sbn_prover_prove_host_columns.argtypes = [vp, vp, sz, u32, vp, sz, vp, C.POINTER(vp)]
            L.sbn_prove_columns.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config), vp, sz, u32, u32, vp, sz, C.POINTER(vp)]
            L.sbn_batch_prover_prove_host_columns.argtypes = [vp, vp, sz, u32, vp, sz, sz, C.POINTER(vp)]
            L.sbn_gather_columns.argtypes = [vp, sz, sz, sz, sz, vp]
            L.sbn_reduce_words.argtypes = [vp, sz, C.c_int, vp]
        L.sbn_prove_cache_configure.argtypes = [C.c_uint64]
        L.sbn_prove_cache_stats.argtypes = [vp]
        L.sbn_first_non_canonical.argtypes = [vp, sz, C.c_int, vp]
        L.sbn_prover_stage_times.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
        L.sbn_prover_trace_device_ptr.restype = vp
        L.sbn_prover_trace_device_ptr.argtypes = [vp]
        L.sbn_prover_generate_trace.argtypes = [vp, vp, sz, vp]
        L.sbn_prover_read_trace.argtypes = [vp, vp]
        L.sbn_chain_instances.argtypes = [C.c_int32, vp, sz, vp, vp, vp]
        L.sbn_prover_generate_trace_chained.argtypes = [vp, vp, sz, vp, vp, vp]
        L.sbn_prover_check_trace.argtypes = [vp, C.c_uint64, C.POINTER(_TraceReport), vp]
        L.sbn_prover_check_times.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
        L.sbn_check_trace_host.argtypes = [C.POINTER(_AirDesc), vp, u32, vp, sz, C.c_uint64, C.POINTER(_TraceReport), vp]
        L.sbn_trace_segment_name.restype = C.c_char_p
        L.sbn_trace_segment_name.argtypes = [C.c_int]
        L.sbn_split_prover_check_trace.argtypes = [vp, C.c_uint64, C.POINTER(_TraceReport), vp]
        L.sbn_air_constraint_blocks.restype = sz
        L.sbn_air_constraint_blocks.argtypes = [C.POINTER(_AirDesc), vp, sz]
        L.sbn_constraint_section_name.restype = C.c_char_p
        L.sbn_constraint_section_name.argtypes = [C.c_int]
        L.sbn_air_permutation_pair.argtypes = [C.POINTER(_AirDesc), sz, C.POINTER(u32), C.POINTER(u32)]
        L.sbn_explain_rows_host.argtypes = [C.POINTER(_AirDesc), vp, u32, vp, sz, C.c_uint64, vp, sz, vp, vp]
        L.sbn_explain_trace_host.argtypes = [C.POINTER(_AirDesc), vp, u32, vp, sz, C.c_uint64, vp, vp]
        L.sbn_prover_explain_rows.argtypes = [vp, C.c_uint64, vp, sz, vp, vp]
        L.sbn_prover_explain_trace.argtypes = [vp, C.c_uint64, vp, vp]
        L.sbn_prover_explain_times.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
        L.sbn_explain_permutations_host.argtypes = [C.POINTER(_AirDesc), vp, u32, vp, sz, sz, vp, vp]
        L.sbn_prover_explain_permutations.argtypes = [vp, vp, sz, sz, vp, vp]
        L.sbn_prover_explain_permutation_times.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
        if hasattr(L, "sbn_prover_diff_witness"):   # (a library named by SBN_LIB may predate the witness diff)
            L.sbn_instances_from_public_inputs.argtypes = [C.c_int32, vp, sz, sz, vp, vp]
            L.sbn_prover_diff_witness.argtypes = [vp, vp, sz, C.POINTER(_WitnessDiff), vp, vp, vp, sz]
            L.sbn_prover_diff_witness_times.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
            L.sbn_diff_witness_host.argtypes = [C.POINTER(_AirDesc), vp, u32, vp, sz, vp, sz, C.POINTER(_WitnessDiff), vp, vp, vp, sz]
        L.sbn_split_prover_explain_rows.argtypes = [vp, C.c_uint64, vp, sz, vp, vp]
        L.sbn_split_prover_explain_trace.argtypes = [vp, C.c_uint64, vp, vp]
        L.sbn_batch_prover_create.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config), u32, u32, C.POINTER(vp)]
        L.sbn_batch_prover_prove_ios.argtypes = [vp, vp, sz, sz, sz, C.POINTER(vp)]
        L.sbn_batch_prover_destroy.argtypes = [vp]
        L.sbn_msm_num_units.restype = sz
        L.sbn_msm_num_units.argtypes = [sz, sz]
        L.sbn_msm_instances.argtypes = [C.c_int32, vp, sz, sz, vp, vp, vp]
        L.sbn_batch_prover_prove_msm.argtypes = [vp, vp, sz, vp, C.POINTER(vp), vp, vp]
        L.sbn_msm_check_links.argtypes = [C.c_int32, sz, C.POINTER(vp), sz, sz, vp, vp, vp]
        L.sbn_curve_generator.argtypes = [C.c_int32, vp]
        L.sbn_g2_cofactor.argtypes = [vp]
        L.sbn_scalar_mul_instances.argtypes = [C.c_int32, vp, vp, sz, sz, sz, vp, vp, vp, vp]
        L.sbn_prover_generate_trace_scalar_muls.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp]
        L.sbn_batch_prover_prove_scalar_muls.argtypes = [vp, vp, vp, sz, sz, vp, C.POINTER(vp), vp, vp, vp]
        L.sbn_scalar_mul_check.argtypes = [C.c_int32, sz, C.POINTER(vp), sz, sz, vp, vp, sz, vp, vp, vp]
        L.sbn_batch_prover_prove_mul_by_cofactor.argtypes = [vp, vp, sz, C.POINTER(vp), vp, vp, vp]
        L.sbn_mul_by_cofactor_check.argtypes = [sz, C.POINTER(vp), sz, sz, vp, vp, vp]
        L.sbn_msm_batch_instances.argtypes = [C.c_int32, vp, vp, sz, vp, sz, sz, vp, vp, vp, vp]
        L.sbn_prover_generate_trace_msm_batch.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp]
        L.sbn_batch_prover_prove_msm_batch.argtypes = [vp, vp, vp, sz, vp, sz, C.POINTER(vp), vp, vp, vp, vp]
        L.sbn_msm_batch_check.argtypes = [C.c_int32, sz, C.POINTER(vp), sz, vp, sz, vp, vp, sz, vp, vp, vp]
        L.sbn_start_candidate.argtypes = [C.c_int32, C.c_uint32, vp]
        L.sbn_msm_batch_instances_complete.argtypes = [C.c_int32, vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]
        L.sbn_prover_generate_trace_msm_batch_complete.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
        L.sbn_batch_prover_prove_msm_batch_complete.argtypes = [vp, vp, vp, vp, sz, C.POINTER(vp), vp, vp, vp, vp, vp, vp, vp]
        L.sbn_bn_x.argtypes = [vp]
        L.sbn_power_instances.argtypes = [C.c_int32, vp, vp, sz, sz, sz, sz, vp, vp]
        L.sbn_prover_generate_trace_powers.argtypes = [vp, vp, vp, sz, sz, sz, vp, vp, vp]
        L.sbn_batch_prover_prove_powers.argtypes = [vp, vp, vp, sz, sz, sz, C.POINTER(vp), vp, vp]
        L.sbn_power_check.argtypes = [C.c_int32, sz, C.POINTER(vp), sz, sz, sz, vp, vp, sz, vp]
        L.sbn_program_levels.argtypes = [vp, sz, vp, vp]
        L.sbn_program_instances.argtypes = [C.c_int32, vp, sz, vp, sz, vp, sz, sz, vp, vp]
        L.sbn_prover_generate_trace_program.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, vp, vp]
        L.sbn_batch_prover_prove_program.argtypes = [vp, vp, sz, vp, sz, vp, sz, C.POINTER(vp), vp, vp]
        L.sbn_program_check.argtypes = [C.c_int32, sz, C.POINTER(vp), sz, vp, sz, vp, sz, vp, sz, vp]
        L.sbn_fq12_frobenius.argtypes = [vp, u32, vp]
        L.sbn_fq12_inverse.argtypes = [vp, vp]
        L.sbn_program_m_levels.argtypes = L.sbn_program_levels.argtypes
        L.sbn_program_m_instances.argtypes = L.sbn_program_instances.argtypes
        L.sbn_prover_generate_trace_program_m.argtypes = L.sbn_prover_generate_trace_program.argtypes
        L.sbn_batch_prover_prove_program_m.argtypes = L.sbn_batch_prover_prove_program.argtypes
        L.sbn_program_m_check.argtypes = L.sbn_program_check.argtypes
        L.sbn_curve_program_instances.argtypes = [C.c_int32, vp, sz, vp, sz, vp, sz, sz, vp, vp, vp, vp, vp]
        L.sbn_prover_generate_trace_curve_program.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp]
        L.sbn_batch_prover_prove_curve_program.argtypes = [vp, vp, sz, vp, sz, vp, sz, C.POINTER(vp), vp, vp, vp, vp, vp]
        L.sbn_curve_program_check.argtypes = [C.c_int32, sz, C.POINTER(vp), sz, vp, sz, vp, sz, vp, sz, u32, vp, vp, vp]
        L.sbn_prove.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config), vp, u32, vp, sz, C.POINTER(vp)]
        L.sbn_proof_num_words.restype = sz
        L.sbn_proof_num_words.argtypes = [vp]
        L.sbn_proof_words.restype = C.POINTER(C.c_uint64)
        L.sbn_proof_words.argtypes = [vp]
        L.sbn_proof_serialize.restype = sz
        L.sbn_proof_serialize.argtypes = [vp, vp, sz]
        L.sbn_proof_degree_bits.restype = u32
        L.sbn_proof_degree_bits.argtypes = [vp]
        L.sbn_proof_free.argtypes = [vp]
        L.sbn_verify.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config), vp, sz]
        L.sbn_verifier_create.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config), u32, u32, C.POINTER(vp)]
        L.sbn_verifier_verify.argtypes = [vp, vp, vp, sz, vp]
        L.sbn_verifier_reason.restype = C.c_char_p
        L.sbn_verifier_reason.argtypes = [vp, sz]
        L.sbn_verifier_stage_times.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
        L.sbn_verifier_destroy.argtypes = [vp]
        L.sbn_commit_values.argtypes = [vp, sz, sz, u32, u32, vp, vp, vp]
        L.sbn_poseidon_permute_batch.argtypes = [vp, sz]
        if hasattr(L, "sbn_poseidon_permute_coop_batch"):   # (absent from an older build named by SBN_LIB for an A/B)
            L.sbn_poseidon_permute_coop_batch.argtypes = [vp, sz]
        L.sbn_poseidon_permute_host.argtypes = [vp, sz, C.c_int]
        L.sbn_field_mul_batch.argtypes = [vp, vp, vp, sz, C.c_int]
        L.sbn_bn254_fq_batch.argtypes = [C.c_int, vp, vp, vp, sz, C.c_int]
        L.sbn_set_device.argtypes = [C.c_int]
        L.sbn_set_thread_device.argtypes = [C.c_int]
        L.sbn_host_curve_chains.argtypes = [C.c_int, vp, sz, vp, vp, C.c_int]
        L.sbn_prover_describe.argtypes = [vp, C.c_char_p, sz]
        L.sbn_settings_check.argtypes = [C.c_char_p, sz]
        if hasattr(L, "sbn_fixed_columns_range"):   # (a library named by SBN_LIB may predate them)
            L.sbn_fixed_columns_range.argtypes = [vp, vp, vp]
            L.sbn_fixed_columns_check.argtypes = [vp, C.c_uint32, vp, vp]
        if hasattr(L, "sbn_prover_load_trace_rows"):   # (a library named by SBN_LIB may predate the row-major calls)
            L.sbn_air_num_main_columns.restype = sz
            L.sbn_air_num_main_columns.argtypes = [C.POINTER(_AirDesc)]
            L.sbn_trace_from_rows_host.argtypes = [C.POINTER(_AirDesc), C.POINTER(_HostRows), u32, vp, vp]
            L.sbn_prover_load_trace_rows.argtypes = [vp, C.POINTER(_HostRows), u32, vp, sz, vp]
            L.sbn_prover_load_trace_rows_device.argtypes = [vp, vp, sz, sz, u32, vp, sz, vp]
            L.sbn_prover_prove_host_rows.argtypes = [vp, C.POINTER(_HostRows), u32, vp, sz, vp, C.POINTER(vp)]
            L.sbn_prove_rows.argtypes = [C.POINTER(_AirDesc), C.POINTER(_Config), C.POINTER(_HostRows), u32, vp, sz, C.POINTER(vp)]
        if hasattr(L, "sbn_prover_set_guard"):
            for f in ("sbn_prover_set_guard", "sbn_batch_prover_set_guard", "sbn_split_prover_set_guard"):
                getattr(L, f).argtypes = [vp, u32]
            L.sbn_prove_set_guard.argtypes = [u32]
            L.sbn_prover_guard_stats.argtypes = [vp, vp]
            L.sbn_batch_prover_guard_stats.argtypes = [vp, vp]
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        raise SbnError(rc, lib().sbn_last_error().decode())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


GUARD = {None: 0, "off": 0, "device": 1, "host": 2}   # SBN_GUARD_OFF, SBN_GUARD_DEVICE, SBN_GUARD_HOST


def _guard_mode(guard):
    """The mode of a `guard=` argument: None / "off", "device", "host", or an integer for itself (so that a caller can hand the
    library a mode it does not know)."""
    if guard is None or isinstance(guard, str):
        if guard not in GUARD:
            raise ValueError(f"guard must be None, 'device' or 'host', not {guard!r}")
        return GUARD[guard]
    return int(guard)


GuardStats = collections.namedtuple("GuardStats", ("checked", "rejected", "ns", "device_bytes"))


def _guard_stats(getter, h):
    out = (C.c_uint64 * 4)()
    _check(getter(h, out))
    return GuardStats(*(int(v) for v in out))


def prove_set_guard(guard):
    """Verified proving for the one-shot calls prove() / prove_columns() / prove_rows(), process-wide (sbn_prove_set_guard): with
    "device" or "host" a proof that its verifier rejects is an SbnError with code -6 and the verifier's reason; None restores the
    unguarded calls."""
    _check(lib().sbn_prove_set_guard(_guard_mode(guard)))


class StarkConfig:
    """starky `StarkConfig` (+ FriConfig); `standard_fast_config()` as in exp.rs:250-253."""

    def __init__(self):
        self._c = _Config()
        lib().sbn_standard_fast_config(C.byref(self._c))

    @staticmethod
    def standard_fast_config(num_columns=None, num_public_inputs=None):
        return StarkConfig()

    @staticmethod
    def for_rate(rate_bits):
        """standard_fast_config at another blowup and the same conjectured security (sbn_config_for_rate): 84 / 42 / 28 queries
        at rate_bits 1 / 2 / 3.  The provers and verifiers accept rate_bits 1 and 3."""
        cfg = StarkConfig()
        lib().sbn_config_for_rate(rate_bits, C.byref(cfg._c))
        return cfg

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "_c"), name)

    def __setattr__(self, name, value):
        if name != "_c" and any(name == f[0] for f in _Config._fields_):
            setattr(self._c, name, value)
        else:
            object.__setattr__(self, name, value)


class _Stark:
    kind = 0

    def __init__(self, num_io=0):
        self.num_io = num_io
        self._d = _AirDesc(self.kind, num_io)

    def config(self):
        return StarkConfig.standard_fast_config(self.num_columns, self.num_public_inputs)

    @property
    def num_columns(self):
        return lib().sbn_air_num_columns(C.byref(self._d))

    @property
    def num_public_inputs(self):
        return lib().sbn_air_num_public_inputs(C.byref(self._d))

    @property
    def num_main_columns(self):
        """Columns of a row in front of the reference's `transpose` (sbn_air_num_main_columns): what main-row mode of the row-major
        calls takes; 0 for a table that is no Exp table."""
        return lib().sbn_air_num_main_columns(C.byref(self._d))

    def num_permutation_zs(self, config=None):
        config = config or StarkConfig()
        return lib().sbn_air_num_permutation_zs(C.byref(self._d), C.byref(config._c))

    @property
    def num_constraints(self):
        return lib().sbn_air_num_constraints(C.byref(self._d))

    def constraint_degree(self):
        return 3

    def constraint_blocks(self):
        """The blocks of the table's constraint stream (sbn_air_constraint_blocks): the emissions of the regrouped evaluator, in
        order, as ConstraintBlock objects.  What explain_rows / explain_trace name."""
        blocks = getattr(self, "_blocks", None)
        if blocks is None:
            B = lib().sbn_air_constraint_blocks(C.byref(self._d), None, 0)
            if B == 0:
                raise SbnError(-1, lib().sbn_last_error().decode())
            raw = (_ConstraintBlock * B)()
            lib().sbn_air_constraint_blocks(C.byref(self._d), raw, B)
            blocks = self._blocks = [ConstraintBlock(b, r) for b, r in enumerate(raw)]
        return blocks

    def permutation_pair(self, z):
        """(lhs column, rhs column) of permutation Z column z (sbn_air_permutation_pair)."""
        lhs, rhs = C.c_uint32(), C.c_uint32()
        _check(lib().sbn_air_permutation_pair(C.byref(self._d), z, C.byref(lhs), C.byref(rhs)))
        return int(lhs.value), int(rhs.value)


class G1Stark(_Stark):
    """Reference `G1Stark` (src/curves/g1/muladd.rs:462-624): one affine add per row."""
    kind = AIR_G1_OP

    def __init__(self):
        super().__init__(0)

    def generate_trace(self, pts):
        """pts: (rows, 32) uint32 = a.x a.y b.x b.y as 8xu32 LE limbs -> column-major (ncols, rows) uint64."""
        pts = np.ascontiguousarray(pts, dtype=np.uint32)
        rows = pts.shape[0]
        trace = np.zeros((self.num_columns, rows), dtype=np.uint64)
        _check(lib().sbn_generate_trace_g1_op(_ptr(pts), rows, _ptr(trace)))
        return trace


class ModularStark(_Stark):
    """Reference `ModularStark` (src/modular/modular.rs:361-537): one a * b mod p per row -- the reference's test table for the modular gadget."""
    kind = AIR_MODULAR

    def __init__(self):
        super().__init__(0)

    def generate_trace(self, ops):
        """ops: (rows, 16) uint32 = a b as 8xu32 LE limbs (both < p) -> column-major (ncols, rows) uint64."""
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        rows = ops.shape[0]
        assert ops.shape == (rows, 16)
        trace = np.zeros((self.num_columns, rows), dtype=np.uint64)
        _check(lib().sbn_generate_trace_modular(_ptr(ops), rows, _ptr(trace)))
        return trace


class LookupStark(_Stark):
    """Reference `MyStark` (src/utils/lookup.rs:136-213), the unit-test table of the lookup argument: inputs, table, permuted
    inputs, permuted table; any power-of-two height >= 512 on the device (the reference's own 8-row instance: oracle only)."""
    kind = AIR_LOOKUP

    def __init__(self):
        super().__init__(0)

    def generate_trace(self, inputs, table):
        """inputs, table: (rows,) uint64 canonical field elements, every input value present in the table -> (4, rows) uint64."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
        table = np.ascontiguousarray(table, dtype=np.uint64)
        assert inputs.shape == table.shape and inputs.ndim == 1
        trace = np.zeros((4, inputs.shape[0]), dtype=np.uint64)
        _check(lib().sbn_generate_trace_lookup(_ptr(inputs), _ptr(table), inputs.shape[0], _ptr(trace)))
        return trace


MyStark = LookupStark   # the reference's name for it (a test-module local)


class FlagStark(_Stark):
    """Reference `FlagStark` (src/utils/flags.rs:379-547), the unit-test table of the exponent-bit flags: num_io inputs of 8 u32
    limbs, 512 rows each; no permutation pairs, so its proofs carry no permutation-Z commitment."""
    kind = AIR_FLAGS

    def generate_trace(self, limbs):
        """limbs: (num_io, 8) uint32 -> (17 + 4 num_io, 512 num_io) uint64."""
        limbs = np.ascontiguousarray(limbs, dtype=np.uint32)
        assert limbs.shape == (self.num_io, 8)
        trace = np.zeros((self.num_columns, 512 * self.num_io), dtype=np.uint64)
        _check(lib().sbn_generate_trace_flags(_ptr(limbs), self.num_io, _ptr(trace)))
        return trace


class FlagU64Stark(_Stark):
    """The `FlagStark` of src/fields/fq12_u64/flags_u64.rs:289-420 (u64 exponents, 128 rows per input, no permutation pairs)."""
    kind = AIR_FLAGS_U64

    def generate_trace(self, exps):
        """exps: (num_io,) uint64 < p -> (7 + 4 num_io, 128 num_io) uint64."""
        exps = np.ascontiguousarray(exps, dtype=np.uint64)
        assert exps.shape == (self.num_io,)
        trace = np.zeros((self.num_columns, 128 * self.num_io), dtype=np.uint64)
        _check(lib().sbn_generate_trace_flags_u64(_ptr(exps), self.num_io, _ptr(trace)))
        return trace


class Fq12Stark(_Stark):
    """Reference `Fq12Stark` (src/fields/fq12/mul.rs:355-517): one Fq12 product per row -- the reference's test table for eval_fq12_mul."""
    kind = AIR_FQ12_MUL

    def __init__(self):
        super().__init__(0)

    def generate_trace(self, ops):
        """ops: (rows, 192) uint32 = x[12] y[12] (flat-basis coefficients < p, 8xu32 LE limbs each)."""
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        rows = ops.shape[0]
        assert ops.shape == (rows, 192)
        trace = np.zeros((self.num_columns, rows), dtype=np.uint64)
        _check(lib().sbn_generate_trace_fq12_mul(_ptr(ops), rows, _ptr(trace)))
        return trace


class G1ExpStark(_Stark):
    """Reference `G1ExpStark` (src/curves/g1/exp.rs:232-742): 512 rows per scalar multiplication."""
    kind = AIR_G1_EXP

    def generate_trace_and_public_inputs(self, ios):
        """ios: (num_io, 40) uint32 = x.x x.y offset.x offset.y exp_val (8xu32 LE limbs each)."""
        ios = np.ascontiguousarray(ios, dtype=np.uint32)
        assert ios.shape == (self.num_io, 40)
        trace = np.zeros((self.num_columns, 512 * self.num_io), dtype=np.uint64)
        pi = np.zeros(self.num_public_inputs, dtype=np.uint64)
        _check(lib().sbn_generate_trace_g1_exp(_ptr(ios), self.num_io, _ptr(trace), _ptr(pi)))
        return trace, pi

    def generate_trace(self, ios):
        return self.generate_trace_and_public_inputs(ios)[0]

    def generate_public_inputs(self, ios):
        return self.generate_trace_and_public_inputs(ios)[1]


class G2ExpStark(_Stark):
    """Reference `G2ExpStark` (src/curves/g2/exp.rs:248-807): G1ExpStark's machine over Fq2 coordinates."""
    kind = AIR_G2_EXP

    def generate_trace_and_public_inputs(self, ios):
        """ios: (num_io, 72) uint32 = x.x.c0 x.x.c1 x.y.c0 x.y.c1 offset.(x.c0 x.c1 y.c0 y.c1) exp_val."""
        ios = np.ascontiguousarray(ios, dtype=np.uint32)
        assert ios.shape == (self.num_io, 72)
        trace = np.zeros((self.num_columns, 512 * self.num_io), dtype=np.uint64)
        pi = np.zeros(self.num_public_inputs, dtype=np.uint64)
        _check(lib().sbn_generate_trace_g2_exp(_ptr(ios), self.num_io, _ptr(trace), _ptr(pi)))
        return trace, pi

    def generate_trace(self, ios):
        return self.generate_trace_and_public_inputs(ios)[0]

    def generate_public_inputs(self, ios):
        return self.generate_trace_and_public_inputs(ios)[1]


class Fq12ExpStark(_Stark):
    """Reference `Fq12ExpStark` (src/fields/fq12/exp.rs:223-605): offset * x^e in Fq12, 512 rows per instance."""
    kind = AIR_FQ12_EXP

    def generate_trace_and_public_inputs(self, ios):
        """ios: (num_io, 200) uint32 = x[12] offset[12] (flat-basis coefficients, 8xu32 LE limbs each) exp_val[8]."""
        ios = np.ascontiguousarray(ios, dtype=np.uint32)
        assert ios.shape == (self.num_io, 200)
        trace = np.zeros((self.num_columns, 512 * self.num_io), dtype=np.uint64)
        pi = np.zeros(self.num_public_inputs, dtype=np.uint64)
        _check(lib().sbn_generate_trace_fq12_exp(_ptr(ios), self.num_io, _ptr(trace), _ptr(pi)))
        return trace, pi

    def generate_trace(self, ios):
        return self.generate_trace_and_public_inputs(ios)[0]

    def generate_public_inputs(self, ios):
        return self.generate_trace_and_public_inputs(ios)[1]


class FqExpStark(_Stark):
    """Reference `FqExpStark` (src/fields/fq/exp.rs:193-582): offset * x^e in the base field Fq, 512 rows per instance."""
    kind = AIR_FQ_EXP

    def generate_trace_and_public_inputs(self, ios):
        """ios: (num_io, 24) uint32 = x offset exp_val (8xu32 LE limbs each)."""
        ios = np.ascontiguousarray(ios, dtype=np.uint32)
        assert ios.shape == (self.num_io, 24)
        trace = np.zeros((self.num_columns, 512 * self.num_io), dtype=np.uint64)
        pi = np.zeros(self.num_public_inputs, dtype=np.uint64)
        _check(lib().sbn_generate_trace_fq_exp(_ptr(ios), self.num_io, _ptr(trace), _ptr(pi)))
        return trace, pi

    def generate_trace(self, ios):
        return self.generate_trace_and_public_inputs(ios)[0]

    def generate_public_inputs(self, ios):
        return self.generate_trace_and_public_inputs(ios)[1]


class Fq12ExpU64Stark(_Stark):
    """Reference `Fq12ExpU64Stark` (src/fields/fq12_u64/exp_u64.rs:243-571): offset * x^e in Fq12 for a u64 exponent,
    128 rows per instance."""
    kind = AIR_FQ12_EXP_U64
    rows_per_instance = 128

    def generate_trace_and_public_inputs(self, ios):
        """ios: (num_io, 194) uint32 = x[12] offset[12] (8xu32 LE limbs each) exp_val (low, high)."""
        ios = np.ascontiguousarray(ios, dtype=np.uint32)
        assert ios.shape == (self.num_io, 194)
        trace = np.zeros((self.num_columns, 128 * self.num_io), dtype=np.uint64)
        pi = np.zeros(self.num_public_inputs, dtype=np.uint64)
        _check(lib().sbn_generate_trace_fq12_exp_u64(_ptr(ios), self.num_io, _ptr(trace), _ptr(pi)))
        return trace, pi

    def generate_trace(self, ios):
        return self.generate_trace_and_public_inputs(ios)[0]

    def generate_public_inputs(self, ios):
        return self.generate_trace_and_public_inputs(ios)[1]


# u32 words of x and of the exponent in an instance row of an Exp table: the one table of them on this side (csrc: PiLayout)
_EXP_IO_WORDS = {AIR_G1_EXP: (16, 8), AIR_G2_EXP: (32, 8), AIR_FQ_EXP: (8, 8), AIR_FQ12_EXP: (96, 8), AIR_FQ12_EXP_U64: (96, 2)}


def _chain_words(stark):
    """(u32 words of x, of the exponent) in an instance row of the Exp table `stark`."""
    try:
        return _EXP_IO_WORDS[stark.kind]
    except KeyError:
        raise SbnError(-1, "chained instance lists cover the Exp tables") from None


def _chain_args(stark, terms, start):
    xw, ew = _chain_words(stark)
    terms = np.ascontiguousarray(terms, dtype=np.uint32)
    start = np.ascontiguousarray(start, dtype=np.uint32).reshape(-1)
    if terms.ndim != 2 or terms.shape[0] < 1 or terms.shape[1] != xw + ew or start.shape[0] != xw:
        raise SbnError(-1, f"terms must be [count][{xw + ew}] u32 and start {xw} u32")
    return terms, start, xw, ew


def chain_instances(stark, terms, start):
    """The explicit instance list of a chained one (sbn_chain_instances): terms = the rows of `ios` without their offset words
    (x, then exp_val), start = the offset of instance 0; offset[k+1] = output[k].  Returns (ios, final): the list as the
    generators take it and the last output in the word shape of start.  Any count >= 1; no device needed."""
    terms, start, xw, ew = _chain_args(stark, terms, start)
    ios = np.zeros((terms.shape[0], 2 * xw + ew), dtype=np.uint32)
    final = np.zeros(xw, dtype=np.uint32)
    _check(lib().sbn_chain_instances(stark.kind, _ptr(terms), terms.shape[0], _ptr(start), _ptr(ios), _ptr(final)))
    return ios, final


def msm_num_units(count, num_io):
    """ceil(count / num_io); 0 when either is 0 (sbn_msm_num_units)."""
    return int(lib().sbn_msm_num_units(count, num_io))


def msm_instances(stark, terms, start):
    """A chained list of any length cut into units of stark.num_io instances (sbn_msm_instances): the list of chain_instances, the
    last unit padded with copies of the last instance.  Returns (ios_units, final): (units, num_io, words per instance) uint32
    as BatchProver.prove_ios takes it, and the output of the last real instance in the word shape of start.  No device needed."""
    terms, start, xw, ew = _chain_args(stark, terms, start)
    if stark.num_io < 1:
        raise SbnError(-1, "the table has no instances")
    units = msm_num_units(terms.shape[0], stark.num_io)
    ios = np.zeros((units, stark.num_io, 2 * xw + ew), dtype=np.uint32)
    final = np.zeros(xw, dtype=np.uint32)
    _check(lib().sbn_msm_instances(stark.kind, _ptr(terms), terms.shape[0], stark.num_io, _ptr(start), _ptr(ios), _ptr(final)))
    return ios, final


def _unit_public_inputs(stark, public_inputs_per_unit):
    """(pis, ptrs, n): the public inputs of every unit as flat uint64 arrays, their addresses as the C array the *_check calls take,
    and the unit count.  ptrs points into pis: keep pis referenced across the C call."""
    pis = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1) for p in public_inputs_per_unit]
    if any(p.shape[0] != stark.num_public_inputs for p in pis):
        raise SbnError(-1, f"every unit has {stark.num_public_inputs} public inputs")
    return pis, (C.c_void_p * max(len(pis), 1))(*[p.ctypes.data for p in pis]), len(pis)


def msm_check_links(stark, public_inputs_per_unit, count, start, terms=None):
    """The link check of a long chained list (sbn_msm_check_links) on the public inputs of its unit proofs: the units are one
    chained list from `start`, padded as msm_instances pads, and (with `terms`) its x and exponents are the caller's.  Returns the
    last output in the word shape of start; raises SbnError(-6) naming the first instance and field that breaks.  Verifies NO
    proof: verify_msm does both."""
    xw, ew = _chain_words(stark)
    start = np.ascontiguousarray(start, dtype=np.uint32).reshape(-1)
    if start.shape[0] != xw:
        raise SbnError(-1, f"start must be {xw} u32")
    if terms is not None:
        terms = np.ascontiguousarray(terms, dtype=np.uint32)
        if terms.shape != (count, xw + ew):
            raise SbnError(-1, f"terms must be [count][{xw + ew}] u32")
    pis, ptrs, n = _unit_public_inputs(stark, public_inputs_per_unit)
    final = np.zeros(xw, dtype=np.uint32)
    _check(lib().sbn_msm_check_links(stark.kind, stark.num_io, ptrs, n, count, _ptr(terms), _ptr(start), _ptr(final)))
    return final


# 2p - r: the twist's group has order r (2p - r); the scalar of cofactor clearing (sbn_g2_cofactor; g2/circuit.rs:335-367)
G2_COFACTOR = 21888242871839275222246405745257275088844257914179612981679871602714643921549


def _curve_words(stark):
    """u32 words of a point of the curve table `stark` (16 on G1, 32 on the twist)."""
    if stark.kind not in (AIR_G1_EXP, AIR_G2_EXP):
        raise SbnError(-7, "scalar multiplications cover the curve tables G1ExpStark and G2ExpStark")
    return _EXP_IO_WORDS[stark.kind][0]


def generator(stark):
    """The generator the reference uses as the offset of independent instances (sbn_curve_generator): (1, 2) on G1, ark_bn254's
    G2Affine::generator() on the twist, as the x words of an `ios` row."""
    out = np.zeros(_curve_words(stark), dtype=np.uint32)
    _check(lib().sbn_curve_generator(stark.kind, _ptr(out)))
    return out


def _scalar_mul_args(stark, points, scalars, offset):
    """points (count, 16E), scalars (count, 8) or (8,) / (1, 8) = one scalar shared by every instance (Python ints are taken as
    256-bit little-endian limbs), offset (16E,) or None = the generator."""
    w = _curve_words(stark)
    points = np.ascontiguousarray(points, dtype=np.uint32)
    if isinstance(scalars, int):
        scalars = [(scalars >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    scalars = np.ascontiguousarray(scalars, dtype=np.uint32)
    if scalars.ndim == 1:
        scalars = scalars.reshape(1, -1)
    if points.ndim != 2 or points.shape[1] != w or scalars.ndim != 2 or scalars.shape[1] != 8:
        raise SbnError(-1, f"points must be [count][{w}] u32 and scalars [count][8] or [8] u32")
    if offset is not None:
        offset = np.ascontiguousarray(offset, dtype=np.uint32).reshape(-1)
        if offset.shape[0] != w:
            raise SbnError(-1, f"offset must be {w} u32")
    return points, scalars, offset, w


def scalar_mul_instances(stark, points, scalars, offset=None):
    """Independent scalar multiplications e_k x_k as instances of the curve table `stark` (sbn_scalar_mul_instances): every
    instance carries `offset` (None: the generator) and the last unit is padded with copies of the last instance.  Returns
    (ios_units, products, infinity): (units, num_io, words per instance) uint32 as BatchProver.prove_ios takes it, the products
    (count, 16E) uint32 and a (count,) uint8 flag per product that is the point at infinity (its words are zero).  Scalars are
    256-bit and never reduced.  No device needed."""
    points, scalars, offset, w = _scalar_mul_args(stark, points, scalars, offset)
    count = points.shape[0]
    units = msm_num_units(count, stark.num_io)
    ios = np.zeros((units, stark.num_io, 2 * w + 8), dtype=np.uint32)
    products = np.zeros((count, w), dtype=np.uint32)
    infinity = np.zeros(count, dtype=np.uint8)
    _check(lib().sbn_scalar_mul_instances(stark.kind, _ptr(points), _ptr(scalars), scalars.shape[0], count, stark.num_io, _ptr(offset),
                                          _ptr(ios), _ptr(products), _ptr(infinity)))
    return ios, products, infinity


def scalar_mul_check(stark, public_inputs_per_unit, points, scalars, offset=None):
    """The check of a batch of scalar multiplications (sbn_scalar_mul_check) on the public inputs of its unit proofs: x, exponents
    and offset are the caller's, the pads repeat the last instance, every output is a point of the curve.  Returns (products,
    infinity) recomputed from the outputs; raises SbnError(-6) naming the first instance and field that breaks.  Verifies NO proof:
    verify_scalar_muls does both."""
    points, scalars, offset, w = _scalar_mul_args(stark, points, scalars, offset)
    count = points.shape[0]
    pis, ptrs, n = _unit_public_inputs(stark, public_inputs_per_unit)
    products = np.zeros((count, w), dtype=np.uint32)
    infinity = np.zeros(count, dtype=np.uint8)
    _check(lib().sbn_scalar_mul_check(stark.kind, stark.num_io, ptrs, n, count, _ptr(points), _ptr(scalars), scalars.shape[0],
                                      _ptr(offset), _ptr(products), _ptr(infinity)))
    return products, infinity


def mul_by_cofactor_check(stark, public_inputs_per_unit, points):
    """scalar_mul_check for cofactor clearing on the twist (sbn_mul_by_cofactor_check): the generator as offset, the shared scalar
    G2_COFACTOR.  Returns (cleared, infinity).  Any table but G2ExpStark is refused."""
    if stark.kind != AIR_G2_EXP:
        raise SbnError(-1, "cofactor clearing is a call of G2ExpStark (the twist)")
    points = np.ascontiguousarray(points, dtype=np.uint32)
    if points.ndim != 2 or points.shape[1] != 32:
        raise SbnError(-1, "points must be [count][32] u32")
    count = points.shape[0]
    pis, ptrs, n = _unit_public_inputs(stark, public_inputs_per_unit)
    cleared = np.zeros((count, 32), dtype=np.uint32)
    infinity = np.zeros(count, dtype=np.uint8)
    _check(lib().sbn_mul_by_cofactor_check(stark.num_io, ptrs, n, count, _ptr(points), _ptr(cleared), _ptr(infinity)))
    return cleared, infinity


# ---- batches of short MSMs: segmented chained lists (include/sbn.h, "Batches of short MSMs") -----------------------------------
def _msm_batch_args(stark, terms, lengths, starts):
    """terms (M, T) uint32 as chain_instances takes them, lengths (segments,) with every length >= 1 and sum M, starts (segments, W)
    = one start per segment, (W,) / (1, W) = one start shared by all, or None = the generator on a curve table, one on a field
    table.  Returns (terms, lengths, starts, xw, ew, curve)."""
    xw, ew = _chain_words(stark)
    terms = np.ascontiguousarray(terms, dtype=np.uint32)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint64).reshape(-1)
    if terms.ndim != 2 or terms.shape[0] < 1 or terms.shape[1] != xw + ew:
        raise SbnError(-1, f"terms must be [M][{xw + ew}] u32")
    if lengths.shape[0] and int(lengths.sum()) != terms.shape[0]:
        raise SbnError(-1, f"the lengths add up to {int(lengths.sum())} instances, terms holds {terms.shape[0]}")
    if starts is not None:
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        if starts.ndim == 1:
            starts = starts.reshape(1, -1)
        if starts.ndim != 2 or starts.shape[1] != xw:
            raise SbnError(-1, f"starts must be [segments][{xw}] or [{xw}] u32")
    return terms, lengths, starts, xw, ew, stark.kind in (AIR_G1_EXP, AIR_G2_EXP)


def _msm_batch_outputs(segments, xw, curve):
    finals = np.zeros((segments, xw), dtype=np.uint32)
    sums = np.zeros((segments, xw), dtype=np.uint32) if curve else None
    infinity = np.zeros(segments, dtype=np.uint8) if curve else None
    return finals, sums, infinity


def msm_batch_instances(stark, terms, lengths, starts=None):
    """Many short chained lists packed into shared units (sbn_msm_batch_instances): segment s holds lengths[s] consecutive rows of
    terms; its first instance starts from its start, every other one from the output before it; the last unit is padded with copies
    of the last instance.  Returns (ios_units, finals, sums, infinity): (units, num_io, words per instance) uint32 as
    BatchProver.prove_ios takes it, the last output of every segment, and on the curve tables final - start with a flag per sum that
    is the point at infinity (None, None on field tables).  No device needed."""
    terms, lengths, starts, xw, ew, curve = _msm_batch_args(stark, terms, lengths, starts)
    if stark.num_io < 1:
        raise SbnError(-1, "the table has no instances")
    units = msm_num_units(terms.shape[0], stark.num_io)
    ios = np.zeros((units, stark.num_io, 2 * xw + ew), dtype=np.uint32)
    finals, sums, infinity = _msm_batch_outputs(len(lengths), xw, curve)
    _check(lib().sbn_msm_batch_instances(stark.kind, _ptr(terms), _ptr(lengths), len(lengths), _ptr(starts), starts.shape[0] if starts is not None else 1,
                                         stark.num_io, _ptr(ios), _ptr(finals), _ptr(sums), _ptr(infinity)))
    return ios, finals, sums, infinity


def msm_batch_check(stark, public_inputs_per_unit, lengths, starts=None, terms=None):
    """The check of a batch of short MSMs (sbn_msm_batch_check) on the public inputs of its unit proofs: every head starts from the
    start of its segment, every other offset is the output before it (across unit boundaries), the pads repeat the last instance
    and (with `terms`) x and exponents are the caller's.  Returns (finals, sums, infinity) read and recomputed from the outputs;
    raises SbnError(-6) naming the first instance, its segment and the field that breaks.  Verifies NO proof: verify_msms does
    both."""
    xw, ew = _chain_words(stark)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint64).reshape(-1)
    if terms is None:   # only the starts need shaping
        _, _, starts, _, _, curve = _msm_batch_args(stark, np.zeros((1, xw + ew), dtype=np.uint32), lengths[:0], starts)
    else:
        terms, _, starts, _, _, curve = _msm_batch_args(stark, terms, lengths, starts)
    pis, ptrs, n = _unit_public_inputs(stark, public_inputs_per_unit)
    finals, sums, infinity = _msm_batch_outputs(len(lengths), xw, curve)
    _check(lib().sbn_msm_batch_check(stark.kind, stark.num_io, ptrs, n, _ptr(lengths), len(lengths), _ptr(terms), _ptr(starts),
                                     starts.shape[0] if starts is not None else 1, _ptr(finals), _ptr(sums), _ptr(infinity)))
    return finals, sums, infinity


# ---- complete sums: the library picks the start of every segment (include/sbn.h, "Complete sums") ------------------------------
START_CANDIDATES = 8   # SBN_START_CANDIDATES


def start_candidate(stark, j):
    """Start candidate j < START_CANDIDATES of the curve table `stark` (sbn_start_candidate): a fixed point of the table's curve
    with no chosen relation to the generator, as the x words of an `ios` row."""
    if not 0 <= int(j) < 2 ** 32:
        raise SbnError(-1, f"start candidate {j}: there are {START_CANDIDATES}")
    out = np.zeros(_curve_words(stark), dtype=np.uint32)
    _check(lib().sbn_start_candidate(stark.kind, int(j), _ptr(out)))
    return out


def _complete_args(stark, terms, lengths, term_infinity):
    """terms, lengths as msm_batch_instances takes them; term_infinity (M,) bytes or None: a non-zero entry makes that term the
    point at infinity (its words are not read).  Returns (terms, lengths, term_infinity, xw, ew)."""
    if stark.kind not in (AIR_G1_EXP, AIR_G2_EXP):
        raise SbnError(-7, "complete sums cover the curve tables G1ExpStark and G2ExpStark")
    terms, lengths, _, xw, ew, _ = _msm_batch_args(stark, terms, lengths, None)
    if term_infinity is not None:
        term_infinity = np.ascontiguousarray(term_infinity, dtype=np.uint8).reshape(-1)
        if term_infinity.shape[0] != terms.shape[0]:
            raise SbnError(-1, f"term_infinity must hold one byte per term ({terms.shape[0]})")
    return terms, lengths, term_infinity, xw, ew


def _complete_outputs(M, segments, xw, ew):
    """(terms_eff, starts, choice, finals, sums, infinity)"""
    return (np.zeros((M, xw + ew), dtype=np.uint32), np.zeros((segments, xw), dtype=np.uint32), np.zeros(segments, dtype=np.uint8),
            np.zeros((segments, xw), dtype=np.uint32), np.zeros((segments, xw), dtype=np.uint32), np.zeros(segments, dtype=np.uint8))


def msm_batch_instances_complete(stark, terms, lengths, term_infinity=None):
    """msm_batch_instances on the two curve tables with the start of every segment picked by the library, so that no valid input
    is refused (sbn_msm_batch_instances_complete).  Returns (ios, terms_eff, starts, choice, finals, sums, infinity): terms_eff are
    the terms with (generator, exponent 0) for the masked ones, starts[s] = start_candidate(stark, choice[s]), and the rest is what
    msm_batch_instances(stark, terms_eff, lengths, starts) returns.  No device needed."""
    terms, lengths, term_infinity, xw, ew = _complete_args(stark, terms, lengths, term_infinity)
    if stark.num_io < 1:
        raise SbnError(-1, "the table has no instances")
    units = msm_num_units(terms.shape[0], stark.num_io)
    ios = np.zeros((units, stark.num_io, 2 * xw + ew), dtype=np.uint32)
    eff, starts, choice, finals, sums, infinity = _complete_outputs(terms.shape[0], len(lengths), xw, ew)
    _check(lib().sbn_msm_batch_instances_complete(stark.kind, _ptr(terms), _ptr(term_infinity), _ptr(lengths), len(lengths), stark.num_io, _ptr(ios),
                                                  _ptr(eff), _ptr(starts), _ptr(choice), _ptr(finals), _ptr(sums), _ptr(infinity)))
    return ios, eff, starts, choice, finals, sums, infinity


# ---- field powers and power towers (include/sbn.h, "Field powers") -------------------------------------------------------------
BN_P = 21888242871839275222246405745257275088696311157297823662689037894645226208583   # the base field of BN254
BN_X = 4965661367192848881                # the BN parameter x = 0x44E992B44A6909F1 (sbn_bn_x): p, r and the final exponentiation are polynomials in it
FQ_INVERSE_EXP = BN_P - 2                 # x^(p-2) = 1/x for x != 0 (and 0 for x = 0)
FQ_LEGENDRE_EXP = (BN_P - 1) // 2         # 1 for a non-zero square, p - 1 for a non-residue, 0 for 0
FQ_SQRT_EXP = (BN_P + 1) // 4             # a square root of x when x is a square: valid because p = 3 mod 4 (check with fq_sqrt_flags)


def _power_words(stark):
    """(u32 words of a field element, of the exponent) in an instance row of the field Exp table `stark`."""
    if getattr(stark, "kind", None) not in (AIR_FQ_EXP, AIR_FQ12_EXP, AIR_FQ12_EXP_U64):
        raise SbnError(-7, "field powers cover the field tables FqExpStark, Fq12ExpStark and Fq12ExpU64Stark")
    return _EXP_IO_WORDS[stark.kind]


def _int_limbs(v, n):
    if v < 0 or v >> (32 * n):
        raise SbnError(-1, f"{v} does not fit {32 * n} bits")
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def _power_args(stark, bases, exps, depth):
    """bases (count, W) uint32, or Python ints for FqExpStark; exps (count, ew) uint32, or (ew,) / (1, ew) / one Python int = one
    exponent shared by every tower, or a list of Python ints = one per tower (little-endian u32 limbs); depth >= 1."""
    w, ew = _power_words(stark)
    if w == 8 and not isinstance(bases, np.ndarray) and len(bases) and all(isinstance(b, int) for b in bases):
        bases = [_int_limbs(b, 8) for b in bases]
    bases = np.ascontiguousarray(bases, dtype=np.uint32)
    if isinstance(exps, int):
        exps = _int_limbs(exps, ew)
    elif not isinstance(exps, np.ndarray) and len(exps) and all(isinstance(e, int) for e in exps) and len(exps) != ew:
        exps = [_int_limbs(e, ew) for e in exps]
    exps = np.ascontiguousarray(exps, dtype=np.uint32)
    if exps.ndim == 1:
        exps = exps.reshape(1, -1)
    if bases.ndim != 2 or bases.shape[0] < 1 or bases.shape[1] != w or exps.ndim != 2 or exps.shape[1] != ew:
        raise SbnError(-1, f"bases must be [count][{w}] u32 and exps [count][{ew}] or [{ew}] u32")
    if int(depth) < 1:
        raise SbnError(-1, "depth must be >= 1")
    return bases, exps, int(depth), w, ew


def bn_x():
    """The BN parameter as the library states it (sbn_bn_x); equals BN_X."""
    out = np.zeros(2, dtype=np.uint32)
    _check(lib().sbn_bn_x(_ptr(out)))
    return int(out[0]) | (int(out[1]) << 32)


def power_instances(stark, bases, exps, depth=1):
    """Powers and power towers as instances of the field Exp table `stark` (sbn_power_instances): `count` towers of `depth`
    consecutive instances, offset one, level 0 x = base, level l x = the output of level l - 1, every level with the tower's
    exponent; the last unit is padded with copies of the last instance.  Returns (ios_units, powers): (units, num_io, words per
    instance) uint32 as BatchProver.prove_ios takes it and the outputs (count, depth, W) uint32, powers[k][l] = base_k^(e^(l+1)).
    Exponents are never reduced.  No device needed."""
    bases, exps, depth, w, ew = _power_args(stark, bases, exps, depth)
    count = bases.shape[0]
    if stark.num_io < 1:
        raise SbnError(-1, "the table has no instances")
    units = msm_num_units(count * depth, stark.num_io)
    ios = np.zeros((units, stark.num_io, 2 * w + ew), dtype=np.uint32)
    powers = np.zeros((count, depth, w), dtype=np.uint32)
    _check(lib().sbn_power_instances(stark.kind, _ptr(bases), _ptr(exps), exps.shape[0], count, depth, stark.num_io, _ptr(ios), _ptr(powers)))
    return ios, powers


def power_check(stark, public_inputs_per_unit, bases, exps, depth=1):
    """The check of a batch of powers / power towers (sbn_power_check) on the public inputs of its unit proofs: offsets are one,
    exponents the caller's, level 0 starts from the caller's base and level l from the output of level l - 1 (across units), the
    pads repeat the last instance, every output is a field element.  Returns the powers (count, depth, W); raises SbnError(-6)
    naming the first instance and field that breaks.  Verifies NO proof: verify_powers does both."""
    bases, exps, depth, w, ew = _power_args(stark, bases, exps, depth)
    count = bases.shape[0]
    pis, ptrs, n = _unit_public_inputs(stark, public_inputs_per_unit)
    powers = np.zeros((count, depth, w), dtype=np.uint32)
    _check(lib().sbn_power_check(stark.kind, stark.num_io, ptrs, n, count, depth, _ptr(bases), _ptr(exps), exps.shape[0], _ptr(powers)))
    return powers


# ---- field programs (include/sbn.h, "Field programs") ---------------------------------------------------------------------------
NODE_OUTPUT = 0x80000000    # x / offset = NODE_OUTPUT | j: the output of node j, j < this node's index
NODE_ONE = 0x7FFFFFFF       # offset only: the field's one


def _program_args(stark, nodes, values, exps):
    """nodes (count, 3) uint32 = (x, offset, exp) per node, or (count, 4) with the maps of a mapped program as the fourth word
    (_program_fn picks the call); values (n_values, W) uint32, or Python ints for FqExpStark; exps
    (n_exps, ew) uint32 or a list of Python ints (little-endian u32 limbs)."""
    w, ew = _power_words(stark)
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
    if w == 8 and not isinstance(values, np.ndarray) and len(values) and all(isinstance(v, int) for v in values):
        values = [_int_limbs(v, 8) for v in values]
    values = np.ascontiguousarray(values, dtype=np.uint32)
    if not isinstance(exps, np.ndarray) and len(exps) and all(isinstance(e, int) for e in exps):
        exps = [_int_limbs(e, ew) for e in exps]
    exps = np.ascontiguousarray(exps, dtype=np.uint32)
    if nodes.ndim != 2 or nodes.shape[1] not in (3, 4) or values.ndim != 2 or values.shape[1] != w or exps.ndim != 2 or exps.shape[1] != ew:
        raise SbnError(-1, f"nodes must be [count][3] (or [count][4] with maps), values [n_values][{w}] and exps [n_exps][{ew}] u32")
    return nodes, values, exps, w, ew


def _program_fn(nodes, name):
    """The C call `name` for a node table: (count, 4) nodes, which carry maps, take its sbn_*program_m* twin."""
    if nodes.shape[1] == 4:
        name = name + "_m" if name.endswith("_program") else name.replace("sbn_program_", "sbn_program_m_")
    return getattr(lib(), name)


def program_levels(nodes):
    """The schedule of a program (sbn_program_levels): (level, depth), level[g] = 0 for a node without links, otherwise 1 + the
    largest level of the nodes it links to; depth = 1 + the largest level.  Structure only; no device needed."""
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
    if nodes.ndim != 2 or nodes.shape[1] not in (3, 4):
        raise SbnError(-1, "nodes must be [count][3] u32 (or [count][4] with maps)")
    level = np.zeros(nodes.shape[0], dtype=np.uint32)
    depth = C.c_uint32(0)
    _check(_program_fn(nodes, "sbn_program_levels")(_ptr(nodes), nodes.shape[0], _ptr(level), C.addressof(depth)))
    return level, int(depth.value)


def program_instances(stark, nodes, values, exps):
    """A program as instances of the field Exp table `stark` (sbn_program_instances): node g is instance g, x and offset each a
    literal of `values` or NODE_OUTPUT | j, the output of an earlier node (offset also NODE_ONE), the exponent an entry of `exps`;
    the last unit is padded with copies of the last instance.  Returns (ios_units, outs): (units, num_io, words per instance)
    uint32 as BatchProver.prove_ios takes it and the outputs (count, W) uint32.  Exponents are never reduced.  No device needed."""
    nodes, values, exps, w, ew = _program_args(stark, nodes, values, exps)
    count = nodes.shape[0]
    if stark.num_io < 1:
        raise SbnError(-1, "the table has no instances")
    units = msm_num_units(count, stark.num_io)
    ios = np.zeros((units, stark.num_io, 2 * w + ew), dtype=np.uint32)
    outs = np.zeros((count, w), dtype=np.uint32)
    _check(_program_fn(nodes, "sbn_program_instances")(stark.kind, _ptr(nodes), count, _ptr(values), values.shape[0], _ptr(exps), exps.shape[0], stark.num_io,
                                       _ptr(ios), _ptr(outs)))
    return ios, outs


def program_check(stark, public_inputs_per_unit, nodes, values, exps):
    """The check of a program (sbn_program_check) on the public inputs of its unit proofs: literals, ones and exponents are the
    caller's, a linked x or offset equals the output of the node it links to (across units), the pads repeat the last instance,
    every output is a field element.  Returns the outputs (count, W); raises SbnError(-6) naming the first instance and field
    that breaks.  Verifies NO proof: verify_program does both."""
    nodes, values, exps, w, ew = _program_args(stark, nodes, values, exps)
    pis, ptrs, n = _unit_public_inputs(stark, public_inputs_per_unit)
    outs = np.zeros((nodes.shape[0], w), dtype=np.uint32)
    _check(_program_fn(nodes, "sbn_program_check")(stark.kind, stark.num_io, ptrs, n, _ptr(nodes), nodes.shape[0], _ptr(values), values.shape[0],
                                   _ptr(exps), exps.shape[0], _ptr(outs)))
    return outs


class Program:
    """A small builder of programs for the field Exp table `stark`.  value(v) and pow / mul / pow_big return handles; a handle or a
    literal (W uint32 words; a Python int for FqExpStark) is accepted wherever an operand is.  Equal literals share one slot of
    `values`, equal exponents one slot of `exps`.  arrays() gives (nodes, values, exps) as program_instances,
    Prover.generate_trace_program, BatchProver.prove_program and verify_program take them; a node handle h is node h.node.
    On the Fq12 tables frobenius(h, m) and conj(h) give the handle of h^(p^m): a mapped link (include/sbn.h, "Mapped links and the
    final exponentiation") when h is a node, a new literal when h is one."""

    class Handle:
        __slots__ = ("ref", "node", "map")

        def __init__(self, ref, node=None, map=0):
            self.ref, self.node, self.map = ref, node, map

    def __init__(self, stark):
        self.stark = stark
        self.w, self.ew = _power_words(stark)
        self.limb_bits = 32 * self.ew - 1   # Horner limbs of pow_big: 2^limb_bits is itself a legal exponent (255, or 63 for the u64 table)
        self._values, self._value_slot, self._exps, self._exp_slot, self._nodes = [], {}, [], {}, []

    def value(self, v):
        """A literal: W uint32 words (a Python int for FqExpStark).  Equal literals share one slot."""
        if isinstance(v, Program.Handle):
            return v
        words = _int_limbs(v, 8) if self.w == 8 and isinstance(v, int) else [int(t) for t in np.asarray(v).reshape(-1)]
        if len(words) != self.w:
            raise SbnError(-1, f"a literal has {self.w} u32 words")
        key = tuple(words)
        if key not in self._value_slot:
            self._value_slot[key] = len(self._values)
            self._values.append(words)
        return Program.Handle(self._value_slot[key])

    def _exp(self, e):
        key = tuple(_int_limbs(int(e), self.ew)) if isinstance(e, (int, np.integer)) else tuple(int(t) for t in np.asarray(e).reshape(-1))
        if len(key) != self.ew:
            raise SbnError(-1, f"an exponent has {self.ew} u32 words")
        if key not in self._exp_slot:
            self._exp_slot[key] = len(self._exps)
            self._exps.append(list(key))
        return self._exp_slot[key]

    def pow(self, x, e, offset=None):
        """The node offset * x^e (offset None: one); e a Python int that fits the exponent field, or its ew words."""
        x = self.value(x)
        off = Program.Handle(NODE_ONE) if offset is None else self.value(offset)
        self._nodes.append((x.ref, off.ref, self._exp(e), x.map | (off.map << 8)))
        g = len(self._nodes) - 1
        return Program.Handle(NODE_OUTPUT | g, g)

    def frobenius(self, h, m):
        """h^(p^m), the Frobenius map m of an Fq12 operand; maps compose mod 12.  On a node handle the map rides on the link (it costs
        no node); on a literal it is applied here (fq12_frobenius) and the result interned as a literal."""
        if self.w != 96:
            raise SbnError(-7, "a Frobenius map is an Fq12 notion: Fq12ExpStark and Fq12ExpU64Stark")
        h, m = self.value(h), int(m) % 12
        if h.ref & NODE_OUTPUT:
            return Program.Handle(h.ref, h.node, (h.map + m) % 12)
        if h.ref == NODE_ONE or m == 0:
            return h
        return self.value(fq12_frobenius(self._values[h.ref], m))

    def conj(self, h):
        """The conjugate h^(p^6)."""
        return self.frobenius(h, 6)

    def mul(self, a, b):
        """The product a * b: pow(a, 1, offset=b)."""
        return self.pow(a, 1, offset=b)

    def pow_big(self, x, e):
        """x^e for a Python int e >= 0 of any length, by Horner over limbs of limb_bits bits, most significant first: the first
        limb is one node, every further limb two (acc^(2^limb_bits), then x^limb with offset = acc).  A zero limb still emits
        its nodes, so the node count depends on the bit length of e alone."""
        e = int(e)
        if e < 0:
            raise SbnError(-1, "the exponent must be >= 0")
        x = self.value(x)
        b = self.limb_bits
        limbs = [(e >> (b * i)) & ((1 << b) - 1) for i in range(max(1, -(-e.bit_length() // b)))]
        acc = self.pow(x, limbs[-1])
        for limb in reversed(limbs[:-1]):
            acc = self.pow(x, limb, offset=self.pow(acc, 1 << b))
        return acc

    def __len__(self):
        return len(self._nodes)

    def arrays(self):
        """(nodes (count, 3), values (n_values, W), exps (n_exps, ew)), uint32; nodes (count, 4), the maps as the fourth word, when
        some link carries a map."""
        nodes = np.array(self._nodes, dtype=np.uint32).reshape(-1, 4)
        if not nodes[:, 3].any():
            nodes = np.ascontiguousarray(nodes[:, :3])
        return (nodes, np.array(self._values, dtype=np.uint32).reshape(-1, self.w), np.array(self._exps, dtype=np.uint32).reshape(-1, self.ew))


# ---- mapped links and the final exponentiation (include/sbn.h, "Mapped links and the final exponentiation") -----------------------
FINAL_EXP_NODES = 16        # SBN_FINAL_EXP_NODES
_FQ12_ONE = np.array([1] + [0] * 95, dtype=np.uint32)


def _fq12_words(f):
    f = np.ascontiguousarray(f, dtype=np.uint32).reshape(-1)
    if f.shape[0] != 96:
        raise SbnError(-1, "an Fq12 element has 96 u32 words")
    return f


def fq12_frobenius(f, m):
    """f^(p^m) for an Fq12 element in the flat basis (96 u32 words), m in 0 .. 11 (sbn_fq12_frobenius).  No device needed."""
    f, out = _fq12_words(f), np.zeros(96, dtype=np.uint32)
    if not 0 <= int(m) <= 0xFFFFFFFF:
        raise SbnError(-1, "a Frobenius map is 0 .. 11")
    _check(lib().sbn_fq12_frobenius(_ptr(f), int(m), _ptr(out)))
    return out


def fq12_conjugate(f):
    """The conjugate f^(p^6)."""
    return fq12_frobenius(f, 6)


def fq12_inverse(f):
    """f^-1 in Fq12 (sbn_fq12_inverse); zero is refused.  No device needed."""
    f, out = _fq12_words(f), np.zeros(96, dtype=np.uint32)
    _check(lib().sbn_fq12_inverse(_ptr(f), _ptr(out)))
    return out


def final_exponentiation(pg, f, f_inv=None):
    """Appends the FINAL_EXP_NODES = 16 nodes of the final exponentiation f -> f^((p^12 - 1) / r) to the program `pg` on
    Fq12ExpU64Stark, by the node table of include/sbn.h.  f: 96 u32 words; f_inv (default fq12_inverse(f)) is a claim the first node
    checks.  Returns (check, result) handles: the output of `check` must be one, the output of `result` is the value."""
    if getattr(pg.stark, "kind", None) != AIR_FQ12_EXP_U64:
        raise SbnError(-1, "the final exponentiation is a program of Fq12ExpU64Stark")
    f = _fq12_words(f)
    fi = pg.value(fq12_inverse(f) if f_inv is None else _fq12_words(f_inv))
    fv, F, cj = pg.value(f), pg.frobenius, pg.conj
    check = pg.pow(fi, 1, offset=fv)                        # 0
    n1 = pg.pow(fi, 1, offset=cj(fv))                       # 1
    e = pg.pow(n1, 1, offset=F(n1, 2))                      # 2: the easy part
    fx = pg.pow(e, BN_X)                                    # 3
    fx2 = pg.pow(fx, BN_X)                                  # 4
    fx3 = pg.pow(fx2, BN_X)                                 # 5
    n6 = pg.pow(F(e, 2), 1, offset=F(e, 1))                 # 6
    n7 = pg.pow(F(e, 3), 1, offset=n6)                      # 7
    n8 = pg.pow(F(fx2, 1), 1, offset=fx)                    # 8
    n9 = pg.pow(F(fx3, 1), 1, offset=fx3)                   # 9
    acc = pg.pow(cj(e), 2, offset=n7)                       # 10
    acc = pg.pow(F(fx2, 2), 6, offset=acc)                  # 11
    acc = pg.pow(F(fx, 7), 12, offset=acc)                  # 12
    acc = pg.pow(cj(n8), 18, offset=acc)                    # 13
    acc = pg.pow(cj(fx2), 30, offset=acc)                   # 14
    return check, pg.pow(cj(n9), 36, offset=acc)            # 15


def _final_exp_program(stark, fs, f_invs):
    fs = np.ascontiguousarray(fs, dtype=np.uint32).reshape(-1, 96)
    if f_invs is not None:
        f_invs = np.ascontiguousarray(f_invs, dtype=np.uint32).reshape(-1, 96)
        if f_invs.shape[0] != fs.shape[0]:
            raise SbnError(-1, "one f_inv per f")
    pg = Program(stark)
    for t in range(fs.shape[0]):
        final_exponentiation(pg, fs[t], None if f_invs is None else f_invs[t])
    return pg.arrays()


def verify_final_exponentiations(stark, config, proofs, fs, verifier=None):
    """Verifies the unit proofs of BatchProver.prove_final_exponentiations (host verifier, or a Verifier of the table in batches),
    reads the inverse of input t from the x public inputs of node 16 t, runs program_check on the program rebuilt from `fs` and
    those inverses, and requires the output of every node 16 t to be one.  Returns the results (count, 96); raises SbnError
    naming the unit, the instance and field, or the input whose inverse is none."""
    proofs = list(proofs)
    fs = np.ascontiguousarray(fs, dtype=np.uint32).reshape(-1, 96)
    _verify_units(stark, config, proofs, verifier)
    pis = [np.asarray(p.public_inputs(), dtype=np.uint64) for p in proofs]
    if len(pis) != msm_num_units(FINAL_EXP_NODES * fs.shape[0], stark.num_io):
        raise SbnError(-6, f"{len(pis)} units given, {fs.shape[0]} final exponentiations have {msm_num_units(FINAL_EXP_NODES * fs.shape[0], stark.num_io)}")
    f_invs = np.zeros_like(fs)
    for t in range(fs.shape[0]):
        g = FINAL_EXP_NODES * t
        x = pis[g // stark.num_io].reshape(stark.num_io, -1)[g % stark.num_io, :192]   # 16-bit limbs, low first
        if (x >> np.uint64(16)).any():
            raise SbnError(-6, f"input {t}: an x limb of instance {g} is out of range")
        f_invs[t] = (x[0::2] | (x[1::2] << np.uint64(16))).astype(np.uint32)
    nodes, values, exps = _final_exp_program(stark, fs, f_invs)
    outs = program_check(stark, pis, nodes, values, exps)
    for t in range(fs.shape[0]):
        if not np.array_equal(outs[FINAL_EXP_NODES * t], _FQ12_ONE):
            raise SbnError(-6, f"input {t}: f * f_inv is not one (the output of node {FINAL_EXP_NODES * t}), so the x of that node is no inverse of f")
    return outs[FINAL_EXP_NODES - 1::FINAL_EXP_NODES].copy()


# ---- curve programs (include/sbn.h, "Curve programs") ---------------------------------------------------------------------------
NODE_START = 0x7FFFFFFE     # offset only, curve programs: the start the library picks (one per program)


def _curve_program_args(stark, nodes, points, exps):
    """nodes (count, 3) uint32 = (x, offset, exp) per node; points (n_points, W) uint32; exps (n_exps, 8) uint32 or a list of Python
    ints (256 bits, never reduced)."""
    if getattr(stark, "kind", None) not in (AIR_G1_EXP, AIR_G2_EXP):
        raise SbnError(-7, "curve programs cover the curve tables G1ExpStark and G2ExpStark")
    w = _curve_words(stark)
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
    points = np.ascontiguousarray(points, dtype=np.uint32)
    if not isinstance(exps, np.ndarray) and len(exps) and all(isinstance(e, int) for e in exps):
        exps = [_int_limbs(e, 8) for e in exps]
    exps = np.ascontiguousarray(exps, dtype=np.uint32)
    if nodes.ndim != 2 or nodes.shape[1] != 3 or points.ndim != 2 or points.shape[1] != w or exps.ndim != 2 or exps.shape[1] != 8:
        raise SbnError(-1, f"nodes must be [count][3], points [n_points][{w}] and exps [n_exps][8] u32")
    return nodes, points, exps, w


def _curve_program_outputs(count, w):
    """(outs, values, infinity, choice)"""
    return np.zeros((count, w), dtype=np.uint32), np.zeros((count, w), dtype=np.uint32), np.zeros(count, dtype=np.uint8), np.zeros(1, dtype=np.uint8)


def curve_program_instances(stark, nodes, points, exps):
    """A program as instances of the curve table `stark` (sbn_curve_program_instances): node g is instance g = offset + e x, x a
    literal of `points` or NODE_OUTPUT | j, offset a literal, NODE_OUTPUT | j or NODE_START, the start the library picks (the
    smallest start_candidate from which no node has a bad event).  Returns (ios_units, outs, values, infinity, choice): the explicit
    padded list as BatchProver.prove_ios takes it, the table outputs (count, W), the values out + (-blind) with their flags (1: the
    point at infinity, words zero) and the candidate chosen.  No device needed."""
    nodes, points, exps, w = _curve_program_args(stark, nodes, points, exps)
    count = nodes.shape[0]
    if stark.num_io < 1:
        raise SbnError(-1, "the table has no instances")
    units = msm_num_units(count, stark.num_io)
    ios = np.zeros((units, stark.num_io, 2 * w + 8), dtype=np.uint32)
    outs, values, infinity, choice = _curve_program_outputs(count, w)
    _check(lib().sbn_curve_program_instances(stark.kind, _ptr(nodes), count, _ptr(points), points.shape[0], _ptr(exps), exps.shape[0], stark.num_io,
                                             _ptr(ios), _ptr(outs), _ptr(values), _ptr(infinity), _ptr(choice)))
    return ios, outs, values, infinity, int(choice[0])


def curve_program_check(stark, public_inputs_per_unit, nodes, points, exps, choice):
    """The check of a curve program (sbn_curve_program_check) on the public inputs of its unit proofs: literals and exponents are
    the caller's, a NODE_START offset is start candidate `choice`, a linked x or offset equals the output of the node it links to
    (across units), the pads repeat the last instance, every output is a point of the curve.  Returns (outs, values, infinity), the
    values from the blinds recomputed from `choice` and the exponents; raises SbnError(-6) naming the first instance and field that
    breaks.  Verifies NO proof: verify_curve_program does both."""
    nodes, points, exps, w = _curve_program_args(stark, nodes, points, exps)
    pis, ptrs, n = _unit_public_inputs(stark, public_inputs_per_unit)
    outs, values, infinity, _ = _curve_program_outputs(nodes.shape[0], w)
    if not 0 <= int(choice) < 2 ** 32:
        raise SbnError(-1, f"choice {choice}: there are {START_CANDIDATES} start candidates")
    _check(lib().sbn_curve_program_check(stark.kind, stark.num_io, ptrs, n, _ptr(nodes), nodes.shape[0], _ptr(points), points.shape[0],
                                         _ptr(exps), exps.shape[0], int(choice), _ptr(outs), _ptr(values), _ptr(infinity)))
    return outs, values, infinity


class CurveProgram:
    """A small builder of programs for the curve table `stark`.  point(P) and mul / add / lincomb return handles; a handle or a
    literal point (W uint32 words) is accepted wherever an operand is.  Equal literals share one slot of `points`, equal exponents
    one slot of `exps`.  arrays() gives (nodes, points, exps) as curve_program_instances, Prover.generate_trace_curve_program,
    BatchProver.prove_curve_program and verify_curve_program take them; a node handle h is node h.node, and values[h.node] of those
    calls is the point the handle stands for."""

    START = Program.Handle(NODE_START)

    def __init__(self, stark):
        self.stark = stark
        self.w = _curve_words(stark)
        self._points, self._point_slot, self._exps, self._exp_slot, self._nodes = [], {}, [], {}, []

    def point(self, p):
        """A literal point: W uint32 words.  Equal literals share one slot."""
        if isinstance(p, Program.Handle):
            return p
        key = tuple(int(t) for t in np.asarray(p).reshape(-1))
        if len(key) != self.w:
            raise SbnError(-1, f"a point has {self.w} u32 words")
        if key not in self._point_slot:
            self._point_slot[key] = len(self._points)
            self._points.append(list(key))
        return Program.Handle(self._point_slot[key])

    def _exp(self, e):
        key = tuple(_int_limbs(int(e), 8)) if isinstance(e, (int, np.integer)) else tuple(int(t) for t in np.asarray(e).reshape(-1))
        if len(key) != 8:
            raise SbnError(-1, "an exponent has 8 u32 words")
        if key not in self._exp_slot:
            self._exp_slot[key] = len(self._exps)
            self._exps.append(list(key))
        return self._exp_slot[key]

    def mul(self, x, e, offset=START):
        """The node offset + e x (offset START: the value of the node is e x); e a Python int below 2^256, or its 8 words."""
        x = self.point(x)
        if x.ref == NODE_START:
            raise SbnError(-1, "START is an offset, not an x")
        self._nodes.append((x.ref, self.point(offset).ref, self._exp(e)))
        g = len(self._nodes) - 1
        return Program.Handle(NODE_OUTPUT | g, g)

    def add(self, a, b):
        """The sum a + b: mul(b, 1, offset=a)."""
        return self.mul(b, 1, offset=a)

    def lincomb(self, terms):
        """The sum of e x over terms = [(e, x), ...], one node per term, each continuing from the one before it."""
        acc = CurveProgram.START
        for e, x in terms:
            acc = self.mul(x, e, offset=acc)
        if acc is CurveProgram.START:
            raise SbnError(-1, "no term")
        return acc

    def __len__(self):
        return len(self._nodes)

    def arrays(self):
        """(nodes (count, 3), points (n_points, W), exps (n_exps, 8)), uint32."""
        return (np.array(self._nodes, dtype=np.uint32).reshape(-1, 3), np.array(self._points, dtype=np.uint32).reshape(-1, self.w),
                np.array(self._exps, dtype=np.uint32).reshape(-1, 8))


def fq_sqrt_flags(xs, roots):
    """Per element, whether root^2 == x in Fq: what a caller of FqExpStark with FQ_SQRT_EXP checks, because x^((p+1)/4) is a square
    root only when x is a square (a non-residue gives a root of -x: not an error, the flag is False).  xs, roots: Python ints or
    (count, 8) uint32 limbs.  Returns a (count,) bool array."""
    def ints(v):
        if isinstance(v, np.ndarray):
            return [sum(int(w) << (32 * i) for i, w in enumerate(row)) for row in v.reshape(-1, 8)]
        return [int(x) for x in v]
    xs, roots = ints(xs), ints(roots)
    if len(xs) != len(roots):
        raise SbnError(-1, "xs and roots differ in length")
    return np.array([x < BN_P and r < BN_P and r * r % BN_P == x for x, r in zip(xs, roots)], dtype=bool)


class Proof:
    """StarkProofWithPublicInputs as canonical proof words (layout: include/sbn.h)."""

    def __init__(self, words, degree_bits):
        self.words = words
        self.degree_bits = degree_bits

    def to_bytes(self):
        return self.words.astype("<u8").tobytes()

    def recover_degree_bits(self, config=None):
        return self.degree_bits

    def public_inputs(self):
        """The public inputs the proof carries: the last n_public_inputs words (header word 5)."""
        n = int(self.words[5])
        return self.words[len(self.words) - n:]

    def fields(self):
        """The proof as the reference's struct tree (starky proof.rs `StarkProof` / `StarkOpeningSet`, plonky2
        fri/proof.rs `FriProof`): a dict of numpy views into the words, read in the order include/sbn.h documents.
        The Rust shim's `proof_from_words` (integration/rust/starky-bn254-amd/src/convert.rs) reads the same way."""
        w = self.words
        if len(w) < 12 or int(w[0]) != 0x31564F5250424E53:
            raise ValueError("not a proof of this library")
        (degree_bits, ncol, nz, nq, npi, cap_h, rate_bits, nlayers, arity_bits, fpl, nqueries) = (int(x) for x in w[1:12])
        pos = [12]

        def take(n, shape=None):
            if pos[0] + n > len(w):
                raise ValueError("proof words truncated")
            v = w[pos[0]:pos[0] + n]
            pos[0] += n
            return v.reshape(shape) if shape else v

        capn, lde_bits = 1 << cap_h, degree_bits + rate_bits
        out = {"degree_bits": degree_bits, "trace_cap": take(4 * capn, (capn, 4))}
        out["permutation_zs_cap"] = take(4 * capn, (capn, 4)) if nz else None
        out["quotient_polys_cap"] = take(4 * capn, (capn, 4))
        op = {"local_values": take(2 * ncol, (ncol, 2)), "next_values": take(2 * ncol, (ncol, 2))}
        op["permutation_zs"] = take(2 * nz, (nz, 2)) if nz else None
        op["permutation_zs_next"] = take(2 * nz, (nz, 2)) if nz else None
        op["quotient_polys"] = take(2 * nq, (nq, 2))
        out["openings"] = op
        fri = {"commit_phase_merkle_caps": [take(4 * capn, (capn, 4)) for _ in range(nlayers)], "query_round_proofs": []}
        widths = [ncol] + ([nz] if nz else []) + [nq]
        for _ in range(nqueries):
            initial = [(take(wd), take(4 * (lde_bits - cap_h), (lde_bits - cap_h, 4))) for wd in widths]
            steps, bits = [], lde_bits
            for _ in range(nlayers):
                evals = take(2 << arity_bits, (1 << arity_bits, 2))
                bits -= arity_bits
                steps.append({"evals": evals, "merkle_proof": take(4 * (bits - cap_h), (bits - cap_h, 4))})
            fri["query_round_proofs"].append({"initial_trees_proof": initial, "steps": steps})
        fri["final_poly"] = take(2 * fpl, (fpl, 2))
        fri["pow_witness"] = int(take(1)[0])
        out["opening_proof"] = fri
        out["public_inputs"] = take(npi)
        if pos[0] != len(w):
            raise ValueError("trailing words after the proof")
        return out


def _take_proof(h):
    L = lib()
    n = L.sbn_proof_num_words(h)
    words = np.ctypeslib.as_array(L.sbn_proof_words(h), shape=(n,)).copy()
    db = L.sbn_proof_degree_bits(h)
    L.sbn_proof_free(h)
    return Proof(words, db)


def settings_check():
    """The SBN_* switches of this process as a prover created now would resolve them (csrc/settings.hpp), as a dict of strings;
    raises SbnError(-1) naming a value that is not understood.  Needs no device."""
    buf = C.create_string_buffer(1024)
    _check(lib().sbn_settings_check(buf, 1024))
    return dict(kv.partition("=")[::2] for kv in buf.value.decode().split(" "))


def fixed_columns_range(stark):
    """The shape-constant columns [first, end) of a table (sbn_fixed_columns_range): the words a trace of this shape holds there do
    not depend on the instances, and a Prover transforms them once.  (0, 0) for the tables without any.  Needs no device."""
    f0, f1 = C.c_uint32(0), C.c_uint32(0)
    _check(lib().sbn_fixed_columns_range(C.byref(stark._d), C.byref(f0), C.byref(f1)))
    return int(f0.value), int(f1.value)


def fixed_columns_check(stark, degree_bits, block):
    """Does `block`, the columns fixed_columns_range(stark) of a trace of 2^degree_bits rows, hold the generators' words?  The
    comparison Prover.load_trace runs, on the device (sbn_fixed_columns_check)."""
    f0, f1 = fixed_columns_range(stark)
    block = np.ascontiguousarray(block, dtype=np.uint64)
    if block.shape != (f1 - f0, 1 << degree_bits):
        raise SbnError(-1, "block shape does not match the table's shape-constant columns")
    match = C.c_int(0)
    _check(lib().sbn_fixed_columns_check(C.byref(stark._d), degree_bits, _ptr(block), C.byref(match)))
    return bool(match.value)


_NO_ROW = (1 << 64) - 1   # UINT64_MAX: "no such row" in the reports of the trace diagnostics


class TraceReport:
    """What Prover.check_trace / check_trace_host found (sbn_trace_report): which rows of the trace break a constraint, by
    segment (air_head, air_tail, perm_lo, perm_hi).  A debugging aid, not a soundness statement (include/sbn.h).
    first_failing_row and the segments' first rows are None when nothing fails; row_flags is the uint8 array of per-row
    segment bits, or None when it was not asked for."""

    def __init__(self, raw, row_flags, rows_per_instance=None):
        self.rows, self.failing_rows = int(raw.rows), int(raw.failing_rows)
        self.first_failing_row = None if raw.first_failing_row == _NO_ROW else int(raw.first_failing_row)
        self.num_zs, self.z_split = int(raw.num_zs), int(raw.z_split)
        self.segments = [{"name": lib().sbn_trace_segment_name(s).decode(), "failing_rows": int(raw.seg_failing_rows[s]),
                          "first_row": None if raw.seg_first_row[s] == _NO_ROW else int(raw.seg_first_row[s])}
                         for s in range(int(raw.num_segments))]
        self.row_flags = row_flags
        self.rows_per_instance = rows_per_instance   # Exp and Flag tables: rows of one instance; else None

    @property
    def ok(self):
        return self.failing_rows == 0

    def failing_instances(self):
        """Exp tables: the instances (row // rows_per_instance) with a failing row, ascending.  Every one of them with
        flags=True; without the flags only what the report itself names (the first failing row of each segment)."""
        if self.rows_per_instance is None:
            raise ValueError("this table has no instances")
        if self.row_flags is not None:
            return [int(k) for k in np.unique(np.nonzero(self.row_flags)[0] // self.rows_per_instance)]
        firsts = [s["first_row"] for s in self.segments if s["first_row"] is not None]
        return sorted({r // self.rows_per_instance for r in firsts})

    def _where(self, row):
        if self.rows_per_instance is None:
            return f"row {row}"
        return f"row {row} (instance {row // self.rows_per_instance}, row {row % self.rows_per_instance} of {self.rows_per_instance})"

    def __str__(self):
        if self.ok:
            return f"ok: all {self.rows} rows satisfy the constraints"
        names = ", ".join(s["name"] for s in self.segments if s["first_row"] == self.first_failing_row)
        return f"{self._where(self.first_failing_row)}: {names}; {self.failing_rows} row{'s' if self.failing_rows != 1 else ''} fail"

    def __repr__(self):
        return f"<TraceReport {self}>"

    def __eq__(self, other):
        if not isinstance(other, TraceReport):
            return NotImplemented
        same_flags = (self.row_flags is None) == (other.row_flags is None) and (self.row_flags is None or np.array_equal(self.row_flags, other.row_flags))
        return same_flags and (self.rows, self.failing_rows, self.first_failing_row, self.num_zs, self.z_split, self.segments) == \
            (other.rows, other.failing_rows, other.first_failing_row, other.num_zs, other.z_split, other.segments)


def _rows_per_instance(stark):
    if stark.kind in (AIR_G1_EXP, AIR_G2_EXP, AIR_FQ12_EXP, AIR_FQ_EXP, AIR_FLAGS):
        return 512
    return 128 if stark.kind in (AIR_FQ12_EXP_U64, AIR_FLAGS_U64) else None


def check_trace_host(stark, trace, public_inputs, seed=0, flags=False):
    """Which rows of `trace` break a constraint of `stark`, on host threads (no device): sbn_check_trace_host.  The same
    TraceReport, for the same seed, as Prover.check_trace gives for the loaded trace."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    n = trace.shape[1] if trace.ndim == 2 else 0
    if trace.ndim != 2 or trace.shape[0] != stark.num_columns or n == 0 or n & (n - 1):
        raise SbnError(-1, "trace shape does not match the table")
    raw = _TraceReport(struct_size=C.sizeof(_TraceReport))
    row_flags = np.zeros(n, dtype=np.uint8) if flags else None
    _check(lib().sbn_check_trace_host(C.byref(stark._d), _ptr(trace), n.bit_length() - 1, _ptr(pi), len(pi), seed, C.byref(raw), _ptr(row_flags)))
    return TraceReport(raw, row_flags, _rows_per_instance(stark))


class ConstraintBlock:
    """One block of a table's constraint stream (sbn_constraint_block): constraints [first, first + count) in emission order,
    the segment of the trace check it belongs to, what it is (section, instance) and the trace columns it is about."""

    def __init__(self, index, raw):
        self.index, self.first, self.count, self.segment = index, int(raw.first), int(raw.count), int(raw.segment)
        self.section = int(raw.section)
        self.name = lib().sbn_constraint_section_name(self.section).decode()
        self.instance = None if raw.instance == 0xFFFFFFFF else int(raw.instance)
        self.col_first, self.col_count = int(raw.col_first), int(raw.col_count)

    def __str__(self):
        s = self.name + (f"[{self.instance}]" if self.instance is not None else "")
        if self.count > 1:
            s += f" [{self.first}, {self.first + self.count})"
        if self.col_count:
            s += f" cols {self.col_first}..{self.col_first + self.col_count}"
        return s

    def __repr__(self):
        return f"<ConstraintBlock {self.index}: {self}>"


def _set_bits(bits, count):
    return [int(i) for i in np.nonzero(np.unpackbits(bits, bitorder="little")[:count])[0]]


class RowExplanation:
    """The blocks and the permutation Z columns one row breaks.  str() reads like a diagnosis."""

    def __init__(self, stark, row, blocks, zs):
        self.stark, self.row, self.blocks, self.zs = stark, row, blocks, zs

    @property
    def ok(self):
        return not self.blocks and not self.zs

    def __str__(self):
        rpi = _rows_per_instance(self.stark)
        where = f"row {self.row}" if rpi is None else f"row {self.row} (instance {self.row // rpi}, row {self.row % rpi} of {rpi})"
        if self.ok:
            return where + ": clean"
        parts = list(dict.fromkeys(str(b) for b in self.blocks))   # (the two constraints of a lookup pair read the same)
        parts += ["Z %d (cols %d, %d)" % ((z,) + self.stark.permutation_pair(z)) for z in self.zs]
        return where + ": " + "; ".join(parts)

    def __repr__(self):
        return f"<RowExplanation {self}>"


class RowsExplanation:
    """What explain_rows found: one RowExplanation per listed row (len, index, iterate), and the raw bitmaps block_flags
    [n_rows][(B + 7) // 8] and z_flags [n_rows][(num_zs + 7) // 8] (bit b of a row's entry, least significant bit first)."""

    def __init__(self, stark, rows, block_flags, z_flags):
        self.stark, self.rows, self.block_flags, self.z_flags = stark, [int(r) for r in rows], block_flags, z_flags

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, k):
        blocks = self.stark.constraint_blocks()
        zs = _set_bits(self.z_flags[k], self.stark.num_permutation_zs())
        return RowExplanation(self.stark, self.rows[k], [blocks[b] for b in _set_bits(self.block_flags[k], len(blocks))], zs)

    def __iter__(self):
        return (self[k] for k in range(len(self)))

    def __str__(self):
        return "\n".join(str(r) for r in self)

    def __eq__(self, other):
        if not isinstance(other, RowsExplanation):
            return NotImplemented
        return self.rows == other.rows and np.array_equal(self.block_flags, other.block_flags) and np.array_equal(self.z_flags, other.z_flags)


class TraceExplanation:
    """What explain_trace found over every row: per block and per Z column the number of failing rows and the first of them.
    block_failing_rows / block_first_row [B] and z_failing_rows / z_first_row [num_zs] are uint64 arrays (first row =
    2^64 - 1 where clean); failing_blocks() / failing_zs() list what fails."""

    def __init__(self, stark, block_stats, z_stats):
        self.stark = stark
        self.block_failing_rows, self.block_first_row = block_stats[:, 0].copy(), block_stats[:, 1].copy()
        self.z_failing_rows, self.z_first_row = z_stats[:, 0].copy(), z_stats[:, 1].copy()

    @property
    def ok(self):
        return not self.block_failing_rows.any() and not self.z_failing_rows.any()

    def failing_blocks(self):
        """[(ConstraintBlock, failing rows, first row)] in stream order."""
        blocks = self.stark.constraint_blocks()
        return [(blocks[b], int(self.block_failing_rows[b]), int(self.block_first_row[b])) for b in np.nonzero(self.block_failing_rows)[0]]

    def failing_zs(self):
        """[(z, failing rows, first row)]."""
        return [(int(z), int(self.z_failing_rows[z]), int(self.z_first_row[z])) for z in np.nonzero(self.z_failing_rows)[0]]

    def __str__(self):
        if self.ok:
            return "ok: no block and no Z column fails on any row"
        plural = lambda k: f"{k:,} row{'s' if k != 1 else ''}"   # noqa: E731
        lines = [f"{b} fails on {plural(k)}, first on row {r}" for b, k, r in self.failing_blocks()]
        lines += ["Z %d (cols %d, %d) fails on %s, first on row %d" % ((z,) + self.stark.permutation_pair(z) + (plural(k), r)) for z, k, r in self.failing_zs()]
        return "\n".join(lines)

    def __repr__(self):
        return f"<TraceExplanation {len(self.failing_blocks())} blocks, {len(self.failing_zs())} Z columns fail>"

    def __eq__(self, other):
        if not isinstance(other, TraceExplanation):
            return NotImplemented
        return all(np.array_equal(getattr(self, f), getattr(other, f)) for f in ("block_failing_rows", "block_first_row", "z_failing_rows", "z_first_row"))


PERM_PAIR_STAT = np.dtype([(f, np.uint64) for f in ("differing_values", "excess_lhs", "excess_rhs", "entries")])                  # sbn_perm_pair_stat
PERM_DIFF_ENTRY = np.dtype([(f, np.uint64) for f in ("value", "count_lhs", "count_rhs", "first_row_lhs", "first_row_rhs")])     # sbn_perm_diff_entry


class PermutationExplanation:
    """What explain_permutations found: the lhs column of every chosen permutation pair against its rhs column as multisets.
    zs [n_out] is the pair of every output index, stats [n_out] a structured array (differing_values, excess_lhs, excess_rhs,
    entries: exact whatever per_pair was), entries [n_out][per_pair] the differing values of each pair, smallest first (value,
    count_lhs, count_rhs, first_row_lhs, first_row_rhs; a first row of 2^64 - 1 = the value is not in that column), of which
    the first stats["entries"] are meaningful.  pairs lists the failing pairs in ascending z as dicts."""

    def __init__(self, stark, zs, stats, entries):
        self.stark, self.zs, self.stats, self.entries = stark, zs, stats, entries

    @property
    def ok(self):
        return not self.stats["differing_values"].any()

    @property
    def pairs(self):
        out = []
        for k in sorted(np.nonzero(self.stats["differing_values"])[0], key=lambda k: int(self.zs[k])):
            st, z = self.stats[k], int(self.zs[k])
            lhs, rhs = self.stark.permutation_pair(z)
            ents = [{f: (None if f.startswith("first_row") and int(e[f]) == _NO_ROW else int(e[f])) for f in PERM_DIFF_ENTRY.names}
                    for e in self.entries[k, :int(st["entries"])]]
            out.append({"z": z, "lhs_col": lhs, "rhs_col": rhs, "differing_values": int(st["differing_values"]),
                        "excess_lhs": int(st["excess_lhs"]), "excess_rhs": int(st["excess_rhs"]), "entries": ents})
        return out

    def __str__(self):
        if self.ok:
            return "ok: the two columns of every permutation pair hold the same values"
        cells = lambda k: f"{k:,} cell{'s' if k != 1 else ''}"   # noqa: E731
        side = lambda c, r, name: f"{c:,} x {name}" + (f" (first row {r})" if r is not None else "")   # noqa: E731
        lines = []
        for q in self.pairs:
            d, el, er = q["differing_values"], q["excess_lhs"], q["excess_rhs"]
            more = f"{cells(el)} more on each side" if el == er else f"{cells(el)} more on lhs, {er:,} on rhs"
            parts = ["Z %d (cols %d, %d): %s value%s differ%s, %s" % (q["z"], q["lhs_col"], q["rhs_col"], f"{d:,}", "" if d == 1 else "s", "s" if d == 1 else "", more)]
            parts += ["%d: %s, %s" % (e["value"], side(e["count_lhs"], e["first_row_lhs"], "lhs"), side(e["count_rhs"], e["first_row_rhs"], "rhs")) for e in q["entries"]]
            if len(q["entries"]) < d:
                parts.append(f"{d - len(q['entries']):,} more not listed")
            lines.append("; ".join(parts))
        return "\n".join(lines)

    def __repr__(self):
        return f"<PermutationExplanation {int(np.count_nonzero(self.stats['differing_values']))} of {len(self.zs)} pairs differ>"

    def __eq__(self, other):
        if not isinstance(other, PermutationExplanation):
            return NotImplemented
        if not (np.array_equal(self.zs, other.zs) and np.array_equal(self.stats, other.stats)):
            return False
        return all(np.array_equal(self.entries[k, :int(m)], other.entries[k, :int(m)]) for k, m in enumerate(self.stats["entries"]))


def _explain_permutations_buffers(stark, zs, per_pair):
    """zs as the C calls take it (None: all pairs), the pair of every output index, and the two output arrays."""
    Z = stark.num_permutation_zs()
    zs = None if zs is None else np.ascontiguousarray(zs, dtype=np.uint32).reshape(-1)
    which = np.arange(Z, dtype=np.uint32) if zs is None else zs
    per_pair = int(per_pair)
    if per_pair < 0:
        raise SbnError(-1, "per_pair is negative")
    return zs, which, per_pair, np.zeros(len(which), dtype=PERM_PAIR_STAT), np.zeros((len(which), per_pair), dtype=PERM_DIFF_ENTRY)


def _opt_ptr(a):
    return None if a is None or a.size == 0 else _ptr(a)


def _explain_rows_buffers(stark, rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
    B, Z = len(stark.constraint_blocks()), stark.num_permutation_zs()
    return rows, np.zeros((len(rows), (B + 7) // 8), dtype=np.uint8), np.zeros((len(rows), (Z + 7) // 8), dtype=np.uint8)


def _explain_trace_buffers(stark):
    B, Z = len(stark.constraint_blocks()), stark.num_permutation_zs()
    return np.zeros((B, 2), dtype=np.uint64), np.zeros((Z, 2), dtype=np.uint64)


def _host_trace_args(stark, trace, public_inputs):
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    n = trace.shape[1] if trace.ndim == 2 else 0
    if trace.ndim != 2 or trace.shape[0] != stark.num_columns or n == 0 or n & (n - 1):
        raise SbnError(-1, "trace shape does not match the table")
    return trace, pi, n.bit_length() - 1


TRACE_REDUCE = 1   # SBN_TRACE_REDUCE (include/sbn.h)


_U64 = np.dtype(np.uint64)


class ColumnTable:
    """The pointer table of a trace held as separate columns, built once for several calls: a sequence of 1-D uint64 arrays, or a
    2-D uint64 array whose rows are contiguous, with any stride between rows (big[::2], big[::-1]).  Nothing is copied -- an array
    of another dtype or with strided elements is refused -- and the table keeps the references that keep the memory alive.
    Prover.prove_host_columns, prove_columns and BatchProver.prove_host_traces take a ColumnTable wherever they take columns
    (building the table of 1676 arrays costs about as much Python time as a millisecond of proving)."""

    def __init__(self, columns):
        if isinstance(columns, np.ndarray) and columns.ndim == 2:
            a = columns
            if a.dtype != _U64 or (a.shape[1] > 1 and a.strides[1] != 8):
                raise SbnError(-1, "columns must be uint64 with contiguous rows")
            self.addr = (a.ctypes.data + np.arange(a.shape[0], dtype=np.int64) * a.strides[0]).astype(np.uint64)
            self.n, self._keep = a.shape[1], [a]
        else:
            keep = list(columns)
            n = len(keep[0]) if keep and isinstance(keep[0], np.ndarray) and keep[0].ndim == 1 else 0
            addr = np.empty(len(keep), dtype=np.uint64)
            for c, a in enumerate(keep):
                if type(a) is not np.ndarray or (a.dtype is not _U64 and a.dtype != _U64) or a.shape != (n,) or (n > 1 and a.strides[0] != 8):
                    raise SbnError(-1, f"column {c} must be a contiguous 1-D uint64 array of the first column's length")
                addr[c] = a.__array_interface__["data"][0]
            self.addr, self.n, self._keep = addr, n, keep

    def __len__(self):
        return len(self.addr)


def _column_pointers(columns, ncols=None, n=None):
    """The ColumnTable of `columns` (itself, if it is one), checked against a table's column count and height."""
    t = columns if isinstance(columns, ColumnTable) else ColumnTable(columns)
    if (ncols is not None and len(t) != ncols) or (n is not None and t.n != n):
        raise SbnError(-1, "columns do not match the table")
    return t


def gather_columns(columns, word0, length):
    """Flat words [word0, word0 + length) of the column-major matrix whose columns are `columns` (sbn_gather_columns: the copy
    Prover.prove_host_columns makes into each piece of its upload ring; test hook).  No device needed."""
    t = _column_pointers(columns)
    out = np.zeros(length, dtype=np.uint64)
    _check(lib().sbn_gather_columns(_ptr(t.addr), len(t), t.n, word0, length, _ptr(out)))
    return out


def reduce_words(words, on_device=True):
    """In place, every word >= p of a contiguous 1-D uint64 array becomes w - p; returns how many changed (sbn_reduce_words: the
    kernel of Prover.prove_host_columns(reduce=True); test hook).  on_device=False runs a host loop and needs no device."""
    w = words
    if not isinstance(w, np.ndarray) or w.dtype != np.uint64 or w.ndim != 1 or (len(w) > 1 and w.strides[0] != 8) or not w.flags.writeable:
        raise SbnError(-1, "words must be a writeable contiguous 1-D uint64 array")
    out = C.c_uint64(0)
    _check(lib().sbn_reduce_words(_ptr(w), len(w), 1 if on_device else 0, C.byref(out)))
    return int(out.value)


class RowTable:
    """The sbn_host_rows of a ROW-major trace: a 2-D uint64 array whose rows are contiguous, with any stride between rows that is a
    non-negative multiple of 8 bytes and at least a row (big[:, :398] of a wider matrix: the flat form), or a sequence of 1-D
    uint64 arrays of one length (the pointer form, the reference's Vec<Vec<F>>).  Nothing is copied, and the table keeps the
    references that keep the memory alive.  The row-major calls take a RowTable wherever they take rows."""

    def __init__(self, rows):
        r = _HostRows(struct_size=C.sizeof(_HostRows))
        if isinstance(rows, np.ndarray) and rows.ndim == 2:
            a = rows
            if a.dtype != _U64 or (a.shape[1] > 1 and a.strides[1] != 8):
                raise SbnError(-1, "rows must be uint64 with contiguous rows")
            if a.shape[0] > 1 and (a.strides[0] % 8 or a.strides[0] < 8 * a.shape[1]):
                raise SbnError(-1, "the row stride must be a multiple of 8 bytes and at least a row")
            r.flat, r.row_stride = a.ctypes.data, (a.strides[0] // 8 if a.shape[0] > 1 else a.shape[1])
            r.n_rows, r.n_cols = a.shape
            self._keep = [a]
        else:
            keep = list(rows)
            n_cols = len(keep[0]) if keep and isinstance(keep[0], np.ndarray) and keep[0].ndim == 1 else 0
            addr = np.empty(len(keep), dtype=np.uint64)
            for i, a in enumerate(keep):
                if type(a) is not np.ndarray or (a.dtype is not _U64 and a.dtype != _U64) or a.shape != (n_cols,) or (n_cols > 1 and a.strides[0] != 8):
                    raise SbnError(-1, f"row {i} must be a contiguous 1-D uint64 array of the first row's length")
                addr[i] = a.__array_interface__["data"][0]
            r.row_ptrs, r.n_rows, r.n_cols = addr.ctypes.data, len(keep), n_cols
            self._keep = [keep, addr]
        self.raw = r

    @property
    def shape(self):
        return (self.raw.n_rows, self.raw.n_cols)


def _row_table(rows):
    return rows if isinstance(rows, RowTable) else RowTable(rows)


def trace_from_rows_host(stark, rows, reduce=False):
    """The column-major trace of a row-major one, on host threads (sbn_trace_from_rows_host; no device): `rows` as RowTable takes
    them, num_columns wide (whole-row mode: transposed and checked) or num_main_columns wide (main-row mode, the five Exp tables:
    the derived columns are appended as the host generators do).  reduce=True: words >= p are taken mod p instead of refused, and
    (trace, number of words changed) is returned."""
    t = _row_table(rows)
    out = np.zeros((stark.num_columns, t.raw.n_rows), dtype=np.uint64)
    reduced = C.c_uint64(0)
    _check(lib().sbn_trace_from_rows_host(C.byref(stark._d), C.byref(t.raw), TRACE_REDUCE if reduce else 0, _ptr(out), C.byref(reduced)))
    return (out, int(reduced.value)) if reduce else out


def explain_rows_host(stark, trace, public_inputs, rows, seed=0):
    """Which constraint blocks and Z columns the listed rows of `trace` break, on host threads (sbn_explain_rows_host).  The
    same RowsExplanation, for the same seed, as Prover.explain_rows gives for the loaded trace."""
    trace, pi, bits = _host_trace_args(stark, trace, public_inputs)
    rows, bf, zf = _explain_rows_buffers(stark, rows)
    _check(lib().sbn_explain_rows_host(C.byref(stark._d), _ptr(trace), bits, _ptr(pi), len(pi), seed, _ptr(rows), len(rows), _ptr(bf), _ptr(zf)))
    return RowsExplanation(stark, rows, bf, zf)


def explain_trace_host(stark, trace, public_inputs, seed=0):
    """Per block and Z column, on how many rows of `trace` it fails and where first, on host threads (sbn_explain_trace_host)."""
    trace, pi, bits = _host_trace_args(stark, trace, public_inputs)
    bs, zs = _explain_trace_buffers(stark)
    _check(lib().sbn_explain_trace_host(C.byref(stark._d), _ptr(trace), bits, _ptr(pi), len(pi), seed, _ptr(bs), _ptr(zs)))
    return TraceExplanation(stark, bs, zs)


def explain_permutations_host(stark, trace, zs=None, per_pair=8):
    """The values and rows behind failing permutation pairs of `trace`, on host threads (sbn_explain_permutations_host): per
    pair of zs (None: all) the exact multiset difference of its two columns, the per_pair smallest differing values listed.
    The same PermutationExplanation as Prover.explain_permutations gives for the loaded trace."""
    trace, _, bits = _host_trace_args(stark, trace, np.zeros(0, dtype=np.uint64))
    zs, which, per_pair, st, en = _explain_permutations_buffers(stark, zs, per_pair)
    _check(lib().sbn_explain_permutations_host(C.byref(stark._d), _ptr(trace), bits, None if zs is None else _ptr(zs), len(which), per_pair,
                                               _opt_ptr(st), _opt_ptr(en)))
    return PermutationExplanation(stark, which, st, en)


WITNESS_CELL = np.dtype([(f, np.uint64) for f in ("row", "column", "got", "want")])   # sbn_witness_cell


class WitnessDiff:
    """What diff_witness found (sbn_witness_diff): the trace against the canonical witness of its instance list, cell by cell.
    cells, main_cells, rows, columns and pi_words are exact whatever the cap was; first_row, first_column and first_pi_word are None
    when nothing differs there; column_cells / column_first_row [num_columns] are the per-column counts and first differing rows
    (2^64 - 1: none); raw_cells is the list as the library wrote it (WITNESS_CELL), `listed` the same cells as dicts: ascending
    (row, column) over the main columns, the derived columns only behind them.  Each listed cell carries its instance and its row
    inside the instance and names what checks it: the constraint blocks whose column range holds the column, or the permutation
    pairs of a permuted column."""

    def __init__(self, stark, raw, column_cells, column_first_row, cells):
        self.stark = stark
        none = lambda v: None if v == _NO_ROW else int(v)   # noqa: E731
        self.cells, self.main_cells, self.rows, self.columns = int(raw.cells), int(raw.main_cells), int(raw.rows), int(raw.columns)
        self.first_row, self.first_column = none(raw.first_row), none(raw.first_column)
        self.pi_words, self.first_pi_word = int(raw.pi_words), none(raw.first_pi_word)
        self.column_cells, self.column_first_row = column_cells, column_first_row
        self.raw_cells = cells[:int(raw.listed)]
        self.rows_per_instance = _rows_per_instance(stark)

    @property
    def ok(self):
        return self.cells == 0 and self.pi_words == 0

    def checked_by(self, column):
        """Names of what checks `column`: the constraint blocks whose column range holds it, else its permutation pairs."""
        names = getattr(self.stark, "_column_checks", None)
        if names is None:   # once per table: a wide trace lists thousands of cells
            by_block, by_pair = {}, {}
            for b in self.stark.constraint_blocks():
                for c in range(b.col_first, b.col_first + b.col_count):
                    by_block.setdefault(c, {})[str(b).split(" [")[0].split(" cols ")[0]] = None   # (a lookup pair's two constraints are two blocks of one name)
            for z in range(self.stark.num_permutation_zs()):
                l, r = self.stark.permutation_pair(z)
                for c in {l, r}:
                    by_pair.setdefault(c, []).append("Z %d (cols %d, %d)" % (z, l, r))
            names = self.stark._column_checks = (by_block, by_pair)
        return list(names[0].get(column, ())) or list(names[1].get(column, ()))

    @property
    def listed(self):
        rpi = self.rows_per_instance
        return [{"row": int(c["row"]), "column": int(c["column"]), "got": int(c["got"]), "want": int(c["want"]), "instance": int(c["row"]) // rpi,
                 "instance_row": int(c["row"]) % rpi, "main": int(c["column"]) < self.stark.num_main_columns, "checked_by": self.checked_by(int(c["column"]))}
                for c in self.raw_cells]

    def __str__(self):
        if self.ok:
            return "ok: the trace is the canonical witness of its instances"
        plural = lambda k, w: f"{k:,} {w}{'' if k == 1 else 's'}"   # noqa: E731
        parts = []
        if self.cells:
            parts.append(f"{plural(self.cells, 'cell')} differ{'s' if self.cells == 1 else ''} in {plural(self.columns, 'column')} on {plural(self.rows, 'row')} "
                         f"({self.main_cells:,} in the main columns)")
        for c in self.listed:
            by = ", ".join(c["checked_by"])
            parts.append(f"row {c['row']} (instance {c['instance']}, row {c['instance_row']} of {self.rows_per_instance}) col {c['column']} [{by}]: "
                         f"got {c['got']:#x}, canonical {c['want']:#x}")
        if len(self.raw_cells) < self.cells:
            parts.append(f"{self.cells - len(self.raw_cells):,} more not listed")
        if self.pi_words:
            parts.append(f"{plural(self.pi_words, 'public input')} differ{'s' if self.pi_words == 1 else ''}, first word {self.first_pi_word}")
        return "; ".join(parts)

    def __repr__(self):
        return f"<WitnessDiff {self.cells} cells, {self.pi_words} public inputs differ>"

    def _key(self):
        return (self.cells, self.main_cells, self.rows, self.columns, self.first_row, self.first_column, self.pi_words, self.first_pi_word)

    def __eq__(self, other):
        if not isinstance(other, WitnessDiff):
            return NotImplemented
        return self._key() == other._key() and np.array_equal(self.column_cells, other.column_cells) and \
            np.array_equal(self.column_first_row, other.column_first_row) and np.array_equal(self.raw_cells, other.raw_cells)


def _diff_witness_buffers(stark, ios, cells):
    """ios as the C calls take it (None: from the public inputs), the report, the two per-column arrays and the list."""
    cells = int(cells)
    if cells < 0:
        raise SbnError(-1, "cells is negative")
    ios = None if ios is None else np.ascontiguousarray(ios, dtype=np.uint32)
    words = _EXP_IO_WORDS.get(stark.kind)
    if ios is not None and words is not None and ios.shape != (stark.num_io, 2 * words[0] + words[1]):
        raise SbnError(-1, f"ios must be {stark.num_io} rows of {2 * words[0] + words[1]} u32 words")
    C_ = stark.num_columns
    return ios, cells, _WitnessDiff(struct_size=C.sizeof(_WitnessDiff)), np.zeros(C_, dtype=np.uint64), np.zeros(C_, dtype=np.uint64), np.zeros(cells, dtype=WITNESS_CELL)


def diff_witness_host(stark, trace, public_inputs, ios=None, cells=16):
    """`trace` against the canonical witness of its instance list, cell by cell, on host threads (sbn_diff_witness_host): the
    instances are `ios`, or those the public inputs carry.  The same WitnessDiff as Prover.diff_witness gives for the loaded trace;
    any height the host generators take."""
    trace, pi, bits = _host_trace_args(stark, trace, public_inputs)
    ios, cells, raw, cc, cf, ce = _diff_witness_buffers(stark, ios, cells)
    _check(lib().sbn_diff_witness_host(C.byref(stark._d), _ptr(trace), bits, _ptr(pi), len(pi), None if ios is None else _ptr(ios), stark.num_io,
                                       C.byref(raw), _ptr(cc), _ptr(cf), _opt_ptr(ce), cells))
    return WitnessDiff(stark, raw, cc, cf, ce)


def instances_from_public_inputs(stark, pi):
    """(ios, outputs) of the public inputs of an Exp table (sbn_instances_from_public_inputs): the instance rows generate_trace
    takes, [num_io][2 xw + ew] u32, and the outputs in the word shape of x, [num_io][xw] u32."""
    pi = np.ascontiguousarray(pi, dtype=np.uint64).reshape(-1)
    iow = _EXP_IO_WORDS.get(stark.kind)
    if iow is None:
        raise SbnError(-1, "not an Exp table")
    xw, ew = iow
    ios = np.zeros((stark.num_io, 2 * xw + ew), dtype=np.uint32)
    outs = np.zeros((stark.num_io, xw), dtype=np.uint32)
    _check(lib().sbn_instances_from_public_inputs(stark.kind, _ptr(pi), len(pi), stark.num_io, _ptr(ios), _ptr(outs)))
    return ios, outs


class Prover:
    """Device context for one (table, degree_bits): buffers stay allocated across proofs.  lde="compact" (rate_bits > 1): the
    LDEs of the wide matrices are not kept, the opened rows are recomputed from the coefficients (include/sbn.h SBN_LDE_COMPACT);
    the proofs are the same words.  guard="device" | "host": verified proving (set_guard)."""

    def __init__(self, stark, config, degree_bits, lde="full", guard=None):
        self.stark, self.config, self.degree_bits = stark, config, degree_bits
        self._h = C.c_void_p()
        opt = _prover_options(lde)
        mode = _guard_mode(guard)
        # by the header's contract the same call; so the "full" path of this class never enters sbn_prover_create_with (a GPU test calls
        # it with SBN_LDE_FULL through ctypes), and a library named by SBN_LIB that lacks the new entry points still serves it
        if opt is None or opt.lde_storage == LDE_STORAGE["full"]:
            _check(lib().sbn_prover_create(C.byref(stark._d), C.byref(config._c), degree_bits, C.byref(self._h)))
        else:
            _check(lib().sbn_prover_create_with(C.byref(stark._d), C.byref(config._c), degree_bits, C.byref(opt), C.byref(self._h)))
        if mode:   # (guard=None never enters the new entry point, as lde="full" above)
            self.set_guard(mode)

    def set_guard(self, guard):
        """Verified proving (sbn_prover_set_guard): with "device" or "host" every proof this context returns has passed that
        verifier first -- the words are those of the unguarded call; a proof the verifier rejects is an SbnError with code -6 whose
        .reason is the verifier's own text, and the trace stays loaded for check_trace / explain_* / diff_witness.  None: off."""
        _check(lib().sbn_prover_set_guard(self._h, _guard_mode(guard)))

    def guard_stats(self):
        """GuardStats(checked, rejected, ns, device_bytes): proofs the guard checked and rejected, host nanoseconds spent checking,
        device bytes of the guard's verifier."""
        return _guard_stats(lib().sbn_prover_guard_stats, self._h)

    def load_trace(self, trace, public_inputs):
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        _check(lib().sbn_prover_load_trace(self._h, _ptr(trace), _ptr(pi), len(pi)))

    def load_trace_device(self, device_ptr, public_inputs):
        pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        _check(lib().sbn_prover_load_trace_device(self._h, C.c_void_p(device_ptr), _ptr(pi), len(pi)))

    def trace_device_ptr(self):
        return lib().sbn_prover_trace_device_ptr(self._h)

    def generate_trace(self, ios):
        """On-device G1ExpStark::generate_trace + generate_public_inputs; returns the public inputs."""
        ios = np.ascontiguousarray(ios, dtype=np.uint32)
        pi = np.zeros(self.stark.num_public_inputs, dtype=np.uint64)
        _check(lib().sbn_prover_generate_trace(self._h, _ptr(ios), ios.shape[0], _ptr(pi)))
        return pi

    def generate_trace_chained(self, terms, start):
        """generate_trace on the list chain_instances(stark, terms, start) gives, the offsets built on the device where the
        table's chains run there; returns (public inputs, ios)."""
        terms, start, xw, ew = _chain_args(self.stark, terms, start)
        pi = np.zeros(self.stark.num_public_inputs, dtype=np.uint64)
        ios = np.zeros((terms.shape[0], 2 * xw + ew), dtype=np.uint32)
        _check(lib().sbn_prover_generate_trace_chained(self._h, _ptr(terms), terms.shape[0], _ptr(start), _ptr(pi), _ptr(ios)))
        return pi, ios

    def generate_trace_scalar_muls(self, points, scalars, offset=None):
        """generate_trace on the one-unit list scalar_mul_instances(stark, points, scalars, offset) gives, expanded and un-offset
        on the device where the table's chains run there; returns (public inputs, products, infinity, ios)."""
        points, scalars, offset, w = _scalar_mul_args(self.stark, points, scalars, offset)
        count = points.shape[0]
        pi = np.zeros(self.stark.num_public_inputs, dtype=np.uint64)
        products = np.zeros((count, w), dtype=np.uint32)
        infinity = np.zeros(count, dtype=np.uint8)
        ios = np.zeros((count, 2 * w + 8), dtype=np.uint32)
        _check(lib().sbn_prover_generate_trace_scalar_muls(self._h, _ptr(points), _ptr(scalars), scalars.shape[0], count, _ptr(offset),
                                                           _ptr(pi), _ptr(products), _ptr(infinity), _ptr(ios)))
        return pi, products, infinity, ios

    def generate_trace_msms(self, terms, lengths, starts=None):
        """generate_trace on the one-unit list msm_batch_instances(stark, terms, lengths, starts) gives (M <= num_io, the rest
        padded), the offsets, finals and sums derived on the device where the table's chains run there; returns (public inputs,
        finals, sums, infinity, ios)."""
        terms, lengths, starts, xw, ew, curve = _msm_batch_args(self.stark, terms, lengths, starts)
        pi = np.zeros(self.stark.num_public_inputs, dtype=np.uint64)
        ios = np.zeros((self.stark.num_io, 2 * xw + ew), dtype=np.uint32)
        finals, sums, infinity = _msm_batch_outputs(len(lengths), xw, curve)
        _check(lib().sbn_prover_generate_trace_msm_batch(self._h, _ptr(terms), _ptr(lengths), len(lengths), _ptr(starts),
                                                         starts.shape[0] if starts is not None else 1, _ptr(pi), _ptr(finals), _ptr(sums), _ptr(infinity),
                                                         _ptr(ios)))
        return pi, finals, sums, infinity, ios

    def generate_trace_msms_complete(self, terms, lengths, term_infinity=None):
        """generate_trace on the one-unit list msm_batch_instances_complete(stark, terms, lengths, term_infinity) gives (M <=
        num_io, the rest padded); returns (public inputs, terms_eff, starts, choice, finals, sums, infinity, ios).  A failing call
        leaves no trace loaded."""
        terms, lengths, term_infinity, xw, ew = _complete_args(self.stark, terms, lengths, term_infinity)
        pi = np.zeros(self.stark.num_public_inputs, dtype=np.uint64)
        ios = np.zeros((self.stark.num_io, 2 * xw + ew), dtype=np.uint32)
        eff, starts, choice, finals, sums, infinity = _complete_outputs(terms.shape[0], len(lengths), xw, ew)
        _check(lib().sbn_prover_generate_trace_msm_batch_complete(self._h, _ptr(terms), _ptr(term_infinity), _ptr(lengths), len(lengths), _ptr(pi), _ptr(eff),
                                                                  _ptr(starts), _ptr(choice), _ptr(finals), _ptr(sums), _ptr(infinity), _ptr(ios)))
        return pi, eff, starts, choice, finals, sums, infinity, ios

    def generate_trace_powers(self, bases, exps, depth=1):
        """generate_trace on the one-unit list power_instances(stark, bases, exps, depth) gives (count * depth <= num_io, the
        rest padded), the towers linked and walked on the device where the table's chains run there; returns (public inputs,
        powers, ios)."""
        bases, exps, depth, w, ew = _power_args(self.stark, bases, exps, depth)
        count = bases.shape[0]
        pi = np.zeros(self.stark.num_public_inputs, dtype=np.uint64)
        powers = np.zeros((count, depth, w), dtype=np.uint32)
        ios = np.zeros((self.stark.num_io, 2 * w + ew), dtype=np.uint32)
        _check(lib().sbn_prover_generate_trace_powers(self._h, _ptr(bases), _ptr(exps), exps.shape[0], count, depth, _ptr(pi), _ptr(powers), _ptr(ios)))
        return pi, powers, ios

    def generate_trace_program(self, nodes, values, exps):
        """generate_trace on the one-unit list program_instances(stark, nodes, values, exps) gives (count <= num_io, the rest
        padded), the links resolved on the device, one launch per level, where the table's chains run there; returns (public
        inputs, outs, ios).  A failing call leaves no trace loaded."""
        nodes, values, exps, w, ew = _program_args(self.stark, nodes, values, exps)
        pi = np.zeros(self.stark.num_public_inputs, dtype=np.uint64)
        outs = np.zeros((nodes.shape[0], w), dtype=np.uint32)
        ios = np.zeros((self.stark.num_io, 2 * w + ew), dtype=np.uint32)
        _check(_program_fn(nodes, "sbn_prover_generate_trace_program")(self._h, _ptr(nodes), nodes.shape[0], _ptr(values), values.shape[0], _ptr(exps), exps.shape[0],
                                                       _ptr(pi), _ptr(outs), _ptr(ios)))
        return pi, outs, ios

    def generate_trace_curve_program(self, nodes, points, exps):
        """generate_trace on the one-unit list curve_program_instances(stark, nodes, points, exps) gives (count <= num_io, the rest
        padded); where the table's chains run on the device the links are resolved there, one launch per level, from start
        candidate 0, and a bad event falls back to the host derivation.  Returns (public inputs, outs, values, infinity, choice,
        ios).  A failing call leaves no trace loaded."""
        nodes, points, exps, w = _curve_program_args(self.stark, nodes, points, exps)
        pi = np.zeros(self.stark.num_public_inputs, dtype=np.uint64)
        outs, values, infinity, choice = _curve_program_outputs(nodes.shape[0], w)
        ios = np.zeros((self.stark.num_io, 2 * w + 8), dtype=np.uint32)
        _check(lib().sbn_prover_generate_trace_curve_program(self._h, _ptr(nodes), nodes.shape[0], _ptr(points), points.shape[0], _ptr(exps), exps.shape[0],
                                                             _ptr(pi), _ptr(outs), _ptr(values), _ptr(infinity), _ptr(choice), _ptr(ios)))
        return pi, outs, values, infinity, int(choice[0]), ios

    def read_trace(self):
        trace = np.zeros((self.stark.num_columns, 1 << self.degree_bits), dtype=np.uint64)
        _check(lib().sbn_prover_read_trace(self._h, _ptr(trace)))
        return trace

    def check_trace(self, seed=0, flags=False):
        """Which rows of the loaded trace break a constraint (sbn_prover_check_trace: the quotient stage's constraint kernels
        on the trace domain).  The trace stays loaded; flags=True also returns the per-row segment bits."""
        raw = _TraceReport(struct_size=C.sizeof(_TraceReport))
        row_flags = np.zeros(1 << self.degree_bits, dtype=np.uint8) if flags else None
        _check(lib().sbn_prover_check_trace(self._h, seed, C.byref(raw), _ptr(row_flags)))
        return TraceReport(raw, row_flags, _rows_per_instance(self.stark))

    def _times(self, getter, keys):
        """What a *_times getter of the C ABI wrote, under `keys` in their order."""
        buf = (C.c_float * len(keys))()
        k = getter(self._h, buf, len(keys))
        return dict(zip(keys, (float(buf[i]) for i in range(k))))

    def check_times(self):
        """Device times of the last check_trace() in ms (HIP events)."""
        return self._times(lib().sbn_prover_check_times, ("perm_z", "constraints", "reduction", "download"))

    def explain_rows(self, rows, seed=0):
        """Which constraint blocks and Z columns the listed rows of the loaded trace break (sbn_prover_explain_rows)."""
        rows, bf, zf = _explain_rows_buffers(self.stark, rows)
        _check(lib().sbn_prover_explain_rows(self._h, seed, _ptr(rows), len(rows), _ptr(bf), _ptr(zf)))
        return RowsExplanation(self.stark, rows, bf, zf)

    def explain_trace(self, seed=0):
        """Per block and Z column, on how many rows of the loaded trace it fails and where first (sbn_prover_explain_trace)."""
        bs, zs = _explain_trace_buffers(self.stark)
        _check(lib().sbn_prover_explain_trace(self._h, seed, _ptr(bs), _ptr(zs)))
        return TraceExplanation(self.stark, bs, zs)

    def explain_times(self):
        """Device times of the last explain_rows() / explain_trace() in ms (HIP events)."""
        return self._times(lib().sbn_prover_explain_times, ("perm_z", "explain", "download"))

    def explain_permutations(self, zs=None, per_pair=8):
        """The values and rows behind failing permutation pairs of the loaded trace (sbn_prover_explain_permutations): signed
        histograms in LDS, bit for bit what explain_permutations_host gives."""
        zs, which, per_pair, st, en = _explain_permutations_buffers(self.stark, zs, per_pair)
        _check(lib().sbn_prover_explain_permutations(self._h, None if zs is None else _ptr(zs), len(which), per_pair, _opt_ptr(st), _opt_ptr(en)))
        return PermutationExplanation(self.stark, which, st, en)

    def explain_permutation_times(self):
        """Times of the last explain_permutations() in ms: the two kernels (HIP events), download + host merge (host clock)."""
        return self._times(lib().sbn_prover_explain_permutation_times, ("histogram", "rows", "download_merge"))

    def diff_witness(self, ios=None, cells=16):
        """The loaded trace against the canonical witness of its instance list, cell by cell (sbn_prover_diff_witness): the
        witness is rebuilt on the device from `ios`, or from the instances the loaded public inputs carry; `cells` differing
        cells are listed (0 .. 65536).  The trace stays loaded, also after a refused list."""
        ios, cells, raw, cc, cf, ce = _diff_witness_buffers(self.stark, ios, cells)
        _check(lib().sbn_prover_diff_witness(self._h, None if ios is None else _ptr(ios), self.stark.num_io, C.byref(raw), _ptr(cc), _ptr(cf), _opt_ptr(ce), cells))
        return WitnessDiff(self.stark, raw, cc, cf, ce)

    def diff_times(self):
        """Times of the last diff_witness() in ms: device witness, compare kernel (HIP events), listing + downloads (host clock)."""
        return self._times(lib().sbn_prover_diff_witness_times, ("witness", "compare", "list_download"))

    def prove(self):
        h = C.c_void_p()
        _check(lib().sbn_prover_prove(self._h, C.byref(h)))
        return _take_proof(h)

    def prove_host_trace(self, trace, public_inputs):
        """load_trace + prove in one call: the host trace crosses PCIe inside the trace commitment, chunk by chunk, and is checked for
        canonical form on the device.  Same proof; afterwards the trace is resident (prove() can be repeated).  A refused call
        leaves no trace loaded."""
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if trace.shape != (self.stark.num_columns, 1 << self.degree_bits):
            raise SbnError(-1, "trace shape does not match the prover")
        h = C.c_void_p()
        _check(lib().sbn_prover_prove_host_trace(self._h, _ptr(trace), _ptr(pi), len(pi), C.byref(h)))
        return _take_proof(h)

    def prove_host_columns(self, columns, public_inputs, reduce=False):
        """prove_host_trace for a trace held as separate columns (the reference's Vec<PolynomialValues<F>>): a sequence of 1-D
        uint64 arrays, or a 2-D array whose rows are contiguous with any stride between them.  The data is never copied on the
        host: the upload gathers from the columns into its pinned ring.  reduce=False: the proof and the refusals of
        prove_host_trace on the flattened matrix.  reduce=True: words and public inputs >= p are taken mod p (the words on the
        device) instead of refused, and (Proof, number of trace words changed) is returned."""
        t = _column_pointers(columns, self.stark.num_columns, 1 << self.degree_bits)   # (holds the references during the call)
        pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        h, reduced = C.c_void_p(), C.c_uint64(0)
        _check(lib().sbn_prover_prove_host_columns(self._h, _ptr(t.addr), len(t), TRACE_REDUCE if reduce else 0, _ptr(pi), len(pi), C.byref(reduced), C.byref(h)))
        proof = _take_proof(h)
        return (proof, int(reduced.value)) if reduce else proof

    def load_trace_rows(self, rows, public_inputs, reduce=False):
        """load_trace for a ROW-major trace (sbn_prover_load_trace_rows): `rows` as RowTable takes them, num_columns wide, or
        num_main_columns wide on the Exp tables (the device then writes the derived columns itself).  The transposition and the
        canonical-form check run on the device.  reduce=True returns the number of trace words taken mod p."""
        t = _row_table(rows)
        pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        reduced = C.c_uint64(0)
        _check(lib().sbn_prover_load_trace_rows(self._h, C.byref(t.raw), TRACE_REDUCE if reduce else 0, _ptr(pi), len(pi), C.byref(reduced)))
        return int(reduced.value) if reduce else None

    def load_trace_rows_device(self, device_ptr, row_stride, n_cols, public_inputs, reduce=False):
        """The same for rows already in device memory (sbn_prover_load_trace_rows_device): row r at device_ptr + 8 * r * row_stride."""
        pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        reduced = C.c_uint64(0)
        _check(lib().sbn_prover_load_trace_rows_device(self._h, C.c_void_p(device_ptr), row_stride, n_cols, TRACE_REDUCE if reduce else 0, _ptr(pi), len(pi),
                                                       C.byref(reduced)))
        return int(reduced.value) if reduce else None

    def prove_host_rows(self, rows, public_inputs, reduce=False):
        """load_trace_rows + prove in one call (sbn_prover_prove_host_rows).  reduce=True returns (Proof, words changed)."""
        t = _row_table(rows)
        pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        h, reduced = C.c_void_p(), C.c_uint64(0)
        _check(lib().sbn_prover_prove_host_rows(self._h, C.byref(t.raw), TRACE_REDUCE if reduce else 0, _ptr(pi), len(pi), C.byref(reduced), C.byref(h)))
        proof = _take_proof(h)
        return (proof, int(reduced.value)) if reduce else proof

    def stage_times(self):
        buf = (C.c_float * 32)()
        k = lib().sbn_prover_stage_times(self._h, buf, 32)
        return {lib().sbn_prover_stage_name(i).decode(): float(buf[i]) for i in range(k)}

    def describe(self):
        """The SBN_* switches this prover was created under, resolved (csrc/settings.hpp), as a dict of strings."""
        buf = C.create_string_buffer(1024)
        _check(lib().sbn_prover_describe(self._h, buf, 1024))
        out = {}
        for kv in buf.value.decode().split(" "):
            k, _, v = kv.partition("=")
            out[k] = v
        return out

    def close(self):
        if self._h:
            lib().sbn_prover_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchProver:
    """`inflight` prover contexts on one GPU: proves a batch of instance lists (witness generated on the device)."""

    def __init__(self, stark, config, degree_bits, inflight=3, lde="full", guard=None):
        self.stark, self.config, self.degree_bits = stark, config, degree_bits
        self._h = C.c_void_p()
        opt = _prover_options(lde)
        mode = _guard_mode(guard)
        if opt is None or opt.lde_storage == LDE_STORAGE["full"]:
            _check(lib().sbn_batch_prover_create(C.byref(stark._d), C.byref(config._c), degree_bits, inflight, C.byref(self._h)))
        else:
            _check(lib().sbn_batch_prover_create_with(C.byref(stark._d), C.byref(config._c), degree_bits, inflight, C.byref(opt), C.byref(self._h)))
        if mode:
            self.set_guard(mode)

    def set_guard(self, guard):
        """Prover.set_guard for every context of the batch (sbn_batch_prover_set_guard): each checks its own proofs on its own
        worker thread with its own verifier.  A unit whose proof is rejected fails the call with code -6, "unit <u>: " and the
        verifier's reason; no proof is returned."""
        _check(lib().sbn_batch_prover_set_guard(self._h, _guard_mode(guard)))

    def guard_stats(self):
        """Prover.guard_stats summed over the contexts."""
        return _guard_stats(lib().sbn_batch_prover_guard_stats, self._h)

    def _unit_buffers(self, count, words):
        """(ios, out) for `count` instances of `words` u32 each cut into units: the (units, num_io, words) list buffer and the
        array of proof handles (never empty)."""
        units = msm_num_units(count, self.stark.num_io)
        return np.zeros((units, self.stark.num_io, words), dtype=np.uint32), (C.c_void_p * max(units, 1))()

    @staticmethod
    def _proofs(out, units):
        return [_take_proof(C.c_void_p(h)) for h in out[:units]]

    def prove_ios(self, ios_units):
        """ios_units: (count, num_io, words_per_instance) uint32 -> list of Proof, in unit order."""
        ios = np.ascontiguousarray(ios_units, dtype=np.uint32)
        count, num_io, w = ios.shape
        out = (C.c_void_p * count)()
        _check(lib().sbn_batch_prover_prove_ios(self._h, _ptr(ios), num_io * w, num_io, count, out))
        return self._proofs(out, count)

    def prove_host_traces(self, units, public_inputs, reduce=False):
        """Units whose traces are in host memory: `units` is a sequence of column sequences as Prover.prove_host_columns takes
        them, public_inputs one array per unit (sbn_batch_prover_prove_host_columns; any table).  -> list of Proof, in unit order;
        one unit's upload runs beside the other contexts' kernels."""
        ncols, n = self.stark.num_columns, 1 << self.degree_bits
        tables = [_column_pointers(u, ncols, n) for u in units]
        count = len(tables)
        pis = [np.ascontiguousarray(p, dtype=np.uint64) for p in public_inputs]
        n_pi = self.stark.num_public_inputs
        if len(pis) != count or any(len(p) != n_pi for p in pis):
            raise SbnError(-1, "one array of the table's public inputs per unit")
        addr = np.concatenate([t.addr for t in tables]) if count else np.zeros(0, dtype=np.uint64)
        pi_addr = np.array([p.ctypes.data for p in pis], dtype=np.uint64)
        out = (C.c_void_p * max(count, 1))()
        _check(lib().sbn_batch_prover_prove_host_columns(self._h, _ptr(addr), ncols, TRACE_REDUCE if reduce else 0, _ptr(pi_addr), n_pi, count, out))
        return self._proofs(out, count)

    def prove_msm(self, terms, start):
        """A chained list of any length (terms, start as chain_instances) proved as units of the table, the last one padded
        (sbn_batch_prover_prove_msm).  Returns (proofs, final, ios): the unit proofs in order, the last output in the word shape
        of start, and the list as msm_instances gives it."""
        terms, start, xw, ew = _chain_args(self.stark, terms, start)
        ios, out = self._unit_buffers(terms.shape[0], 2 * xw + ew)
        final = np.zeros(xw, dtype=np.uint32)
        _check(lib().sbn_batch_prover_prove_msm(self._h, _ptr(terms), terms.shape[0], _ptr(start), out, _ptr(final), _ptr(ios)))
        return self._proofs(out, len(ios)), final, ios

    def prove_scalar_muls(self, points, scalars, offset=None):
        """Independent scalar multiplications of any count (arguments as scalar_mul_instances) proved as units of the table, the
        last one padded (sbn_batch_prover_prove_scalar_muls).  Returns (proofs, products, infinity, ios)."""
        points, scalars, offset, w = _scalar_mul_args(self.stark, points, scalars, offset)
        count = points.shape[0]
        ios, out = self._unit_buffers(count, 2 * w + 8)
        products = np.zeros((count, w), dtype=np.uint32)
        infinity = np.zeros(count, dtype=np.uint8)
        _check(lib().sbn_batch_prover_prove_scalar_muls(self._h, _ptr(points), _ptr(scalars), scalars.shape[0], count, _ptr(offset), out,
                                                        _ptr(products), _ptr(infinity), _ptr(ios)))
        return self._proofs(out, len(ios)), products, infinity, ios

    def prove_mul_by_cofactor(self, points):
        """Cofactor clearing of twist points (g2/circuit.rs:335-367; sbn_batch_prover_prove_mul_by_cofactor): (2p - r) x for every
        point, the generator as offset.  Returns (proofs, cleared, infinity, ios).  A G2ExpStark batch prover only."""
        points = np.ascontiguousarray(points, dtype=np.uint32)
        if points.ndim != 2 or points.shape[1] != 32:
            raise SbnError(-1, "points must be [count][32] u32")
        count = points.shape[0]
        ios, out = self._unit_buffers(count, 72)
        cleared = np.zeros((count, 32), dtype=np.uint32)
        infinity = np.zeros(count, dtype=np.uint8)
        _check(lib().sbn_batch_prover_prove_mul_by_cofactor(self._h, _ptr(points), count, out, _ptr(cleared), _ptr(infinity), _ptr(ios)))
        return self._proofs(out, len(ios)), cleared, infinity, ios

    def prove_msms(self, terms, lengths, starts=None):
        """A batch of short MSMs of any total length (arguments as msm_batch_instances) proved as units of the table, segments
        sharing units and the last unit padded (sbn_batch_prover_prove_msm_batch).  Returns (proofs, finals, sums, infinity, ios)."""
        terms, lengths, starts, xw, ew, curve = _msm_batch_args(self.stark, terms, lengths, starts)
        ios, out = self._unit_buffers(terms.shape[0], 2 * xw + ew)
        finals, sums, infinity = _msm_batch_outputs(len(lengths), xw, curve)
        _check(lib().sbn_batch_prover_prove_msm_batch(self._h, _ptr(terms), _ptr(lengths), len(lengths), _ptr(starts),
                                                      starts.shape[0] if starts is not None else 1, out, _ptr(finals), _ptr(sums), _ptr(infinity), _ptr(ios)))
        return self._proofs(out, len(ios)), finals, sums, infinity, ios

    def prove_msms_complete(self, terms, lengths, term_infinity=None):
        """A batch of short MSMs of any total length with the starts picked by the library (arguments as
        msm_batch_instances_complete; sbn_batch_prover_prove_msm_batch_complete).  Returns (proofs, terms_eff, starts, choice,
        finals, sums, infinity, ios); verify with verify_msms(stark, cfg, proofs, lengths, starts=starts, terms=terms_eff)."""
        terms, lengths, term_infinity, xw, ew = _complete_args(self.stark, terms, lengths, term_infinity)
        ios, out = self._unit_buffers(terms.shape[0], 2 * xw + ew)
        eff, starts, choice, finals, sums, infinity = _complete_outputs(terms.shape[0], len(lengths), xw, ew)
        _check(lib().sbn_batch_prover_prove_msm_batch_complete(self._h, _ptr(terms), _ptr(term_infinity), _ptr(lengths), len(lengths), out, _ptr(eff),
                                                               _ptr(starts), _ptr(choice), _ptr(finals), _ptr(sums), _ptr(infinity), _ptr(ios)))
        return self._proofs(out, len(ios)), eff, starts, choice, finals, sums, infinity, ios

    def prove_scalar_muls_complete(self, points, scalars, point_infinity=None):
        """Independent scalar multiplications e_k x_k of any count as complete sums of length 1 (points (count, 16E), scalars
        (count, 8) or one shared scalar, as prove_scalar_muls takes them; point_infinity (count,) bytes or None).  Returns (proofs,
        products, infinity, terms_eff, starts); verify with verify_msms(stark, cfg, proofs, np.ones(count), starts=starts,
        terms=terms_eff)."""
        points, scalars, _, w = _scalar_mul_args(self.stark, points, scalars, None)
        count = points.shape[0]
        terms = np.concatenate([points, np.broadcast_to(scalars, (count, 8))], axis=1)
        proofs, eff, starts, _, _, sums, infinity, _ = self.prove_msms_complete(terms, np.ones(count, dtype=np.uint64), point_infinity)
        return proofs, sums, infinity, eff, starts

    def prove_msm_complete(self, terms, term_infinity=None):
        """One sum of e_k x_k over all the terms, a complete sum of one segment.  Returns (proofs, sum, infinity, terms_eff, start):
        sum (16E,) uint32 with infinity = 1 and zero words when it is the point at infinity; verify with verify_msms(stark, cfg,
        proofs, [M], starts=start, terms=terms_eff)."""
        terms = np.ascontiguousarray(terms, dtype=np.uint32)
        proofs, eff, starts, _, _, sums, infinity, _ = self.prove_msms_complete(terms, np.array([terms.shape[0]], dtype=np.uint64), term_infinity)
        return proofs, sums[0], int(infinity[0]), eff, starts

    def prove_powers(self, bases, exps, depth=1):
        """Powers / power towers of any count (arguments as power_instances) proved as units of the table, the last one padded
        (sbn_batch_prover_prove_powers).  Returns (proofs, powers, ios)."""
        bases, exps, depth, w, ew = _power_args(self.stark, bases, exps, depth)
        count = bases.shape[0]
        ios, out = self._unit_buffers(count * depth, 2 * w + ew)
        powers = np.zeros((count, depth, w), dtype=np.uint32)
        _check(lib().sbn_batch_prover_prove_powers(self._h, _ptr(bases), _ptr(exps), exps.shape[0], count, depth, out, _ptr(powers), _ptr(ios)))
        return self._proofs(out, len(ios)), powers, ios

    def prove_bn_x_powers(self, fs):
        """f^x, f^(x^2), f^(x^3) for the BN parameter x = BN_X and every f of fs ((count, 96) uint32): towers of depth 3 with the
        shared exponent BN_X, what the hard part of the final exponentiation starts from.  Returns (proofs, powers, ios), powers
        (count, 3, 96).  A Fq12ExpU64Stark batch prover only."""
        if self.stark.kind != AIR_FQ12_EXP_U64:
            raise SbnError(-1, "the BN-parameter powers are a call of Fq12ExpU64Stark")
        return self.prove_powers(fs, BN_X, depth=3)

    def prove_program(self, nodes, values, exps):
        """A program of any count (arguments as program_instances) proved as units of the table, the last one padded
        (sbn_batch_prover_prove_program).  Returns (proofs, outs, ios)."""
        nodes, values, exps, w, ew = _program_args(self.stark, nodes, values, exps)
        count = nodes.shape[0]
        ios, out = self._unit_buffers(count, 2 * w + ew)
        outs = np.zeros((count, w), dtype=np.uint32)
        _check(_program_fn(nodes, "sbn_batch_prover_prove_program")(self._h, _ptr(nodes), count, _ptr(values), values.shape[0], _ptr(exps), exps.shape[0],
                                                    out, _ptr(outs), _ptr(ios)))
        return self._proofs(out, len(ios)), outs, ios

    def prove_final_exponentiations(self, fs, f_invs=None):
        """The final exponentiations f^((p^12 - 1) / r) of fs ((count, 96) uint32) as one program of 16 * count nodes through
        prove_program (final_exponentiation; links never leave their own 16 nodes); f_invs default to fq12_inverse.  Returns
        (proofs, results, ios), results (count, 96).  A Fq12ExpU64Stark batch prover only."""
        nodes, values, exps = _final_exp_program(self.stark, fs, f_invs)
        proofs, outs, ios = self.prove_program(nodes, values, exps)
        return proofs, outs[FINAL_EXP_NODES - 1::FINAL_EXP_NODES].copy(), ios

    def prove_curve_program(self, nodes, points, exps):
        """A curve program of any count (arguments as curve_program_instances) proved as units of the table, the last one padded
        (sbn_batch_prover_prove_curve_program).  Returns (proofs, outs, values, infinity, choice, ios)."""
        nodes, points, exps, w = _curve_program_args(self.stark, nodes, points, exps)
        count = nodes.shape[0]
        ios, out = self._unit_buffers(count, 2 * w + 8)
        outs, values, infinity, choice = _curve_program_outputs(count, w)
        _check(lib().sbn_batch_prover_prove_curve_program(self._h, _ptr(nodes), count, _ptr(points), points.shape[0], _ptr(exps), exps.shape[0],
                                                          out, _ptr(outs), _ptr(values), _ptr(infinity), _ptr(choice), _ptr(ios)))
        return self._proofs(out, len(ios)), outs, values, infinity, int(choice[0]), ios

    def close(self):
        if self._h:
            lib().sbn_batch_prover_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prove(stark, config, trace_poly_values, public_inputs, timing=None):
    """starky `prove(stark, &config, trace_poly_values, public_inputs, &mut timing)`."""
    trace = np.ascontiguousarray(trace_poly_values, dtype=np.uint64)
    pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    n = trace.shape[1]
    if trace.shape[0] != stark.num_columns or n & (n - 1):
        raise SbnError(-1, "trace shape does not match the table")
    h = C.c_void_p()
    _check(lib().sbn_prove(C.byref(stark._d), C.byref(config._c), _ptr(trace), n.bit_length() - 1, _ptr(pi), len(pi), C.byref(h)))
    return _take_proof(h)


def prove_columns(stark, config, columns, public_inputs, reduce=False):
    """prove() for a trace held as separate columns (Prover.prove_host_columns says which forms), through the same context cache."""
    t = _column_pointers(columns, stark.num_columns)
    n = t.n
    if n == 0 or n & (n - 1):
        raise SbnError(-1, "trace shape does not match the table")
    pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    h = C.c_void_p()
    _check(lib().sbn_prove_columns(C.byref(stark._d), C.byref(config._c), _ptr(t.addr), len(t), n.bit_length() - 1, TRACE_REDUCE if reduce else 0,
                                   _ptr(pi), len(pi), C.byref(h)))
    return _take_proof(h)


def prove_rows(stark, config, rows, public_inputs, reduce=False):
    """prove() for a ROW-major trace (Prover.load_trace_rows says which forms and widths), through the same context cache."""
    t = _row_table(rows)
    pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    h = C.c_void_p()
    _check(lib().sbn_prove_rows(C.byref(stark._d), C.byref(config._c), C.byref(t.raw), TRACE_REDUCE if reduce else 0, _ptr(pi), len(pi), C.byref(h)))
    return _take_proof(h)


def prove_cache_configure(budget_bytes):
    """Let prove() keep its device contexts, up to budget_bytes of device memory (least recently used evicted first); 0 (the
    default) creates and destroys one per call and releases what is cached."""
    _check(lib().sbn_prove_cache_configure(int(budget_bytes)))


def prove_cache_stats():
    out = (C.c_uint64 * 6)()
    _check(lib().sbn_prove_cache_stats(out))
    return dict(zip(("hits", "misses", "evictions", "contexts_resident", "bytes_resident", "budget"), (int(v) for v in out)))


def first_non_canonical(words, on_device=True):
    """Index of the first word >= p of a uint64 array, or len(words): the scan of Prover.prove_host_trace (test hook).
    on_device=False runs a host loop and needs no device."""
    w = np.asarray(words)
    if w.dtype != np.uint64 or w.ndim != 1 or not w.flags.c_contiguous:
        w = np.ascontiguousarray(w, dtype=np.uint64).reshape(-1)
    out = C.c_uint64(0)
    _check(lib().sbn_first_non_canonical(_ptr(w), len(w), 1 if on_device else 0, C.byref(out)))
    return int(out.value)


def verify_stark_proof(stark, proof, config):
    """starky `verify_stark_proof(stark, proof, &config)`; raises SbnError when rejected."""
    b = proof.to_bytes() if isinstance(proof, Proof) else bytes(proof)
    buf = (C.c_uint8 * len(b)).from_buffer_copy(b)
    _check(lib().sbn_verify(C.byref(stark._d), C.byref(config._c), buf, len(b)))


def verify_msm(stark, config, proofs, count, start, terms=None, verifier=None):
    """Verifies the unit proofs of a long chained list (BatchProver.prove_msm) and then checks that they link up
    (msm_check_links): with the host verifier, or on the device with `verifier` (a Verifier of the table).  Returns the last
    output in the word shape of start; raises SbnError when a unit is rejected (naming the unit) or a link breaks."""
    proofs = list(proofs)
    _verify_units(stark, config, proofs, verifier)
    return msm_check_links(stark, [p.public_inputs() for p in proofs], count, start, terms)


def _verify_units(stark, config, proofs, verifier):
    """Every unit proof verifies: the host verifier, or `verifier` in batches; raises SbnError naming the unit."""
    if verifier is None:
        for u, p in enumerate(proofs):
            try:
                verify_stark_proof(stark, p, config)
            except SbnError as e:
                raise SbnError(e.code, f"unit {u}: {e}") from None
    else:
        for at in range(0, len(proofs), verifier.max_batch):
            for i, (code, reason) in enumerate(verifier.verify(proofs[at:at + verifier.max_batch])):
                if code != 0:
                    raise SbnError(code, f"unit {at + i}: {reason}")


def verify_scalar_muls(stark, config, proofs, points, scalars, offset=None, verifier=None):
    """Verifies the unit proofs of BatchProver.prove_scalar_muls (host verifier, or a Verifier of the table in batches) and then
    runs scalar_mul_check on their public inputs.  Returns (products, infinity); raises SbnError when a unit is rejected (naming
    the unit) or the check fails (naming the instance and field)."""
    proofs = list(proofs)
    _verify_units(stark, config, proofs, verifier)
    return scalar_mul_check(stark, [p.public_inputs() for p in proofs], points, scalars, offset)


def verify_mul_by_cofactor(stark, config, proofs, points, verifier=None):
    """verify_scalar_muls for BatchProver.prove_mul_by_cofactor: returns (cleared, infinity)."""
    proofs = list(proofs)
    _verify_units(stark, config, proofs, verifier)
    return mul_by_cofactor_check(stark, [p.public_inputs() for p in proofs], points)


def verify_msms(stark, config, proofs, lengths, starts=None, terms=None, verifier=None):
    """Verifies the unit proofs of BatchProver.prove_msms (host verifier, or a Verifier of the table in batches) and then runs
    msm_batch_check on their public inputs.  Returns (finals, sums, infinity); raises SbnError when a unit is rejected (naming the
    unit) or the check fails (naming the instance, its segment and the field)."""
    proofs = list(proofs)
    _verify_units(stark, config, proofs, verifier)
    return msm_batch_check(stark, [p.public_inputs() for p in proofs], lengths, starts, terms)


def verify_powers(stark, config, proofs, bases, exps, depth=1, verifier=None):
    """Verifies the unit proofs of BatchProver.prove_powers (host verifier, or a Verifier of the table in batches) and then runs
    power_check on their public inputs.  Returns the powers (count, depth, W); raises SbnError when a unit is rejected (naming the
    unit) or the check fails (naming the instance and field)."""
    proofs = list(proofs)
    _verify_units(stark, config, proofs, verifier)
    return power_check(stark, [p.public_inputs() for p in proofs], bases, exps, depth)


def verify_program(stark, config, proofs, nodes, values, exps, verifier=None):
    """Verifies the unit proofs of BatchProver.prove_program (host verifier, or a Verifier of the table in batches) and then runs
    program_check on their public inputs.  Returns the outputs (count, W); raises SbnError when a unit is rejected (naming the
    unit) or the check fails (naming the instance and field)."""
    proofs = list(proofs)
    _verify_units(stark, config, proofs, verifier)
    return program_check(stark, [p.public_inputs() for p in proofs], nodes, values, exps)


def verify_curve_program(stark, config, proofs, nodes, points, exps, choice, verifier=None):
    """Verifies the unit proofs of BatchProver.prove_curve_program (host verifier, or a Verifier of the table in batches) and then
    runs curve_program_check on their public inputs.  Returns (values, infinity); raises SbnError when a unit is rejected (naming
    the unit) or the check fails (naming the instance and field)."""
    proofs = list(proofs)
    _verify_units(stark, config, proofs, verifier)
    _, values, infinity = curve_program_check(stark, [p.public_inputs() for p in proofs], nodes, points, exps, choice)
    return values, infinity


def verify_bn_x_powers(stark, config, proofs, fs, verifier=None):
    """verify_powers for BatchProver.prove_bn_x_powers: returns (count, 3, 96) = f^x, f^(x^2), f^(x^3) per input."""
    if stark.kind != AIR_FQ12_EXP_U64:
        raise SbnError(-1, "the BN-parameter powers are a call of Fq12ExpU64Stark")
    return verify_powers(stark, config, proofs, fs, BN_X, depth=3, verifier=verifier)


class Verifier:
    """Batch verifier on the device for proofs of one (table, config, degree_bits): the Merkle hashing and the reduction of the
    opened rows run on the GPU, up to max_batch proofs per call.  Needs a device (SbnError(-3) otherwise): verify_stark_proof
    is the host verifier."""

    def __init__(self, stark, config, degree_bits, max_batch=64):
        self.stark, self.config, self.degree_bits, self.max_batch = stark, config, degree_bits, max_batch
        self._h = C.c_void_p()
        _check(lib().sbn_verifier_create(C.byref(stark._d), C.byref(config._c), degree_bits, max_batch, C.byref(self._h)))

    def verify(self, proofs):
        """proofs: Proof objects or byte strings -> [(code, reason)] in order: what sbn_verify returns for each (0, "" = accepted).
        Raises SbnError when the call itself is refused (an empty list, more than max_batch proofs, a HIP failure)."""
        bufs = [p.to_bytes() if isinstance(p, Proof) else bytes(p) for p in proofs]
        n = len(bufs)
        ptrs = (C.c_char_p * max(n, 1))(*bufs)
        lens = (C.c_size_t * max(n, 1))(*[len(b) for b in bufs])
        status = (C.c_int32 * max(n, 1))()
        _check(lib().sbn_verifier_verify(self._h, ptrs, lens, n, status))
        return [(int(status[i]), lib().sbn_verifier_reason(self._h, i).decode()) for i in range(n)]

    def stage_times(self):
        """Device times of the last verify() in ms (HIP events): upload, kernels, download."""
        buf = (C.c_float * 3)()
        k = lib().sbn_verifier_stage_times(self._h, buf, 3)
        return dict(zip(("upload", "kernels", "download"), (float(buf[i]) for i in range(k))))

    def close(self):
        if self._h:
            lib().sbn_verifier_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def commit_values(cols, rate_bits=1, cap_height=4, want_coeffs=False, want_lde=False):
    """PolynomialBatch::from_values on the device -> (cap, coeffs, lde)."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    ncols, n = cols.shape
    cap = np.zeros((1 << cap_height, 4), dtype=np.uint64)
    coeffs = np.zeros_like(cols) if want_coeffs else None
    lde = np.zeros((ncols, n << rate_bits), dtype=np.uint64) if want_lde else None
    _check(lib().sbn_commit_values(_ptr(cols), ncols, n, rate_bits, cap_height, _ptr(cap), _ptr(coeffs), _ptr(lde)))
    return cap, coeffs, lde


def prover_memory_plan(stark, config, degree_bits, lde="full"):
    """Device bytes Prover(stark, config, degree_bits, lde=lde) allocates at creation; needs no device.  lde=None: no options."""
    out = C.c_uint64(0)
    _check(lib().sbn_prover_memory_plan(C.byref(stark._d), C.byref(config._c), degree_bits, _opt_ref(_prover_options(lde)), C.byref(out)))
    return int(out.value)


def lde_rows(cols, rate_bits, leaf_indices):
    """Rows of the coset LDE of `cols` (ncols, n) at Merkle leaf indices `leaf_indices`, evaluated from the coefficients by the
    kernels of the compact storage -> (len(leaf_indices), ncols)."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    idx = np.ascontiguousarray(leaf_indices, dtype=np.uint32)
    ncols, n = cols.shape
    out = np.zeros((len(idx), ncols), dtype=np.uint64)
    _check(lib().sbn_lde_rows(_ptr(cols), ncols, max(n.bit_length() - 1, 0), rate_bits, _ptr(idx), len(idx), _ptr(out)))
    return out


def poseidon_permute_batch(states):
    s = np.ascontiguousarray(states, dtype=np.uint64).copy()
    _check(lib().sbn_poseidon_permute_batch(_ptr(s), s.shape[0]))
    return s


def poseidon_permute_coop_batch(states):
    """The permutation of (count, 12) states through the 16-lane cooperative form (one lane group per state)."""
    s = np.ascontiguousarray(states, dtype=np.uint64).copy()
    _check(lib().sbn_poseidon_permute_coop_batch(_ptr(s), s.shape[0]))
    return s


def field_mul_batch(a, b, mode=0):
    """a[i] * b[i] mod p with the device multiply (mode 0: the canonical operator* of every kernel; 1: the transforms' weak product),
    on arbitrary 64-bit representatives; canonical results."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    out = np.zeros_like(a)
    _check(lib().sbn_field_mul_batch(_ptr(a), _ptr(b), _ptr(out), a.shape[0], mode))
    return out


BN254_FQ_OPS = {"mul": 0, "add": 1, "sub": 2, "inv": 3, "batch_inv": 4, "fq2_inv": 5}   # sbn_bn254_fq_batch (include/sbn.h)


def bn254_fq_batch(op, a, b=None, on_device=True):
    """The BN254 base-field helpers of the witness generators on Python ints below p (test hook): op in BN254_FQ_OPS; a, b lists of
    ints.  Returns a list of ints, or of (c0, c1) pairs for "fq2_inv" (a = c0, b = c1).  on_device=False runs the host build."""
    def words(vals):
        return np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in vals], dtype=np.uint64).reshape(len(vals), 4)
    code = BN254_FQ_OPS[op]
    wa = words(a)
    wb = words(b) if b is not None else None
    out = np.zeros((len(a), 2 if op == "fq2_inv" else 1, 4), dtype=np.uint64)
    _check(lib().sbn_bn254_fq_batch(code, _ptr(wa), _ptr(wb), _ptr(out), len(a), 1 if on_device else 0))
    vals = [[sum(int(w) << (64 * j) for j, w in enumerate(e)) for e in row] for row in out]
    return [tuple(v) for v in vals] if op == "fq2_inv" else [v[0] for v in vals]


def eval_constraints_host(stark, local_row, next_row, public_inputs, alphas, z_last, l_first, l_last):
    """The table's AIR constraints folded into the two Horner accumulators on one row pair (host, base field)."""
    lv = np.ascontiguousarray(local_row, dtype=np.uint64)
    nv = np.ascontiguousarray(next_row, dtype=np.uint64)
    pi = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    al = np.array(alphas, dtype=np.uint64)
    acc = np.zeros(2, dtype=np.uint64)
    L = lib()
    L.sbn_eval_constraints_host.argtypes = [C.POINTER(_AirDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint64,
                                            C.c_uint64, C.c_void_p]
    _check(L.sbn_eval_constraints_host(C.byref(stark._d), _ptr(lv), _ptr(nv), _ptr(pi), len(pi), _ptr(al), z_last, l_first, l_last, _ptr(acc)))
    return [int(x) for x in acc]


def poseidon_permute_host(states, use_definition=False):
    """The transcript's host permutation (no device): sparse partial rounds, or the plain definition."""
    s = np.ascontiguousarray(states, dtype=np.uint64).copy()
    _check(lib().sbn_poseidon_permute_host(_ptr(s), s.shape[0], 1 if use_definition else 0))
    return s
