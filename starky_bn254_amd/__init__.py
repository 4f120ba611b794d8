"""starky-bn254 on MI355X: Python host-side mirror of the reference's prover interface.

Thin ctypes layer over the C ABI in include/sbn.h (libsbn254.so, built in-tree by
`make -C starky_bn254_amd/csrc`).  There is NO CPU fallback: importing works without a GPU (so the
symbol table can be checked), but every prove()/commit call fails loudly without a HIP device.
"""
from .api import (  # noqa: F401
    AIR_G1_OP, AIR_G1_EXP, AIR_G2_EXP, AIR_FQ12_EXP, AIR_FQ_EXP, AIR_FQ12_EXP_U64, AIR_MODULAR, AIR_FQ12_MUL, AIR_LOOKUP, AIR_FLAGS, AIR_FLAGS_U64, LookupStark, MyStark, FlagStark, FlagU64Stark, SbnError, StarkConfig, G1Stark, ModularStark, Fq12Stark, G1ExpStark, G2ExpStark, Fq12ExpStark,
    FqExpStark, Fq12ExpU64Stark, Prover, BatchProver, Verifier, Proof, TraceReport, check_trace_host,
    ConstraintBlock, RowExplanation, RowsExplanation, TraceExplanation, explain_rows_host, explain_trace_host,
    PermutationExplanation, explain_permutations_host, PERM_PAIR_STAT, PERM_DIFF_ENTRY,
    prove, prove_cache_configure, prove_cache_stats, first_non_canonical, verify_stark_proof, commit_values, eval_constraints_host, poseidon_permute_batch, poseidon_permute_coop_batch, poseidon_permute_host, field_mul_batch, bn254_fq_batch, chain_instances, msm_num_units, msm_instances, msm_check_links, verify_msm, lib, lib_path, EXPORTS,
    G2_COFACTOR, generator, scalar_mul_instances, scalar_mul_check, mul_by_cofactor_check, verify_scalar_muls, verify_mul_by_cofactor,
    msm_batch_instances, msm_batch_check, verify_msms,
    START_CANDIDATES, start_candidate, msm_batch_instances_complete,
    BN_P, BN_X, FQ_INVERSE_EXP, FQ_LEGENDRE_EXP, FQ_SQRT_EXP, bn_x, power_instances, power_check, verify_powers, verify_bn_x_powers, FINAL_EXP_NODES, fq12_frobenius, fq12_conjugate, fq12_inverse, final_exponentiation, verify_final_exponentiations, fq_sqrt_flags,
    NODE_OUTPUT, NODE_ONE, Program, program_levels, program_instances, program_check, verify_program,
    NODE_START, CurveProgram, curve_program_instances, curve_program_check, verify_curve_program,
    prover_memory_plan, lde_rows, LDE_STORAGE,
    TRACE_REDUCE, ColumnTable, prove_columns, gather_columns, reduce_words,
    RowTable, trace_from_rows_host, prove_rows,
    WitnessDiff, WITNESS_CELL, diff_witness_host, instances_from_public_inputs,
    GUARD, GuardStats, prove_set_guard,
)
