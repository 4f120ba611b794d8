"""The StarkConfig matrix shared by test_config_matrix.py (CPU: oracle and host verifier) and test_config_matrix_gpu.py (device
prover).  A row is (cap_height, proof_of_work_bits, fri_arity_bits, fri_final_poly_bits, num_query_rounds); every value lies in
the range config_supported() lets through (csrc/host_common.hpp).  32 proof-of-work bits are left out: 2^32 hashes of grinding
run no code the 20-bit row does not."""
import numpy as np

DEFAULT = (4, 16, 4, 5, 84)

# row -> (FRI layers, final-polynomial length) of a 512-row table, as the oracle produced them when the matrix was written;
# fri_shape() below must give the same
MATRIX = {
    (1, 16, 4, 5, 84): (1, 32), (8, 16, 4, 5, 84): (0, 512), (4, 0, 4, 5, 84): (1, 32), (4, 20, 4, 5, 84): (1, 32),
    (4, 16, 1, 5, 84): (4, 32), (4, 16, 2, 5, 84): (2, 32), (4, 16, 3, 5, 84): (2, 8), (4, 16, 4, 0, 84): (1, 32),
    (4, 16, 4, 9, 84): (0, 512), (4, 16, 4, 12, 84): (0, 512), (4, 16, 4, 5, 1): (1, 32), (4, 16, 4, 5, 512): (1, 32),
    (8, 8, 1, 0, 3): (2, 128), (1, 0, 3, 2, 200): (3, 1), (6, 16, 2, 3, 28): (2, 32),
}
# the rows that also run without the times-X step (fri_variant = SBN_FRI_PLAIN): every arity-2 row and every zero-layer row
PLAIN_TOO = [(4, 16, 1, 5, 84), (8, 8, 1, 0, 3), (8, 16, 4, 5, 84), (4, 16, 4, 9, 84), (4, 16, 4, 12, 84)]
# (row, times_x) of every case
CASES = [(row, True) for row in MATRIX] + [(row, False) for row in PLAIN_TOO]
# the rows of the wide table: the three non-default arities, cap height 1 and cap height 8
WIDE_ROWS = [(4, 16, 1, 5, 84), (4, 16, 2, 5, 84), (4, 16, 3, 5, 84), (1, 16, 4, 5, 84), (8, 16, 4, 5, 84)]


def case_id(case):
    row, times_x = case
    return "-".join(str(v) for v in row) + ("" if times_x else "-plain")


def fri_shape(degree_bits, row, rate_bits=1):
    """plonky2 FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits) -> (layers, final-polynomial length)."""
    cap, _, arity, final, _ = row
    d, layers = degree_bits, 0
    while d > final and d + rate_bits - arity >= cap:
        d, layers = d - arity, layers + 1
    return layers, 1 << d


def make_config(S, row, times_x=True):
    """The product's StarkConfig of a row."""
    cfg = S.StarkConfig()
    cfg.cap_height, cfg.proof_of_work_bits, cfg.fri_arity_bits, cfg.fri_final_poly_bits, cfg.num_query_rounds = row
    cfg.fri_variant = S.api.FRI_TIMES_X if times_x else S.api.FRI_PLAIN
    return cfg


def header(words):
    """(degree_bits, ncol, nz, nq, npi, cap_height, rate_bits, layers, arity_bits, final length, queries) of a proof."""
    return tuple(int(x) for x in words[1:12])


def check_header(words, degree_bits, row):
    """The proof's header carries the row: cap height, arity, query rounds, and the FRI shape fri_shape() derives from it."""
    h = header(words)
    assert (h[0], h[5], h[8], h[10]) == (degree_bits, row[0], row[2], row[4]) and (h[7], h[9]) == fri_shape(degree_bits, row), (h, row)


def difference(got, want, permute):
    """None where the two proofs are equal word for word; else a sentence that names the first differing word and, through the
    parity kit, the first stage that differs (permute: the oracle's Poseidon permutation)."""
    if np.array_equal(got, want):
        return None
    import parity_kit as K
    k = min(len(want), len(got))
    diff = np.nonzero(np.asarray(got[:k]) != np.asarray(want[:k]))[0]
    stage = K.first_difference(K.stage_digests(got, permute), K.stage_digests(want, permute)) if len(got) == len(want) else None
    return (f"{len(got)} / {len(want)} words, first differing word {int(diff[0]) if diff.size else k}, sections at {section_words(want)}, "
            f"first differing stage {stage}")


def section_words(words):
    """One word index inside each section of a proof (layout: include/sbn.h): a cap, an opening, the final polynomial and -- where
    the proof has FRI layers -- the first evaluation of the first query's first FRI step."""
    degree_bits, ncol, nz, nq, npi, cap_h, rate_bits, layers, arity_bits, fpl, _ = header(words)
    capw, sib = 4 << cap_h, 4 * (degree_bits + rate_bits - cap_h)
    openings = 12 + (3 if nz else 2) * capw
    queries = openings + 2 * (2 * ncol + 2 * nz + nq) + layers * capw
    out = {"cap": 12 + capw - 3, "opening": openings + 3, "final_poly": len(words) - npi - 1 - 2 * fpl + 1}
    if layers:
        out["fri_step"] = queries + sum(wd + sib for wd in ([ncol] + ([nz] if nz else []) + [nq]))
    return out


def bump(words, idx):
    t = np.array(words, dtype=np.uint64, copy=True)
    t[idx] = (int(t[idx]) + 1) % 0xFFFFFFFF00000001
    return t
