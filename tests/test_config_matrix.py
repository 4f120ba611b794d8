"""Every StarkConfig the library accepts, on the CPU: the oracle proves and verifies each row of tests/config_matrix.py, and the
product's HOST verifier (sbn_verify needs no device) must agree with it -- accept the oracle's proof under the same config, reject a
changed word in every section, and answer a config that differs in one field the way the proof header and the proof-of-work bound
say.  The device prover runs the same rows against the same oracle in test_config_matrix_gpu.py."""
import numpy as np
import pytest

import config_matrix as M

ROWS = 512
NO_PI = np.zeros(0, dtype=np.uint64)


@pytest.fixture(scope="module")
def tables(S, O, g1op_case):
    """G1Stark (hashed leaves) and LookupStark (4 columns and 2 Zs: leaves that are their own digests), 512 rows each."""
    ins, tab = O.lookup_inputs(ROWS, 9)
    return {"g1op": (S.G1Stark(), O.AIR_G1_OP, g1op_case["trace"]), "lookup": (S.LookupStark(), O.AIR_LOOKUP, O.lookup_trace(ins, tab))}


@pytest.fixture(scope="module")
def proofs(O, tables):
    """The oracle's proof of every (table, case), made once."""
    cache = {}

    def get(table, case):
        if (table, case) not in cache:
            _, kind, trace = tables[table]
            cache[(table, case)] = O.prove(kind, 0, trace, NO_PI, config=case[0] + (case[1],))[0]
        return cache[(table, case)]
    return get


def expected_code(made, asked):
    """What a verifier configured with `asked` must say about a proof made under `made` (both (row, times_x)): -5 when the header the
    config implies differs (cap height, arity, query count, layer count, final length), else -6 when the proof-of-work bound is
    stricter than the one the witness was ground for or the FRI variant differs, else 0."""
    (a, ax), (b, bx) = made, asked
    if (a[0], a[2], a[4]) + M.fri_shape(9, a) != (b[0], b[2], b[4]) + M.fri_shape(9, b):
        return -5
    return -6 if (b[1] > a[1] or ax != bx) else 0


def product_code(S, stark, words, case):
    try:
        S.verify_stark_proof(stark, S.Proof(np.asarray(words, dtype=np.uint64), 9), M.make_config(S, *case))
    except S.SbnError as e:
        return e.code
    return 0


def test_fri_shape_restatement_matches_the_recorded_shapes():
    for row, shape in M.MATRIX.items():
        assert M.fri_shape(9, row) == shape, row
    assert M.fri_shape(9, M.DEFAULT) == (1, 32) and M.fri_shape(16, M.DEFAULT) == (3, 16) and M.fri_shape(18, M.DEFAULT) == (3, 64)


def test_default_config_entry_point_is_unchanged(O, g1op_case):
    """config=None, the default row and the product's default StarkConfig object all give the words of the fixture's plain call."""
    words, _ = O.prove(O.AIR_G1_OP, 0, g1op_case["trace"], NO_PI, config=M.DEFAULT)
    assert np.array_equal(words, g1op_case["proof"])
    assert O.verify(O.AIR_G1_OP, 0, words, config=M.DEFAULT) == (0, "")
    try:
        O.set_final_poly_times_x(False)
        plain, _ = O.prove(O.AIR_G1_OP, 0, g1op_case["trace"], NO_PI)
        assert O.verify(O.AIR_G1_OP, 0, plain) == (0, "")
    finally:
        O.set_final_poly_times_x(True)
    assert np.array_equal(plain, O.prove(O.AIR_G1_OP, 0, g1op_case["trace"], NO_PI, config=M.DEFAULT + (False,))[0])
    assert not np.array_equal(plain, words)
    assert O.verify(O.AIR_G1_OP, 0, plain)[0] != 0 and O.verify(O.AIR_G1_OP, 0, plain, config=M.DEFAULT + (False,)) == (0, "")


@pytest.mark.parametrize("table", ["g1op", "lookup"])
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_oracle_and_host_verifier_agree(S, O, tables, proofs, table, case):
    stark, kind, _ = tables[table]
    row, times_x = case
    ocfg = row + (times_x,)
    words = proofs(table, case)
    assert O.verify(kind, 0, words, config=ocfg) == (0, "")
    h = M.header(words)
    assert (h[0], h[5], h[6], h[8], h[10]) == (9, row[0], 1, row[2], row[4])
    assert (h[7], h[9]) == M.fri_shape(9, row) == M.MATRIX[row]
    assert (h[1], h[2], h[3], h[4]) == (stark.num_columns, stark.num_permutation_zs(), 4, 0)
    assert product_code(S, stark, words, case) == 0
    # one changed word in each section: both verifiers reject, the product's with SBN_ERR_VERIFY_FAILED
    sections = M.section_words(words)
    assert ("fri_step" in sections) == (h[7] > 0)
    for name, idx in sections.items():
        bad = M.bump(words, idx)
        assert O.verify(kind, 0, bad, config=ocfg)[0] != 0, name
        assert product_code(S, stark, bad, case) == -6, name
    # a config that differs in one field (32 bits for the proof-of-work bound: a witness ground for fewer satisfies it with
    # probability 2^-12 at most), the other variant of the final polynomial, and the default config
    cap, pw, ar, fin, nq = row
    others = [((cap % 8 + 1, pw, ar, fin, nq), times_x), ((cap, 32, ar, fin, nq), times_x), ((cap, pw, ar % 4 + 1, fin, nq), times_x),
              ((cap, pw, ar, 12 if fin < 9 else 0, nq), times_x), ((cap, pw, ar, fin, nq % 512 + 1), times_x), (row, not times_x), (M.DEFAULT, True)]
    for other in others:
        want = expected_code(case, other)
        assert product_code(S, stark, words, other) == want, other
        # the oracle reads no arity from the header: with no FRI layer on either side it has nothing to tell two arities apart by
        if not (want == -5 and h[7] == 0 and expected_code(case, (other[0][:2] + (ar,) + other[0][3:], other[1])) == 0):
            assert (O.verify(kind, 0, words, config=other[0] + (other[1],))[0] == 0) == (want == 0), other


def test_the_two_rows_the_default_config_accepts(S, O, tables, proofs):
    """A stricter proof-of-work bound and a final_poly_bits that leaves the shape alone differ from the default config in nothing a
    verifier can see: both verifiers accept those proofs under the default config.  Every other row is refused under it."""
    accepted = [row for row in M.MATRIX if expected_code((row, True), (M.DEFAULT, True)) == 0]
    assert accepted == [(4, 20, 4, 5, 84), (4, 16, 4, 0, 84)]
    stark, kind, _ = tables["g1op"]
    for row in M.MATRIX:
        words = proofs("g1op", (row, True))
        want = 0 if row in accepted else (-6 if row == (4, 0, 4, 5, 84) else -5)
        assert product_code(S, stark, words, (M.DEFAULT, True)) == want, row
        assert (O.verify(kind, 0, words)[0] == 0) == (want == 0), row


@pytest.mark.parametrize("field,value", [("num_challenges", 1), ("num_challenges", 3), ("rate_bits", 0), ("rate_bits", 2), ("cap_height", 0),
                                         ("cap_height", 9), ("fri_arity_bits", 0), ("fri_arity_bits", 5), ("num_query_rounds", 0),
                                         ("num_query_rounds", 513), ("proof_of_work_bits", 33), ("fri_variant", 3)])
def test_unsupported_config_values_are_refused(S, g1op_case, field, value):
    """config_supported() runs before the device is looked for: sbn_prover_create and sbn_verify answer SBN_ERR_UNSUPPORTED."""
    stark = S.G1Stark()
    cfg = stark.config()
    setattr(cfg, field, value)
    with pytest.raises(S.SbnError) as e:
        S.Prover(stark, cfg, 9)
    assert e.value.code == -7
    with pytest.raises(S.SbnError) as e:
        S.verify_stark_proof(stark, S.Proof(g1op_case["proof"], 9), cfg)
    assert e.value.code == -7


@pytest.mark.parametrize("field,value", [("cap_height", 1), ("cap_height", 8), ("fri_arity_bits", 1), ("fri_arity_bits", 4), ("num_query_rounds", 1),
                                         ("num_query_rounds", 512), ("proof_of_work_bits", 0), ("proof_of_work_bits", 32), ("fri_final_poly_bits", 0),
                                         ("fri_final_poly_bits", 40)])
def test_the_ends_of_the_supported_ranges_pass_the_config_check(S, g1op_case, field, value):
    """The other side of the refusals: the extreme supported values get past config_supported() (the verifier then answers about the
    proof, not about the config)."""
    stark = S.G1Stark()
    cfg = stark.config()
    setattr(cfg, field, value)
    try:
        S.verify_stark_proof(stark, S.Proof(g1op_case["proof"], 9), cfg)
    except S.SbnError as e:
        assert e.code in (-5, -6)


@pytest.mark.parametrize("cap_height", [0, 9, 20, 0xFFFFFFFF])
def test_commit_values_refuses_a_cap_height_outside_1_to_8(S, cap_height):
    """sbn_commit_values checks its cap_height before it looks for a device (the tree's level count is computed unsigned)."""
    cols = np.zeros((2, 512), dtype=np.uint64)
    cap = np.zeros((1, 4), dtype=np.uint64)   # (never written: the call is refused)
    with pytest.raises(S.SbnError) as e:
        S.api._check(S.lib().sbn_commit_values(S.api._ptr(cols), 2, 512, 1, cap_height, S.api._ptr(cap), None, None))
    assert e.value.code == -7
