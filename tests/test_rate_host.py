"""rate_bits 3 (a blowup of 8, plonky2's recursion config) on the CPU: the host verifier against the oracle at that rate
(tests/rate_oracle.py), the config helpers and the refusals that are answered before a device is looked for.  The device prover
runs the same tables and rows against the same oracle in test_rate_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import config_matrix as M
import rate_cases as RC

TABLES = ["g1op", "modular", "lookup", "flags"]   # hashed leaves; wide; <= 4 columns (a leaf is its own digest); no Z columns


@pytest.fixture(scope="module")
def R(O):
    import rate_oracle
    rate_oracle.lib()
    return rate_oracle


@pytest.fixture(scope="module")
def proofs(S, O, R):
    return RC.Proofs(S, O, R)


def test_the_shim_at_rate_1_is_the_oracle(O, R, g1op_case):
    words, _ = R.prove(O.AIR_G1_OP, 0, g1op_case["trace"], RC.NO_PI, 1, M.DEFAULT)
    assert np.array_equal(words, g1op_case["proof"])
    assert R.verify(O.AIR_G1_OP, 0, words, 1, M.DEFAULT) == (0, "")


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_host_verifier_accepts_the_oracles_rate_3_proofs(S, R, proofs, table, case):
    stark, kind, num_io, trace = proofs.table(table)
    row, times_x = case
    ocfg = row + (times_x,)
    words = proofs(table, case)
    assert R.verify(kind, num_io, words, 3, ocfg) == (0, "")
    h = M.header(words)
    degree_bits = trace.shape[1].bit_length() - 1
    assert (h[0], h[5], h[6], h[8], h[10]) == (degree_bits, row[0], 3, row[2], row[4])
    assert (h[7], h[9]) == M.fri_shape(degree_bits, row, 3)
    cfg = RC.make_config(S, case)
    assert RC.product_code(S, stark, words, cfg) == 0
    # one changed word in each section: both verifiers reject, the product's with SBN_ERR_VERIFY_FAILED
    sections = M.section_words(words)
    assert ("fri_step" in sections) == (h[7] > 0)
    for name, idx in sections.items():
        bad = M.bump(words, idx)
        assert R.verify(kind, num_io, bad, 3, ocfg)[0] != 0, name
        assert RC.product_code(S, stark, bad, cfg) == -6, name


@pytest.mark.parametrize("table", ["g1op", "lookup"])
def test_a_proof_under_the_other_rate_is_a_shape_refusal(S, O, R, proofs, g1op_case, table):
    stark, kind, num_io, _ = proofs.table(table)
    case = (RC.ROWS[0], True)
    r3, r1 = proofs(table, case), proofs(table, case, 1)
    assert RC.product_code(S, stark, r1, RC.make_config(S, case, 1)) == 0
    assert RC.product_code(S, stark, r3, RC.make_config(S, case, 1)) == -5
    assert RC.product_code(S, stark, r1, RC.make_config(S, case, 3)) == -5
    assert R.verify(kind, num_io, r3, 1, case[0])[0] != 0 and R.verify(kind, num_io, r1, 3, case[0])[0] != 0


def test_config_helpers(S):
    std, c1 = S.StarkConfig(), S.StarkConfig.for_rate(1)
    for name, _ in S.api._Config._fields_:
        assert getattr(c1, name) == getattr(std, name), name
    assert "sbn_config_for_rate" in S.EXPORTS and hasattr(S.lib(), "sbn_config_for_rate")
    want = {1: 84, 2: 42, 3: 28}
    for r, q in want.items():
        c = S.StarkConfig.for_rate(r)
        assert (c.rate_bits, c.num_query_rounds) == (r, q)
        assert c.rate_bits * c.num_query_rounds + c.proof_of_work_bits >= c.security_bits
        for name, _ in S.api._Config._fields_:
            if name not in ("rate_bits", "num_query_rounds"):
                assert getattr(c, name) == getattr(std, name), name


def create_codes(S, stark, cfg, degree_bits):
    """(sbn_prover_create, sbn_verifier_create): 0 and -3 (no device) both mean "got past the checks"."""
    out = []
    for make in (lambda: S.Prover(stark, cfg, degree_bits), lambda: S.Verifier(stark, cfg, degree_bits, 4)):
        try:
            make().close()
            out.append(0)
        except S.SbnError as e:
            out.append(0 if e.code == -3 else e.code)
    return tuple(out)


def test_heights_and_rates_still_refused(S):
    """degree_bits + rate_bits <= 23, checked before a device is looked for; rate_bits 4 and up stay refused."""
    stark = S.LookupStark()
    c3, c1 = S.StarkConfig.for_rate(3), S.StarkConfig.for_rate(1)
    assert create_codes(S, stark, c3, 21) == (-7, -7)
    assert "2^23" in S.lib().sbn_last_error().decode()
    assert create_codes(S, stark, c1, 23) == (-7, -7) and create_codes(S, stark, c3, 8) == (-7, -7)
    for r in (4, 5, 31):
        c = S.StarkConfig.for_rate(3)
        c.rate_bits = r
        assert create_codes(S, stark, c, 9) == (-7, -7), r
        assert RC.product_code(S, stark, np.zeros(16, dtype=np.uint64), c) == -7


def test_accepted_heights_get_past_the_checks(S):
    stark = S.LookupStark()
    assert create_codes(S, stark, S.StarkConfig.for_rate(3), 9) == (0, 0)
    if S.lib().sbn_device_count() == 0:   # (with a device these would allocate the largest contexts; the answer is the same)
        assert create_codes(S, stark, S.StarkConfig.for_rate(3), 20) == (0, 0)
        assert create_codes(S, stark, S.StarkConfig.for_rate(1), 22) == (0, 0)


def test_the_split_prover_refuses_rate_3_for_every_world(S):
    from starky_bn254_amd import split
    L = S.lib()
    split._bind(L)
    stark = S.G1ExpStark(128)
    for cfg, want in ((S.StarkConfig.for_rate(3), -7), (S.StarkConfig.for_rate(1), 0)):
        for world in (1, 2, 4):
            sb, rb = C.c_uint64(), C.c_uint64()
            assert L.sbn_split_exchange_bytes(C.byref(stark._d), C.byref(cfg._c), 16, world, C.byref(sb), C.byref(rb)) == want, world
    comm = split._Comm()
    comm.struct_size, comm.rank, comm.world = C.sizeof(split._Comm), 0, 1
    h = C.c_void_p()
    assert L.sbn_split_prover_create(C.byref(stark._d), C.byref(S.StarkConfig.for_rate(3)._c), 16, C.byref(comm), C.byref(h)) == -7
    assert not h.value and "rate_bits" in L.sbn_last_error().decode()
