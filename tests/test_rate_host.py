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


# ---- tests/golden/rate3_digests.json and its generator -------------------------------------------------------------------------
EXP_DIGESTS = {"g1exp": 128, "fqexp": 128, "fq12expu64": 16, "g2exp": 128, "fq12exp": 16}   # name -> num_io
LOOKUP_DIGESTS = {"lookup18": 18, "lookup19": 19, "lookup20": 20}                            # name -> degree_bits


def is_sha256(v):
    return isinstance(v, str) and len(v) == 64 and set(v) <= set("0123456789abcdef")


def test_every_rate_3_digest_entry_has_its_fields(golden):
    g = golden["rate3_digests"]
    assert (g["rate_bits"], tuple(g["config"])) == (3, RC.ROWS[0])
    assert set(g["cases"]) == set(EXP_DIGESTS) | set(LOOKUP_DIGESTS)
    for name, num_io in EXP_DIGESTS.items():
        e = g["cases"][name]
        assert set(e) == {"num_io", "seed", "proof_words", "proof_sha256", "public_inputs_sha256"}, name
        assert e["num_io"] == num_io and is_sha256(e["proof_sha256"]) and is_sha256(e["public_inputs_sha256"]), name
    for name, bits in LOOKUP_DIGESTS.items():
        e = g["cases"][name]
        assert set(e) == {"degree_bits", "seed", "proof_words", "proof_sha256"}, name
        assert (e["degree_bits"], e["seed"]) == (bits, 200 + bits) and is_sha256(e["proof_sha256"]), name
    for name, e in g["cases"].items():
        assert isinstance(e["proof_words"], int) and e["proof_words"] > 12, name
    # four columns, two Zs, two quotient columns, no public inputs: a height only adds words to the Merkle paths and the FRI layers
    words = [g["cases"][n]["proof_words"] for n in LOOKUP_DIGESTS]
    assert words == sorted(words) and len(set(words)) == 3
    # the entries of the change that brought rate_bits 3 are the ones committed then
    assert g["cases"]["g1exp"]["proof_sha256"] == "0cc626c1219e6ee5ab63fd0af7c34215f11d98a8459428ed92427c76013c4427"
    assert g["cases"]["fqexp"]["proof_sha256"] == "5931d0e6949b503f32ae62caf2cd8b6e89b86d070a2b9d3caf3725b382a59d72"
    assert g["cases"]["fq12expu64"]["proof_sha256"] == "dfb555ea3607aa551f6cf18848b539f4d6d69150f7f2774144d9962b56083317"


def test_the_generator_reproduces_one_entry_alone(golden, tmp_path):
    """make_rate3_digests.py --only fq12expu64 (the smallest table of the file: 2^11 rows): that entry comes out as committed, every
    other entry is copied, and the committed file is not written."""
    import importlib.util
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_rate3_digests.py")
    spec = importlib.util.spec_from_file_location("make_rate3_digests", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert set(gen.NAMES) == set(EXP_DIGESTS) | set(LOOKUP_DIGESTS)
    before = os.stat(gen.JSON).st_mtime_ns
    out = tmp_path / "rate3_digests.json"
    gen.main(["--only", "fq12expu64", "--out", str(out)])
    assert json.load(open(out)) == golden["rate3_digests"]
    assert open(out).read() == open(gen.JSON).read() and os.stat(gen.JSON).st_mtime_ns == before
    with pytest.raises(SystemExit):
        gen.main(["--only", "no_such_case", "--out", str(out)])


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
