"""rate_bits 3 on the device (run on the MI355X box with `-m gpu`): the transforms and the leaf / Merkle kernels at rate_bits 2 and 3
through sbn_commit_values, then whole proofs word for word against the CPU oracle at that rate (tests/rate_oracle.py), the Exp
tables against committed digests of the oracle's proofs (tests/golden/rate3_digests.json), the device verifier, the batch prover,
the trace check and explain on a rate-3 context, and the refusal of the split prover.  Shapes are the smallest at which each
kernel path differs: see the parameter lists."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import config_matrix as M
import rate_cases as RC

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    return S


@pytest.fixture(scope="module")
def R(O):
    import rate_oracle
    rate_oracle.lib()
    return rate_oracle


@pytest.fixture(scope="module")
def proofs(gpu, O, R):
    return RC.Proofs(gpu, O, R)


# ---- sbn_commit_values: the transform plan and the leaf / Merkle kernels of a prover of n rows at rate_bits r -------------------
# (2, 512), (4, 512): leaves that are their own digest; (9, 512): one ragged sponge block; (72, 1024): two column chunks, 64 + 8;
# (8, 2^13): the generic passes at a height with tiles of 16; (16, 2^16), (16, 2^17): the heights whose rate-1 plan is the fused
# middle pass (which must NOT be chosen here) and whose LDE first pass is the zero-aware kernel at r = 2 and 3
SHAPES = [(2, 512), (4, 512), (9, 512), (72, 1024), (8, 1 << 13), (16, 1 << 16), (16, 1 << 17)]


def check_commit(gpu, O, cols, r):
    cap, coeffs, lde = gpu.commit_values(cols, rate_bits=r, cap_height=4, want_coeffs=True, want_lde=True)
    ocap, ocoeffs, olde = O.commit_values(cols, rate_bits=r, cap_height=4, want_coeffs=True, want_lde=True)
    assert lde.shape == (cols.shape[0], cols.shape[1] << r)
    assert np.array_equal(coeffs, ocoeffs), "coefficients differ"
    if not np.array_equal(lde, olde):
        bad = np.argwhere(lde != olde)
        pytest.fail(f"LDE differs at {len(bad)} of {lde.size} points, first (column, row) {tuple(bad[0])}")
    assert np.array_equal(cap, ocap), "Merkle cap differs"


@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_commit_values_matches_the_oracle(gpu, O, shape, r):
    ncols, n = shape
    cols = np.random.default_rng(1000 * r + ncols + n).integers(0, P, size=(ncols, n), dtype=np.uint64)
    check_commit(gpu, O, cols, r)


@pytest.mark.parametrize("r", [2, 3])
def test_commit_values_edge_columns(gpu, O, r):
    """(9, 2^16): columns of all 0, all p - 1 and alternating 0, p - 1 through the zero-aware pass, beside random ones."""
    n = 1 << 16
    cols = np.random.default_rng(77).integers(0, P, size=(9, n), dtype=np.uint64)
    cols[0] = 0
    cols[1] = P - 1
    cols[2, 0::2], cols[2, 1::2] = 0, P - 1
    cols[8, 0::2], cols[8, 1::2] = P - 1, 0
    check_commit(gpu, O, cols, r)


def test_commit_values_range(gpu):
    cols = np.zeros((2, 512), dtype=np.uint64)
    for r in (0, 4):
        with pytest.raises(gpu.SbnError) as e:
            gpu.commit_values(cols, rate_bits=r)
        assert e.value.code == -7


# ---- whole proofs, word for word -------------------------------------------------------------------------------------------
# odd and even lde_log (G1Stark 2^9, 2^10); a wide table; leaves that are their own digest at two heights; no Z columns (two tables)
TABLES = ["g1op9", "g1op10", "modular", "lookup9", "lookup11", "flags", "flagsu64"]


def first_difference(got, want):
    import parity_kit as K
    k = min(len(want), len(got))
    diff = np.nonzero(got[:k] != want[:k])[0]
    return f"{len(got)} / {len(want)} words, first differing word {int(diff[0]) if diff.size else k}, sections at {M.section_words(want)}"


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_proof_words_equal_the_oracles_at_rate_3(gpu, R, proofs, table, case):
    stark, kind, num_io, trace = proofs.table(table)
    bits = trace.shape[1].bit_length() - 1
    cfg = RC.make_config(gpu, case)
    want = proofs(table, case)
    prover = gpu.Prover(stark, cfg, bits)
    try:
        prover.load_trace(trace, RC.NO_PI)
        p1 = prover.prove()
        p2 = prover.prove_host_trace(trace, RC.NO_PI)
        p3 = prover.prove()
    finally:
        prover.close()
    h = M.header(p1.words)
    assert (h[0], h[6]) == (bits, 3) and (h[7], h[9]) == M.fri_shape(bits, case[0], 3)
    if not np.array_equal(p1.words, want):
        pytest.fail(f"{table} {RC.case_id(case)}: device proof differs from the oracle's: {first_difference(p1.words, want)}")
    assert np.array_equal(p2.words, want), "prove_host_trace"
    assert np.array_equal(p3.words, want), "prove after prove_host_trace"
    assert R.verify(kind, num_io, p1.words, 3, case[0] + (case[1],)) == (0, "")
    gpu.verify_stark_proof(stark, p1, cfg)


def test_one_shot_cache_keeps_the_two_rates_apart(gpu, O, proofs, golden):
    """S.prove with the cache on, alternating rate 1 and rate 3 on one table: two misses, two contexts, then hits; the rate-3 words
    are the oracle's, the rate-1 words the committed golden proof's."""
    stark, kind, num_io, trace = proofs.table("g1op9")
    c1, c3 = stark.config(), gpu.StarkConfig.for_rate(3)
    want3 = proofs("g1op9", ((4, 16, 4, 5, 28), True))
    gpu.prove_cache_configure(0)
    before = gpu.prove_cache_stats()
    gpu.prove_cache_configure(1 << 30)
    try:
        got = [gpu.prove(stark, cfg, trace, RC.NO_PI) for cfg in (c1, c3, c1, c3)]
        st = gpu.prove_cache_stats()
        assert (st["misses"] - before["misses"], st["hits"] - before["hits"], st["contexts_resident"]) == (2, 2, 2)
    finally:
        gpu.prove_cache_configure(0)
    g = golden["proof_digests"]["g1op_rows512_seed0"]
    for p in (got[0], got[2]):
        assert len(p.words) == g["proof_words"] and hashlib.sha256(p.to_bytes()).hexdigest() == g["proof_sha256"]
    for p in (got[1], got[3]):
        assert np.array_equal(p.words, want3)


# ---- the Exp tables: device witness -> prove() == the committed digest of the oracle's rate-3 proof ----------------------------
EXP = {"g1exp": ("G1ExpStark", "g1exp_case", 16), "fqexp": ("FqExpStark", "fqexp_case", 16), "fq12expu64": ("Fq12ExpU64Stark", "fq12expu64_case", 11)}


@pytest.mark.parametrize("name", list(EXP))
def test_exp_tables_match_the_committed_rate_3_digests(gpu, golden, request, name):
    cls, fixture, bits = EXP[name]
    g = golden["rate3_digests"]["cases"][name]
    assert tuple(golden["rate3_digests"]["config"]) == (4, 16, 4, 5, 28) and golden["rate3_digests"]["rate_bits"] == 3
    case = request.getfixturevalue(fixture)
    stark, cfg = getattr(gpu, cls)(g["num_io"]), gpu.StarkConfig.for_rate(3)
    prover = gpu.Prover(stark, cfg, bits)
    try:
        pi = prover.generate_trace(case["ios"])
        assert np.array_equal(pi, case["pi"]) and hashlib.sha256(np.asarray(pi, dtype="<u8").tobytes()).hexdigest() == g["public_inputs_sha256"]
        proof = prover.prove()
    finally:
        prover.close()
    assert len(proof.words) == g["proof_words"]
    assert hashlib.sha256(proof.to_bytes()).hexdigest() == g["proof_sha256"]
    bad = gpu.Proof(M.bump(proof.words, M.section_words(proof.words)["opening"]), bits)
    gpu.verify_stark_proof(stark, proof, cfg)
    with pytest.raises(gpu.SbnError) as e:
        gpu.verify_stark_proof(stark, bad, cfg)
    assert e.value.code == -6
    v = gpu.Verifier(stark, cfg, bits, max_batch=2)
    try:
        got = v.verify([proof, bad])
    finally:
        v.close()
    assert got[0] == (0, "") and got[1][0] == -6


# ---- the device verifier ---------------------------------------------------------------------------------------------------
def test_device_verifier_batch_at_rate_3(gpu, proofs):
    """Eight rate-3 proofs of G1Stark 2^9, proofs 2 and 5 changed in different sections: code and reason of every entry are sbn_verify's."""
    stark, kind, num_io, trace = proofs.table("g1op9")
    cfg = gpu.StarkConfig.for_rate(3)
    words = proofs("g1op9", ((4, 16, 4, 5, 28), True))
    sec = M.section_words(words)
    batch = [words] * 8
    batch[2], batch[5] = M.bump(words, sec["fri_step"]), M.bump(words, sec["cap"])
    L = gpu.lib()
    want = []
    for w in batch:
        b = np.asarray(w, dtype="<u8").tobytes()
        rc = L.sbn_verify(C.byref(stark._d), C.byref(cfg._c), b, len(b))
        want.append((rc, L.sbn_last_error().decode() if rc else ""))
    assert [c for c, _ in want] == [0, 0, -6, 0, 0, -6, 0, 0] and want[2][1] != want[5][1]
    v = gpu.Verifier(stark, cfg, 9, max_batch=8)
    try:
        got = v.verify([gpu.Proof(np.asarray(w, dtype=np.uint64), 9) for w in batch])
    finally:
        v.close()
    assert got == want


# ---- the batch prover ------------------------------------------------------------------------------------------------------
def test_batch_prover_at_rate_3(gpu, O, golden, fq12expu64_case):
    stark, cfg = gpu.Fq12ExpU64Stark(16), gpu.StarkConfig.for_rate(3)
    units = np.stack([fq12expu64_case["ios"], O.fq12expu64_inputs(16, 6)[0]])
    bp = gpu.BatchProver(stark, cfg, 11, inflight=2)
    try:
        got = bp.prove_ios(units)
    finally:
        bp.close()
    assert len(got) == 2
    for p in got:
        gpu.verify_stark_proof(stark, p, cfg)
    assert hashlib.sha256(got[0].to_bytes()).hexdigest() == golden["rate3_digests"]["cases"]["fq12expu64"]["proof_sha256"]
    assert not np.array_equal(got[0].words, got[1].words)


# ---- check_trace / explain on a rate-3 context: the trace domain, the prover's scratch -------------------------------------------
@pytest.mark.parametrize("table", ["g1op9", "lookup11"])
def test_trace_check_and_explain_do_not_depend_on_the_rate(gpu, proofs, table):
    stark, kind, num_io, trace = proofs.table(table)
    bits = trace.shape[1].bit_length() - 1
    bad = trace.copy()
    bad[2, 37] = (int(bad[2, 37]) + 1) % P
    rows = [0, 36, 37, 38, trace.shape[1] - 1]
    reports = {}
    for r in (1, 3):
        prover = gpu.Prover(stark, gpu.StarkConfig.for_rate(r), bits)
        try:
            prover.load_trace(trace, RC.NO_PI)
            before = prover.prove()
            valid = (prover.check_trace(5, flags=True), prover.explain_rows(rows, 5), prover.explain_trace(5))
            after = prover.prove()
            prover.load_trace(bad, RC.NO_PI)
            changed = (prover.check_trace(5, flags=True), prover.explain_rows(rows, 5), prover.explain_trace(5))
        finally:
            prover.close()
        assert np.array_equal(before.words, after.words), r
        assert valid[0].ok and valid[2].ok and not changed[0].ok and not changed[2].ok, r
        reports[r] = (valid, changed)
    for k in range(2):
        for a, b in zip(reports[1][k], reports[3][k]):
            assert a == b and str(a) == str(b)
    assert np.array_equal(before.words, proofs(table, ((4, 16, 4, 5, 28), True)))


# ---- the split prover stays at rate 1 --------------------------------------------------------------------------------------
def test_split_prover_refuses_rate_3_with_one_rank(gpu):
    from starky_bn254_amd import split
    L = gpu.lib()
    split._bind(L)
    stark, cfg = gpu.G1ExpStark(128), gpu.StarkConfig.for_rate(3)
    comm = split._Comm()
    comm.struct_size, comm.rank, comm.world = C.sizeof(split._Comm), 0, 1
    h = C.c_void_p()
    assert L.sbn_split_prover_create(C.byref(stark._d), C.byref(cfg._c), 16, C.byref(comm), C.byref(h)) == -7
    assert not h.value
    with pytest.raises(gpu.SbnError) as e:
        split.exchange_bytes(stark, cfg, 16, 1)
    assert e.value.code == -7
