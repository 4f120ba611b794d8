"""rate_bits 3 on the device (run on the MI355X box with `-m gpu`): the transforms and the leaf / Merkle kernels at rate_bits 2 and 3
through sbn_commit_values, then whole proofs word for word against the CPU oracle at that rate (tests/rate_oracle.py), the Exp
tables against committed digests of the oracle's proofs (tests/golden/rate3_digests.json), the device verifier, the batch prover,
the trace check and explain on a rate-3 context, and the refusal of the split prover.  Shapes are the smallest at which each
kernel path differs: see the parameter lists.  Rate 3 runs at every accepted height: 2^9 .. 2^11 under every config row, 2^12 ..
2^15 and 2^17 word for word, 2^16 with the Exp tables and 2^18 .. 2^20 against committed digests; PLANS holds the transform plans
that ntt_columns picks at rates 2 and 3 between those heights.

Mutations tried against this file, once each (library rebuilt with the one change, values only; 93 cases):
  (a) ntt_fast_pass_kernel's upper_zero branch storing `a` for `nw::mul(a, w)`: 9 cases fail -- PLANS 16x16384-r3, 16x32768-r3 and
      16x32768-r2, both cases of test_commit_values_edge_columns_through_the_upper_zero_branch, test_lookup_heights_.. [14] and [15],
      test_flag_heights_.. [32] and [64]; the 84 others pass, among them every case this file had before PLANS was added;
  (b) ntt_columns taking the forward twiddle table for an inverse transform of 2^18 points (`a.tw = (inverse && log_n != 18) ? ..`):
      4 cases fail -- PLANS 4x262144-r2 and 4x262144-r3 (coefficients), test_lookup_largest_heights_.. [18] (first differing stage
      trace_cap) and test_lookup_heights_.. [17] (quotient_polys_cap: the quotient of a 2^17-row table is interpolated over 2^18
      points); the 89 others pass, among them every case this file had before.
  Setting lde_za_log for degree_bits 15 as well was not run: ntt_lde_first_pass_kernel and lde_za_tables are written for any
  n = 256 S, so by the code that plan is slower, not wrong, and no parity test can tell it from the right one."""
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


# ---- the transform plans that no whole height above reaches (ntt_columns / ntt_plan in csrc/prover.hip; LDE = n << r, cut 2^a x 2^b) ----
PLANS = [
    # LDE 2^17 = 512 x 256, neither fused (rate 1 only) nor zero-aware (2^16 / 2^17 rows only): pass A is ntt_fast_pass_kernel<1> in
    # its upper_zero branch with 64 of the 512 rows non-zero, pass B ntt_fast_pass_kernel<0>; inverse 2^14 = 128 x 128, generic passes
    (16, 1 << 14, 3),
    # LDE 2^18 = 512 x 512: fast<1> on both passes, pass A in its upper_zero branch (64 of 512 rows); inverse 2^15 = fast<0> + generic
    (16, 1 << 15, 3),
    # LDE 2^17 as above with 128 of the 512 rows non-zero
    (16, 1 << 15, 2),
    # LDE 2^14 = 128 x 128: ntt_pass_kernel (generic) on both passes, 16 of 128 rows non-zero; nine columns = one ragged sponge block
    (9, 1 << 11, 3),
    # LDE 2^15 = 256 x 128: pass A is fast<0> (not the generic pass: 256-point rows with tiles of 16), pass B generic.  (8, 2^13) at
    # r = 2 above runs the same two kernels; this is the cut with 32 instead of 64 of the 256 rows non-zero, the inverse 2^12 = 64 x 64
    # and the ragged sponge block, and the height 2^12 of the whole proofs below, so it stays
    (9, 1 << 12, 3),
    # inverse 2^18 = 512 x 512: fast<1> on both passes, neither in the upper_zero branch, the 1 / n scale in pass B (at rate 1
    # ntt_fused512 replaces that pass B); LDE 2^20 = 1024 x 1024, generic passes with tiles of 4 (no d_shift_odd, so no split pass A)
    (4, 1 << 18, 2),
    # the same inverse; LDE 2^21 = 2048 x 1024, generic passes with 2^11-point rows (tiles of 2)
    (4, 1 << 18, 3),
    # LDE 2^22 = 2048 x 2048, generic; inverse 2^19 = 1024 (generic) x 512 (fast<1> as pass B); leaves that are their own digest
    (2, 1 << 19, 3),
    # LDE 2^23 = 4096 x 2048, the largest accepted: generic passes with 2^12-point rows (tiles of 1, 64 KiB of LDS); 23-bit leaf indices
    (2, 1 << 20, 3),
]


def plan_columns(ncols, n, r):
    cols = np.random.default_rng(1000 * r + ncols + n).integers(0, P, size=(ncols, n), dtype=np.uint64)
    cols[0, :4] = [0, P - 1, 1, 0xFFFFFFFF00000000]
    return cols


@pytest.mark.parametrize("plan", PLANS, ids=lambda s: f"{s[0]}x{s[1]}-r{s[2]}")
def test_commit_values_at_the_plans_between_the_heights(gpu, O, plan):
    ncols, n, r = plan
    check_commit(gpu, O, plan_columns(ncols, n, r), r)


@pytest.mark.parametrize("n", [1 << 14, 1 << 15])
def test_commit_values_edge_columns_through_the_upper_zero_branch(gpu, O, n):
    """(16, 2^14) and (16, 2^15) at r = 3: columns of all 0, all p - 1 and alternating through ntt_fast_pass_kernel<1>'s upper_zero
    branch (LDEs of 2^17 and 2^18 points), beside random ones."""
    cols = plan_columns(16, n, 3)
    cols[0] = 0
    cols[1] = P - 1
    cols[2, 0::2], cols[2, 1::2] = 0, P - 1
    cols[15, 0::2], cols[15, 1::2] = P - 1, 0
    check_commit(gpu, O, cols, 3)


def test_commit_values_range(gpu):
    cols = np.zeros((2, 512), dtype=np.uint64)
    for r in (0, 4):
        with pytest.raises(gpu.SbnError) as e:
            gpu.commit_values(cols, rate_bits=r)
        assert e.value.code == -7


# ---- whole proofs, word for word -------------------------------------------------------------------------------------------
# odd and even lde_log (G1Stark 2^9, 2^10); a wide table; leaves that are their own digest at two heights; no Z columns (two tables);
# Fq12Stark, the widest single-operation table, whose AIR instantiates its own quotient kernel
TABLES = ["g1op9", "g1op10", "modular", "lookup9", "lookup11", "flags", "flagsu64", "fq12mul"]


def first_difference(O, got, want):
    """The first differing word and, through the parity kit, the first stage of prove() that differs."""
    import parity_kit as K
    k = min(len(want), len(got))
    diff = np.nonzero(got[:k] != want[:k])[0]
    stage = K.first_difference(K.stage_digests(got, O.poseidon_permute), K.stage_digests(want, O.poseidon_permute)) if len(got) == len(want) else None
    return (f"{len(got)} / {len(want)} words, first differing word {int(diff[0]) if diff.size else k}, sections at {M.section_words(want)}, "
            f"first differing stage {stage}")


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_proof_words_equal_the_oracles_at_rate_3(gpu, O, R, proofs, table, case):
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
        pytest.fail(f"{table} {RC.case_id(case)}: device proof differs from the oracle's: {first_difference(O, p1.words, want)}")
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


# ---- whole proofs over the heights, under for_rate(3)'s row with the times-X step ------------------------------------------------------
ROW3 = ((4, 16, 4, 5, 28), True)
# LookupStark (4 columns and 2 Zs: every leaf its own digest), seed 200 + bits.  2^12, 2^13: LDEs of 2^15 and 2^16 points on one
# stream; 2^14, 2^15: LDEs of 2^17 and 2^18 points through ntt_fast_pass_kernel<1>'s upper_zero branch; 2^17: the zero-aware first
# pass of a 2^20-point LDE (2^16 rows has the Exp tables below)
LOOKUP_BITS = [12, 13, 14, 15, 17]
# FlagStark(num_io): 512 * num_io rows = 2^12 .. 2^15, 17 + 4 * num_io columns in hashed leaves, no Z tree; seed 100 + num_io
FLAG_IOS = [8, 16, 32, 64]


class Heights:
    """(stark, oracle kind, num_io, trace, the oracle's rate-3 proof under ROW3) of a table, made once per session."""

    def __init__(self, S, O, R):
        self.S, self.O, self.R, self.cache = S, O, R, {}

    def __call__(self, table, size):
        if (table, size) not in self.cache:
            S, O = self.S, self.O
            if table == "lookup":
                stark, kind, num_io = S.LookupStark(), O.AIR_LOOKUP, 0
                trace = stark.generate_trace(*O.lookup_inputs(1 << size, 200 + size))
            else:
                stark, kind, num_io = S.FlagStark(size), O.AIR_FLAGS, size
                trace = stark.generate_trace(O.flags_inputs(size, 100 + size)[0])
            want = self.R.prove(kind, num_io, trace, RC.NO_PI, 3, ROW3[0] + (ROW3[1],))[0]
            self.cache[(table, size)] = (stark, kind, num_io, trace, want)
        return self.cache[(table, size)]


@pytest.fixture(scope="module")
def heights(gpu, O, R):
    return Heights(gpu, O, R)


def check_height(gpu, O, R, heights, table, size):
    stark, kind, num_io, trace, want = heights(table, size)
    bits = trace.shape[1].bit_length() - 1
    cfg = RC.make_config(gpu, ROW3)
    prover = gpu.Prover(stark, cfg, bits)
    try:
        prover.load_trace(trace, RC.NO_PI)
        p1 = prover.prove()
        p2 = prover.prove()
    finally:
        prover.close()
    h = M.header(p1.words)
    assert (h[0], h[5], h[6], h[8], h[10]) == (bits, 4, 3, 4, 28) and (h[7], h[9]) == M.fri_shape(bits, ROW3[0], 3)
    if not np.array_equal(p1.words, want):
        pytest.fail(f"{table} {size}: device proof differs from the oracle's: {first_difference(O, p1.words, want)}")
    assert np.array_equal(p2.words, p1.words), "second prove()"
    assert R.verify(kind, num_io, p1.words, 3, ROW3[0] + (ROW3[1],)) == (0, "")
    gpu.verify_stark_proof(stark, p1, cfg)


@pytest.mark.parametrize("bits", LOOKUP_BITS)
def test_lookup_heights_equal_the_oracles_at_rate_3(gpu, O, R, heights, bits):
    check_height(gpu, O, R, heights, "lookup", bits)


@pytest.mark.parametrize("num_io", FLAG_IOS)
def test_flag_heights_equal_the_oracles_at_rate_3(gpu, O, R, heights, num_io):
    check_height(gpu, O, R, heights, "flags", num_io)


# ---- the Exp tables: device witness -> prove() == the committed digest of the oracle's rate-3 proof ----------------------------
# G2ExpStark and Fq12ExpStark (the widest table, a translation unit of its own) instantiate their own quotient kernels
EXP = {"g1exp": ("G1ExpStark", "g1exp_case", 16), "fqexp": ("FqExpStark", "fqexp_case", 16), "fq12expu64": ("Fq12ExpU64Stark", "fq12expu64_case", 11),
       "g2exp": ("G2ExpStark", "g2exp_case", 16), "fq12exp": ("Fq12ExpStark", "fq12exp_case", 13)}


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
        # the streamed upload at a height whose commitment runs the zero-aware pass on two streams, then the resident trace again
        streamed = [prover.prove_host_trace(case["trace"], case["pi"]), prover.prove()] if name == "g1exp" else []
    finally:
        prover.close()
    assert len(proof.words) == g["proof_words"]
    assert hashlib.sha256(proof.to_bytes()).hexdigest() == g["proof_sha256"]
    for k, p in enumerate(streamed):
        assert hashlib.sha256(p.to_bytes()).hexdigest() == g["proof_sha256"], ("prove_host_trace", "prove after prove_host_trace")[k]
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


def check_verifier_ends(gpu, stark, cfg, bits, words):
    """The proof and copies bumped in the last query's first Merkle path, its first FRI leaf and the proof-of-work witness: every
    (code, reason) of the device verifier is sbn_verify's (test_verifier_gpu.check_batch asserts that)."""
    from test_verifier_gpu import check_batch, query_words
    where = query_words(words)
    names = ["good", "initial0_sibling", "fri0_leaf_last", "pow_witness"]
    want = check_batch(gpu, stark, cfg, bits, names, [words] + [M.bump(words, where[n]) for n in names[1:]])
    assert want[0] == (0, "") and [c for c, _ in want[1:]] == [-6, -6, -6], want
    assert want[1][1].startswith("invalid Merkle proof"), want[1]


def test_device_verifier_at_the_short_end_of_the_lde_range(gpu, heights):
    """LookupStark at 2^14 rows, rate 3 (the oracle's proof): Merkle paths of 13 siblings over 2^17 leaves."""
    stark, kind, num_io, trace, words = heights("lookup", 14)
    check_verifier_ends(gpu, stark, RC.make_config(gpu, ROW3), 14, words)


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


# ---- the slow cases, kept last: LookupStark above 2^17 rows against committed digests of the oracle's proofs -------------------------
class BigLookups:
    """The device's rate-3 proof of LookupStark at 2^bits rows (inputs O.lookup_inputs(1 << bits, 200 + bits)), made once per session."""

    def __init__(self, S, O):
        self.S, self.O, self.cache = S, O, {}

    def __call__(self, bits):
        if bits not in self.cache:
            stark, cfg = self.S.LookupStark(), self.S.StarkConfig.for_rate(3)
            trace = stark.generate_trace(*self.O.lookup_inputs(1 << bits, 200 + bits))
            prover = self.S.Prover(stark, cfg, bits)
            try:
                prover.load_trace(trace, RC.NO_PI)
                self.cache[bits] = (stark, cfg, trace, prover.prove())
            finally:
                prover.close()
        return self.cache[bits]


@pytest.fixture(scope="module")
def big_lookups(gpu, O):
    return BigLookups(gpu, O)


def check_lookup_digest(gpu, O, R, golden, big_lookups, bits):
    g = golden["rate3_digests"]["cases"][f"lookup{bits}"]
    assert (g["degree_bits"], g["seed"]) == (bits, 200 + bits) and tuple(golden["rate3_digests"]["config"]) == ROW3[0]
    stark, cfg, trace, proof = big_lookups(bits)
    h = M.header(proof.words)
    assert (h[0], h[5], h[6], h[8], h[10]) == (bits, 4, 3, 4, 28) and (h[7], h[9]) == M.fri_shape(bits, ROW3[0], 3)
    if (len(proof.words), hashlib.sha256(proof.to_bytes()).hexdigest()) != (g["proof_words"], g["proof_sha256"]):
        want = R.prove(O.AIR_LOOKUP, 0, trace, RC.NO_PI, 3, ROW3[0] + (ROW3[1],))[0]   # (the slow path: only to name the word)
        pytest.fail(f"LookupStark 2^{bits}: device proof differs from the oracle's: {first_difference(O, proof.words, want)}")
    gpu.verify_stark_proof(stark, proof, cfg)
    return stark, cfg, proof


@pytest.mark.parametrize("bits", [18, 19, 20])
def test_lookup_largest_heights_match_the_committed_rate_3_digests(gpu, O, R, golden, big_lookups, bits):
    """2^18: the unfused inverse transform of 2^18 points (fast<1> on both passes) and a 2^21-point LDE; 2^19, 2^20: LDEs of 2^22 and
    2^23 points (generic passes with 2^11- and 2^12-point rows, two transform streams), 23-bit indices through the leaf, Merkle,
    gather and query kernels.  The time is the host's trace generation and the device."""
    check_lookup_digest(gpu, O, R, golden, big_lookups, bits)


def test_device_verifier_at_the_long_end_of_the_lde_range(gpu, O, R, golden, big_lookups):
    """LookupStark at 2^20 rows, rate 3, the device prover's proof after its digest check: Merkle paths of 19 siblings over 2^23 leaves."""
    stark, cfg, proof = check_lookup_digest(gpu, O, R, golden, big_lookups, 20)
    check_verifier_ends(gpu, stark, cfg, 20, proof.words)
