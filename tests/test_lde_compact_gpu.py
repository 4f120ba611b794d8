"""Compact LDE storage on the device (run on the MI355X box with `-m gpu`): the rows a query opens, evaluated from the coefficients
(sbn_lde_rows) against the oracle's LDE at rate_bits 2 and 3; whole proofs of compact contexts word for word against the CPU oracle
at rate 3 under every config row of tests/rate_cases.py, over the heights 2^12 .. 2^15, and for the Exp tables against the committed
digests of tests/golden/rate3_digests.json; device memory against sbn_prover_memory_plan; the batch prover; trace check and explain
on a compact context.  Shapes are the smallest at which each path differs: see the parameter lists.

Mutations tried against this file, once each on the MI355X (library rebuilt with the one change; 55 cases):
  (a) lde_keep_rows_kernel reading row (j << (r-1)) + 1: 35 cases fail, 20 pass.  Failing: every whole-proof case of a wide table
      (25 of test_compact_proof_words_.., all but the five lookup9 ones), the four flag heights, the four Exp tables, the batch
      prover and the trace-check case; first differing stage quotient_polys_cap wherever a stage is named.  Passing: lookup9 (stays
      whole), test_lde_rows_* and the memory and create_with cases, which do not run the kernel.
  (b) query_rows_table_kernel taking rho = idx[q] without the bit reversal: 45 cases fail, 10 pass.  Failing: all ten test_lde_rows
      cases ("words differ"), and the 35 cases of (a) with first differing stage query_rounds.  Passing: lookup9, test_lde_rows_range,
      the memory and create_with cases.
  (c) the ring wait removed (slot_free always null): 21 cases fail, 34 pass; a race, and it is seen.  Failing, first differing stage
      trace_cap: the 15 whole-proof cases of g1op9, modular and fq12mul (36 + 20, 13 + .., 152 + 84 chunks on one stream), the four Exp
      tables, the batch prover and the trace-check case.  Passing: flags, flagsu64 and the flag heights (a single chunk or two: no
      slot is written twice) and lookup9."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import config_matrix as M
import lde_compact_cases as LC
import rate_cases as RC
import test_rate_gpu as TR

pytestmark = pytest.mark.gpu
P = LC.P


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


@pytest.fixture(scope="module")
def heights(gpu, O, R):
    return TR.Heights(gpu, O, R)


# ---- sbn_lde_rows: values -> coefficients -> the rows at the opened points ---------------------------------------------------------
# (9, 512): a ragged tile of columns (4 + 4 + 1) at the smallest height; (72, 1024): two chunks of the inverse transform; (8, 2^13):
# the generic transform passes; (16, 2^16): the height of the zero-aware LDE pass in the oracle's reference and of 2^19 leaves
SHAPES = [(9, 512), (72, 1024), (8, 1 << 13), (16, 1 << 16)]


class Ldes:
    """(columns, the oracle's LDE in natural row order) of a shape and rate, made once per session and never written to."""

    def __init__(self, O):
        self.O, self.cache = O, {}

    def __call__(self, ncols, n, r):
        if (ncols, n, r) not in self.cache:
            cols = np.random.default_rng(2000 * r + ncols + n).integers(0, P, size=(ncols, n), dtype=np.uint64)
            lde = self.O.commit_values(cols, rate_bits=r, cap_height=4, want_coeffs=False, want_lde=True)[2]
            cols.setflags(write=False)
            lde.setflags(write=False)
            self.cache[(ncols, n, r)] = (cols, lde)
        return self.cache[(ncols, n, r)]


@pytest.fixture(scope="module")
def ldes(O):
    return Ldes(O)


def leaf_sets(m, seed):
    """The corners with a duplicate; 65 indices (one more than a slice of the point table holds); 200 (four slices, the last short)."""
    rng = np.random.default_rng(seed)
    return {"corners": [0, 1, m - 1, m // 2, 1, m - 1], "65": [int(x) for x in rng.integers(0, m, size=65)], "200": [int(x) for x in rng.integers(0, m, size=200)]}


def check_rows(gpu, cols, lde, r, leaves, what):
    lde_log = lde.shape[1].bit_length() - 1
    got = gpu.lde_rows(cols, r, leaves)
    want = np.stack([lde[:, LC.bitrev(i, lde_log)] for i in leaves])
    assert got.shape == want.shape == (len(leaves), cols.shape[0])
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        pytest.fail(f"{what}: {len(bad)} of {got.size} words differ, first (query, column) {tuple(bad[0])}, leaf {leaves[bad[0][0]]}")


@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lde_rows_match_the_oracles_lde(gpu, ldes, shape, r):
    ncols, n = shape
    cols, lde = ldes(ncols, n, r)
    for name, leaves in leaf_sets(n << r, 31 * r + ncols).items():
        check_rows(gpu, cols, lde, r, leaves, f"{ncols}x{n} r={r} {name}")


@pytest.mark.parametrize("r", [2, 3])
def test_lde_rows_edge_columns(gpu, O, r):
    """(9, 2^16): columns of all 0, all p - 1, alternating 0, p - 1, and c X^(n-1) (one non-zero coefficient, the last) beside random ones."""
    n = 1 << 16
    cols = np.random.default_rng(77).integers(0, P, size=(9, n), dtype=np.uint64)
    cols[0] = 0
    cols[1] = P - 1
    cols[2, 0::2], cols[2, 1::2] = 0, P - 1
    cols[3] = LC.column_of_top_coefficient(n, P - 1)
    cols[8] = LC.column_of_top_coefficient(n, 3)
    coeffs, lde = O.commit_values(cols, rate_bits=r, cap_height=4, want_coeffs=True, want_lde=True)[1:]
    assert int(coeffs[3, n - 1]) == P - 1 and not coeffs[3, :n - 1].any() and int(coeffs[8, n - 1]) == 3 and not coeffs[8, :n - 1].any()
    for name, leaves in leaf_sets(n << r, 5 + r).items():
        check_rows(gpu, cols, lde, r, leaves, f"edge columns r={r} {name}")


def test_lde_rows_range(gpu):
    cols = np.zeros((2, 512), dtype=np.uint64)
    for r in (0, 4):
        with pytest.raises(gpu.SbnError) as e:
            gpu.lde_rows(cols, r, [0])
        assert e.value.code == -7
    with pytest.raises(gpu.SbnError) as e:
        gpu.lde_rows(cols, 3, [0, 4096])
    assert e.value.code == -1
    with pytest.raises(gpu.SbnError) as e:
        gpu.lde_rows(np.zeros((2, 256), dtype=np.uint64), 3, [0])
    assert e.value.code == -7


# ---- whole proofs of compact contexts, word for word ---------------------------------------------------------------------------
# g1op9: 2,283 + 1,264 columns = 36 + 20 chunks with ragged tails, every ring slot reused many times; modular and fq12mul: other
# widths (fq12mul the widest, its own quotient kernel); flags, flagsu64: no Z matrix; lookup9: 4 + 2 columns, the table that stays
# whole (a compact context of it is a full one)
TABLES = ["g1op9", "modular", "flags", "flagsu64", "lookup9", "fq12mul"]


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_compact_proof_words_equal_the_oracles_at_rate_3(gpu, O, R, proofs, table, case):
    stark, kind, num_io, trace = proofs.table(table)
    bits = trace.shape[1].bit_length() - 1
    cfg = RC.make_config(gpu, case)
    want = proofs(table, case)
    prover = gpu.Prover(stark, cfg, bits, lde="compact")
    try:
        assert prover.describe()["lde"] == "compact"
        prover.load_trace(trace, RC.NO_PI)
        p1 = prover.prove()
        p2 = prover.prove_host_trace(trace, RC.NO_PI)
        p3 = prover.prove()
    finally:
        prover.close()
    if not np.array_equal(p1.words, want):
        pytest.fail(f"{table} {RC.case_id(case)}: compact proof differs from the oracle's: {TR.first_difference(O, p1.words, want)}")
    if not np.array_equal(p2.words, want):
        pytest.fail(f"{table} {RC.case_id(case)}: prove_host_trace: {TR.first_difference(O, p2.words, want)}")
    if not np.array_equal(p3.words, want):
        pytest.fail(f"{table} {RC.case_id(case)}: prove after prove_host_trace: {TR.first_difference(O, p3.words, want)}")
    assert R.verify(kind, num_io, p1.words, 3, case[0] + (case[1],)) == (0, "")
    gpu.verify_stark_proof(stark, p1, cfg)


@pytest.mark.parametrize("num_io", TR.FLAG_IOS)
def test_compact_flag_heights_equal_the_oracles_at_rate_3(gpu, O, R, heights, num_io):
    """FlagStark(8 .. 64), 2^12 .. 2^15 rows: the generic transform passes and the upper-zero branch write the ring slots."""
    stark, kind, num_io, trace, want = heights("flags", num_io)
    bits = trace.shape[1].bit_length() - 1
    cfg = RC.make_config(gpu, TR.ROW3)
    prover = gpu.Prover(stark, cfg, bits, lde="compact")
    try:
        prover.load_trace(trace, RC.NO_PI)
        p1 = prover.prove()
        p2 = prover.prove()
    finally:
        prover.close()
    if not np.array_equal(p1.words, want):
        pytest.fail(f"FlagStark({num_io}): compact proof differs from the oracle's: {TR.first_difference(O, p1.words, want)}")
    assert np.array_equal(p2.words, want), "second prove()"
    assert R.verify(kind, num_io, p1.words, 3, TR.ROW3[0] + (TR.ROW3[1],)) == (0, "")
    gpu.verify_stark_proof(stark, p1, cfg)


# ---- the Exp tables: device witness into the smaller scratch, then prove() three times == the committed digest ------------------------
# g1exp: 2^16 rows, the zero-aware pass on two transform streams, 35 + 16 chunks; fq12expu64: 2^11; fq12exp: 2^13; g2exp: 2^16
EXP = ["g1exp", "fq12expu64", "fq12exp", "g2exp"]


@pytest.mark.parametrize("name", EXP)
def test_compact_exp_tables_match_the_committed_rate_3_digests(gpu, golden, request, name):
    cls, fixture, bits = TR.EXP[name]
    g = golden["rate3_digests"]["cases"][name]
    assert tuple(golden["rate3_digests"]["config"]) == (4, 16, 4, 5, 28) and golden["rate3_digests"]["rate_bits"] == 3
    case = request.getfixturevalue(fixture)
    stark, cfg = getattr(gpu, cls)(g["num_io"]), gpu.StarkConfig.for_rate(3)
    prover = gpu.Prover(stark, cfg, bits, lde="compact")
    try:
        pi = prover.generate_trace(case["ios"])
        assert np.array_equal(pi, case["pi"])
        got = [prover.prove(), prover.prove(), prover.prove()]
        if name == "g1exp":
            got += [prover.prove_host_trace(case["trace"], case["pi"]), prover.prove()]
    finally:
        prover.close()
    for k, p in enumerate(got):
        assert len(p.words) == g["proof_words"], k
        assert hashlib.sha256(p.to_bytes()).hexdigest() == g["proof_sha256"], ("prove 1", "prove 2", "prove 3", "prove_host_trace", "prove after prove_host_trace")[k]
    gpu.verify_stark_proof(stark, got[0], cfg)


# ---- device memory: what a context allocates is what the plan says ---------------------------------------------------------------------
@pytest.mark.parametrize("table", ["g1op9", "g1exp", "fq12expu64"])
def test_dev_bytes_after_creation_equal_the_memory_plan(gpu, golden, table):
    if table == "g1op9":
        stark, bits = gpu.G1Stark(), 9
    else:
        stark, bits = getattr(gpu, TR.EXP[table][0])(golden["rate3_digests"]["cases"][table]["num_io"]), TR.EXP[table][2]
    cfg = gpu.StarkConfig.for_rate(3)
    seen = {}
    for mode in ("full", "compact"):
        prover = gpu.Prover(stark, cfg, bits, lde=mode)
        try:
            d = prover.describe()
        finally:
            prover.close()
        assert d["lde"] == mode
        assert int(d["dev_bytes"]) == gpu.prover_memory_plan(stark, cfg, bits, lde=mode), (table, mode)
        assert (int(d["lde_ring"]), int(d["lde_ring_bytes"])) == ((LC.RING_DEPTH, LC.ring_bytes(bits, 3)) if mode == "compact" else (0, 0))
        seen[mode] = int(d["dev_bytes"])
    assert seen["full"] - seen["compact"] == LC.expected_saving(stark, cfg, bits)


# ---- the batch prover ----------------------------------------------------------------------------------------------------------
def batch_digests(gpu, golden, ios, units, inflight):
    stark, cfg = gpu.Fq12ExpU64Stark(16), gpu.StarkConfig.for_rate(3)
    bp = gpu.BatchProver(stark, cfg, 11, inflight=inflight, lde="compact")
    try:
        got = bp.prove_ios(np.stack([ios] * units))
    finally:
        bp.close()
    want = golden["rate3_digests"]["cases"]["fq12expu64"]["proof_sha256"]
    return [hashlib.sha256(p.to_bytes()).hexdigest() == want for p in got]


def test_compact_batch_prover_matches_the_committed_digest_for_every_unit(gpu, golden, fq12expu64_case):
    """Three units on three contexts in flight: one unit per context, all three proving at once.  More units than contexts at
    inflight=3 run into a defect that is older than the compact storage and not fixed by it (include/sbn.h at
    sbn_prover_create_with): measured on the MI355X, 15 units of this table at rate 3 give 6 to 7 proofs that differ from the
    single-context proof from the trace cap on -- with the library of the commit before this one and full storage, and with this
    tree in both modes; 1 of 15 at rate 1; units 0 .. 3 never; inflight 1 and 2 never.  The case below holds what does hold."""
    assert batch_digests(gpu, golden, fq12expu64_case["ios"], 3, 3) == [True] * 3


@pytest.mark.parametrize("inflight,units", [(1, 4), (2, 3)])
def test_compact_batch_prover_with_more_units_than_contexts(gpu, golden, fq12expu64_case, inflight, units):
    """A context proves a second unit (witness into the smaller scratch again, then the ring again) with one and two contexts in flight."""
    assert batch_digests(gpu, golden, fq12expu64_case["ios"], units, inflight) == [True] * units


# ---- check_trace / explain read the trace, Z values and scratch only ------------------------------------------------------------------
def test_trace_check_and_explain_on_a_compact_context(gpu, proofs):
    stark, kind, num_io, trace = proofs.table("g1op9")
    bad = trace.copy()
    bad[2, 37] = (int(bad[2, 37]) + 1) % P
    rows = [0, 36, 37, 38, trace.shape[1] - 1]
    cfg = gpu.StarkConfig.for_rate(3)
    reports, words = {}, {}
    for mode in ("full", "compact"):
        prover = gpu.Prover(stark, cfg, 9, lde=mode)
        try:
            prover.load_trace(trace, RC.NO_PI)
            before = prover.prove()
            valid = (prover.check_trace(5, flags=True), prover.explain_rows(rows, 5), prover.explain_trace(5))
            after = prover.prove()
            prover.load_trace(bad, RC.NO_PI)
            changed = (prover.check_trace(5, flags=True), prover.explain_rows(rows, 5), prover.explain_trace(5))
            prover.load_trace(trace, RC.NO_PI)
            again = prover.prove()
        finally:
            prover.close()
        assert np.array_equal(before.words, after.words) and np.array_equal(before.words, again.words), mode
        assert valid[0].ok and valid[2].ok and not changed[0].ok and not changed[2].ok, mode
        reports[mode], words[mode] = (valid, changed), before.words
    for k in range(2):
        for a, b in zip(reports["full"][k], reports["compact"][k]):
            assert a == b and str(a) == str(b)
    assert np.array_equal(words["full"], words["compact"])
    assert np.array_equal(words["compact"], proofs("g1op9", ((4, 16, 4, 5, 28), True)))


# ---- sbn_prover_create_with(full) is sbn_prover_create ---------------------------------------------------------------------------
def test_full_context_through_create_with_is_the_old_one(gpu, proofs):
    stark, kind, num_io, trace = proofs.table("g1op9")
    want = proofs("g1op9", ((4, 16, 4, 5, 28), True))
    cfg = gpu.StarkConfig.for_rate(3)
    provers = [gpu.Prover(stark, cfg, 9)]   # sbn_prover_create itself: what Prover calls for a full context
    for opt in (LC.options(lde_storage=0), None):   # sbn_prover_create_with: SBN_LDE_FULL, then no options at all
        p = gpu.Prover.__new__(gpu.Prover)
        p.stark, p.config, p.degree_bits, p._h = stark, cfg, 9, C.c_void_p()
        assert gpu.lib().sbn_prover_create_with(C.byref(stark._d), C.byref(cfg._c), 9, C.byref(opt) if opt is not None else None, C.byref(p._h)) == 0
        provers.append(p)
    try:
        described = []
        for p in provers:
            p.load_trace(trace, RC.NO_PI)
            assert np.array_equal(p.prove().words, want)
            described.append(p.describe())
    finally:
        for p in provers:
            p.close()
    assert described[0] == described[1] == described[2] and described[0]["lde"] == "full"
