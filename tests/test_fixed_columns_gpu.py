"""The shape-constant trace columns on the device (include/sbn.h sbn_fixed_columns_range; csrc/prover.hip stage_trace_commit, and
csrc/trace_load.hip fixed_columns_check for the comparison behind a load): a prover transforms them in its first proof of a trace that holds the generators' words there and leaves them alone afterwards.
Every proof stays the same words: against the committed oracle digests, against fresh provers, against SBN_FIXED_COLUMNS=0, at
every chunking; describe()["fixed_columns_skipped"] shows that the short path ran where it should and only there."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GL_P = 0xFFFFFFFF00000001

# table class, num_io, degree_bits, conftest case, key of tests/golden/proof_digests.json (the kit's committed seeds), rows per instance, periodic pulse
CASES = {
    "fq12expu64": ("Fq12ExpU64Stark", 16, 11, "fq12expu64_case", "fq12expu64_io16_seed5", 128, False),   # generic pass
    "fq12exp": ("Fq12ExpStark", 16, 13, "fq12exp_case", "fq12exp_io16_seed3", 512, True),
    "g1exp": ("G1ExpStark", 128, 16, "g1exp_case", "g1exp_io128_seed1", 512, True),                       # fused middle pass
    "fqexp": ("FqExpStark", 128, 16, "fqexp_case", "fqexp_io128_seed4", 512, True),                       # 960 columns: the table that admits 8-column chunks
}


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    return S


def _case(gpu, request, table):
    cls, num_io, bits, case, key, rpb, periodic = CASES[table]
    stark = getattr(gpu, cls)(num_io)
    c = request.getfixturevalue(case)
    return stark, bits, c, key


def _digest(proof):
    return hashlib.sha256(proof.to_bytes()).hexdigest()


def _skipped(prover):
    return int(prover.describe()["fixed_columns_skipped"])


def _io_columns(gpu, table):
    """First column of the block, column of the io-pulse counter."""
    cls, num_io, bits, case, key, rpb, periodic = CASES[table]
    f0, f1 = gpu.api.fixed_columns_range(getattr(gpu, cls)(num_io))
    return f0, f1, f0 + (2 if periodic else 0)


def _pulse_pos(q, rpb):
    return (q // 2) * rpb + (rpb - 1 if q % 2 else 0)


@pytest.mark.parametrize("table", ["fq12expu64", "fq12exp", "g1exp"])
def test_three_proofs_one_prover_same_words_as_the_oracle(table, gpu, golden, request):
    """The first proof fills the transforms of the block, the second and third leave all of it untransformed: three times the
    oracle's proof."""
    stark, bits, c, key = _case(gpu, request, table)
    f0, f1 = gpu.api.fixed_columns_range(stark)
    prover = gpu.Prover(stark, stark.config(), bits)
    try:
        d = prover.describe()
        assert d["fixed_columns"] == "1" and d["fixed_columns_range"] == f"{f0}:{f1}" and d["fixed_columns_skipped"] == "0"
        if table == "g1exp":   # the chunk plan of the flagship: chunks 7..13 lie wholly inside the block and are not launched at all
            ch = int(d["ntt_chunk"])
            assert ch == 64 and [k for k in range(-(-stark.num_columns // ch)) if k * ch >= f0 and min((k + 1) * ch, stark.num_columns) <= f1] == list(range(7, 14))
        prover.load_trace(c["trace"], c["pi"])
        proofs, skipped = [], []
        for _ in range(3):
            proofs.append(prover.prove())
            skipped.append(_skipped(prover))
    finally:
        prover.close()
    want = golden["proof_digests"][key]["proof_sha256"]
    assert [_digest(p) for p in proofs] == [want] * 3
    assert np.array_equal(proofs[0].words, proofs[1].words) and np.array_equal(proofs[1].words, proofs[2].words)
    assert skipped == [0, f1 - f0, f1 - f0]


def test_next_trace_on_the_same_prover_loaded(gpu, O, request):
    """load A, prove, load B (other instances), prove: the second proof reuses the block's transforms of the first and equals
    the proof of a fresh prover."""
    stark, bits, c, key = _case(gpu, request, "fq12expu64")
    ios_b, _ = O.fq12expu64_inputs(16, 105)
    trace_b, pi_b = stark.generate_trace_and_public_inputs(ios_b)
    cfg = stark.config()
    one, fresh_a, fresh_b = (gpu.Prover(stark, cfg, bits) for _ in range(3))
    try:
        one.load_trace(c["trace"], c["pi"])
        a = one.prove()
        one.load_trace(trace_b, pi_b)
        b = one.prove()
        assert _skipped(one) > 0
        fresh_a.load_trace(c["trace"], c["pi"])
        fresh_b.load_trace(trace_b, pi_b)
        assert np.array_equal(a.words, fresh_a.prove().words) and np.array_equal(b.words, fresh_b.prove().words)
        assert _skipped(fresh_a) == 0 and _skipped(fresh_b) == 0
        assert not np.array_equal(a.words, b.words)
    finally:
        for p in (one, fresh_a, fresh_b):
            p.close()


def test_next_trace_on_the_same_prover_generated_on_the_device(gpu, O, g1exp_case):
    """The same with the witness built on the device, whose scratch lives at the start of the LDE buffer: it ends in front of
    the block's LDE, so the second proof leaves the block untransformed, and equals a fresh prover's."""
    stark = gpu.G1ExpStark(128)
    cfg = stark.config()
    ios_b, _ = O.g1exp_inputs(128, 101)
    one, fresh = gpu.Prover(stark, cfg, 16), gpu.Prover(stark, cfg, 16)
    try:
        one.generate_trace(g1exp_case["ios"])
        a = one.prove()
        assert _skipped(one) == 0
        one.generate_trace(ios_b)
        b = one.prove()
        assert _skipped(one) == 516
        one.generate_trace(g1exp_case["ios"])
        a2 = one.prove()
        assert _skipped(one) == 516 and np.array_equal(a.words, a2.words)
        fresh.generate_trace(ios_b)
        assert np.array_equal(b.words, fresh.prove().words) and _skipped(fresh) == 0
        gpu.verify_stark_proof(stark, b, cfg)
    finally:
        one.close()
        fresh.close()


def test_other_words_in_the_block_fall_back_and_invalidate(gpu, golden, request, monkeypatch):
    """A valid witness that differs inside the block (a pulse witness at its own pulse row is unconstrained; the generators write
    0) and an invalid one (a pulse column flipped) are proved as before the block was kept -- the words of a prover created with
    SBN_FIXED_COLUMNS=0 -- nothing is left untransformed, and the canonical trace loaded next is transformed whole once more."""
    table = "fq12expu64"
    stark, bits, c, key = _case(gpu, request, table)
    rpb = CASES[table][5]
    f0, f1, io0 = _io_columns(gpu, table)
    cfg = stark.config()
    want = golden["proof_digests"][key]["proof_sha256"]
    q = 3
    pos = _pulse_pos(q, rpb)
    valid = c["trace"].copy()
    assert int(valid[io0 + 1 + 2 * q, pos]) == 0 and int(valid[io0 + 2 + 2 * q, pos]) == 1
    valid[io0 + 1 + 2 * q, pos] = 5
    invalid = c["trace"].copy()
    invalid[io0 + 2 + 2 * q, pos + 1] ^= 1
    on = gpu.Prover(stark, cfg, bits)
    monkeypatch.setenv("SBN_FIXED_COLUMNS", "0")
    off = gpu.Prover(stark, cfg, bits)
    monkeypatch.delenv("SBN_FIXED_COLUMNS")
    try:
        assert on.describe()["fixed_columns"] == "1" and off.describe()["fixed_columns"] == "0" and off.describe()["fixed_columns_range"] == "0:0"
        for other in (valid, invalid):
            on.load_trace(c["trace"], c["pi"])
            assert _digest(on.prove()) == want and _digest(on.prove()) == want and _skipped(on) == f1 - f0   # the block's transforms are resident
            on.load_trace(other, c["pi"])
            off.load_trace(other, c["pi"])
            p_on, p_off = on.prove(), off.prove()
            assert _skipped(on) == 0 and _skipped(off) == 0
            assert np.array_equal(p_on.words, p_off.words) and _digest(p_on) != want
            if other is valid:
                gpu.verify_stark_proof(stark, p_on, cfg)
            assert np.array_equal(on.prove().words, p_on.words) and _skipped(on) == 0                            # and stays on the long path
            on.load_trace(c["trace"], c["pi"])
            assert _digest(on.prove()) == want and _skipped(on) == 0      # d_coef / d_lde held the other words: transformed whole
            assert _digest(on.prove()) == want and _skipped(on) == f1 - f0
        off.load_trace(c["trace"], c["pi"])
        assert _digest(off.prove()) == want and _digest(off.prove()) == want and _skipped(off) == 0
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("table", ["fq12expu64", "fq12exp"])
def test_check_kernel_alone(table, gpu, request):
    """sbn_fixed_columns_check (2^11 rows; 2^13 for the table with a periodic pulse) accepts the generators' block and refuses one
    changed word anywhere: first and last column, first and last row, a pulse row, a word that is the right field element in a
    non-canonical form."""
    stark, bits, c, key = _case(gpu, request, table)
    rpb, periodic = CASES[table][5], CASES[table][6]
    f0, f1, io0 = _io_columns(gpu, table)
    n = 1 << bits
    block = c["trace"][f0:f1].copy()
    check = lambda b: gpu.api.fixed_columns_check(stark, bits, b)   # noqa: E731
    assert check(block) is True
    q = 2 * stark.num_io - 1
    pos = _pulse_pos(q, rpb)
    wit, pul = io0 - f0 + 1 + 2 * q, io0 - f0 + 2 + 2 * q
    changes = [(0, 5, 1), (f1 - f0 - 1, 7, 1),                      # first / last column of the block
               (wit - 2, 0, 1), (wit - 2, n - 1, 1),                # row 0 / row n - 1 (a pulse witness: an inverse)
               (pul, 0, 1), (pul, n - 1, 1), (io0 - f0, n - 1, 1),  # ... of a pulse column, of the io counter
               (wit, pos, 5), (pul, pos, 1),                        # the pulse row: the unconstrained witness word, the pulse itself
               (wit, pos - 1, 1)]                                   # the word next to it
    # the right field element in a non-canonical form: the witness of pulse 2 one row behind its pulse is 1/1; 1 + p fits 64 bits
    assert int(block[io0 - f0 + 5, rpb + 1]) == 1
    changes.append((io0 - f0 + 5, rpb + 1, GL_P))
    if periodic:
        changes += [(1, 62, 3), (1, 63, 1), (1, n - 1, GL_P), (0, n - 1, 64)]   # periodic witness at its pulse row and beside it
    for col, row, delta in changes:
        b = block.copy()
        b[col, row] = (int(b[col, row]) + delta) % (1 << 64)
        assert not np.array_equal(b, block)
        assert check(b) is False, (col, row, delta)
    with pytest.raises(gpu.SbnError):
        gpu.api.fixed_columns_check(gpu.G1Stark(), 9, np.zeros((0, 512), dtype=np.uint64))


@pytest.mark.parametrize("table,chunk", [("fqexp", 8), ("fq12exp", 40), ("fq12exp", 200), ("fq12exp", 152)])
def test_block_against_every_chunk_alignment(table, chunk, gpu, golden, request, monkeypatch):
    """Under SBN_NTT_CHUNK (read when the prover is created).  8, on FqExpStark(128), block 158..674 (a commitment has at most 512
    chunks, which the 9,802 columns of the Fq12 table exceed at 8), and 40, on Fq12ExpStark(16), block 1742..1810: the block
    starts and ends inside chunks and holds whole chunks; 200: it is smaller than a chunk and straddles a boundary; 152: it lies
    inside one chunk, which is transformed as the two pieces around it.  The proofs are those of the default chunking."""
    stark, bits, c, key = _case(gpu, request, table)
    f0, f1 = gpu.api.fixed_columns_range(stark)
    assert (f0, f1) == {"fqexp": (158, 674), "fq12exp": (1742, 1810)}[table] and f0 % chunk and f1 % chunk
    inside = [k for k in range(-(-stark.num_columns // chunk)) if k * chunk >= f0 and (k + 1) * chunk <= f1]
    holds = [k for k in range(-(-stark.num_columns // chunk)) if k * chunk < f0 and f1 < (k + 1) * chunk]
    assert (len(inside), len(holds)) == {8: (64, 0), 40: (1, 0), 200: (0, 0), 152: (0, 1)}[chunk]
    monkeypatch.setenv("SBN_EXPERIMENTAL", "1")
    monkeypatch.setenv("SBN_NTT_CHUNK", str(chunk))
    prover = gpu.Prover(stark, stark.config(), bits)
    try:
        assert prover.describe()["ntt_chunk"] == str(chunk)
        prover.load_trace(c["trace"], c["pi"])
        digests, skipped = [], []
        for _ in range(3):
            digests.append(_digest(prover.prove()))
            skipped.append(_skipped(prover))
    finally:
        prover.close()
    assert digests == [golden["proof_digests"][key]["proof_sha256"]] * 3
    assert skipped == [0, f1 - f0, f1 - f0]
