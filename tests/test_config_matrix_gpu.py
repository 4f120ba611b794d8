"""Every StarkConfig and every table height the device prover accepts (run on the MI355X box with `-m gpu`): each row of
tests/config_matrix.py is proved on the device and compared WORD FOR WORD with the CPU oracle's proof under the same config, so a
wrong leaf digest, fold, gather, cap or transcript step fails here; then every degree_bits from 9 to 22.  The slow cases (2^21 /
2^22-row LookupStark, 2^19-row ModularStark) come last."""
import time

import numpy as np
import pytest

import config_matrix as M

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
NO_PI = np.zeros(0, dtype=np.uint64)


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    return S


@pytest.fixture(scope="module")
def small_tables(gpu, O):
    """Hashed and unhashed leaves, with and without a Z commitment: G1Stark at 1024 rows, LookupStark at 4096 rows (4 columns
    and 2 Zs, every leaf its own digest), FlagStark(2) (1024 rows, no Z commitment)."""
    pts, _ = O.g1op_inputs(1024, 3)
    ins, tab = O.lookup_inputs(4096, 19)
    limbs, _ = O.flags_inputs(2, 28)
    g1, lk, fl = gpu.G1Stark(), gpu.LookupStark(), gpu.FlagStark(2)
    return {"g1op": (g1, O.AIR_G1_OP, 0, g1.generate_trace(pts), NO_PI), "lookup": (lk, O.AIR_LOOKUP, 0, lk.generate_trace(ins, tab), NO_PI),
            "flags": (fl, O.AIR_FLAGS, 2, fl.generate_trace(limbs), NO_PI)}


def check_against_oracle(gpu, O, stark, kind, num_io, trace, pi, case, prover=None):
    """Device proof == the oracle's under the same config, both verifiers accept, a second prove() is word-identical."""
    row, times_x = case
    cfg = M.make_config(gpu, row, times_x)
    bits = trace.shape[1].bit_length() - 1
    own = prover is None
    if own:
        prover = gpu.Prover(stark, cfg, bits)
        prover.load_trace(trace, pi)
    try:
        p1 = prover.prove()
        p2 = prover.prove()
    finally:
        if own:
            prover.close()
    t0 = time.time()
    want, _ = O.prove(kind, num_io, trace, pi, config=row + (times_x,))
    oracle_s = time.time() - t0
    M.check_header(p1.words, bits, row)
    what = M.difference(p1.words, want, O.poseidon_permute)   # names the first word and the first stage that differs
    if what is not None:
        pytest.fail(f"{M.case_id(case)}: device proof differs from the oracle's: {what}")
    assert np.array_equal(p1.words, want)
    assert np.array_equal(p1.words, p2.words)
    assert O.verify(kind, num_io, p1.words, config=row + (times_x,)) == (0, "")
    gpu.verify_stark_proof(stark, p1, cfg)
    return p1, oracle_s


@pytest.mark.parametrize("table", ["g1op", "lookup", "flags"])
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_small_tables_match_the_oracle_under_every_config(gpu, O, small_tables, table, case):
    stark, kind, num_io, trace, pi = small_tables[table]
    check_against_oracle(gpu, O, stark, kind, num_io, trace, pi, case)


@pytest.mark.parametrize("row", M.WIDE_ROWS, ids=lambda r: "-".join(map(str, r)))
def test_wide_table_matches_the_oracle(gpu, O, fq12expu64_case, row):
    """Fq12ExpU64Stark(16): 2^11 rows x 9792 columns, 1224 sponge blocks per leaf in 153 column chunks; the non-default arities and
    the two ends of the cap-height range (a cap of 8 ends every tree before the single-workgroup tail of tree_build_inner, a cap of 1
    runs that tail down to two nodes)."""
    check_against_oracle(gpu, O, gpu.Fq12ExpU64Stark(16), O.AIR_FQ12_EXP_U64, 16, fq12expu64_case["trace"], fq12expu64_case["pi"], (row, True))


def test_one_shot_contexts_of_two_configs_are_not_shared(gpu, O, small_tables):
    """The context cache of the one-shot prove() keys on the config: two calls on one table under two configs are two misses and
    leave two contexts; each proof is the oracle's for its own config, and a repeat of the first is a hit with the same words."""
    stark, kind, num_io, trace, pi = small_tables["g1op"]
    rows = [(4, 16, 1, 5, 84), (6, 16, 2, 3, 28)]
    gpu.prove_cache_configure(0)
    before = gpu.prove_cache_stats()
    gpu.prove_cache_configure(1 << 30)
    try:
        got = [gpu.prove(stark, M.make_config(gpu, row), trace, pi) for row in rows]
        st = gpu.prove_cache_stats()
        assert (st["misses"] - before["misses"], st["hits"] - before["hits"], st["contexts_resident"]) == (2, 0, 2)
        for row, proof in zip(rows, got):
            assert np.array_equal(proof.words, O.prove(kind, num_io, trace, pi, config=row)[0]), row
        again = gpu.prove(stark, M.make_config(gpu, rows[0]), trace, pi)
        st = gpu.prove_cache_stats()
        assert (st["misses"] - before["misses"], st["hits"] - before["hits"], st["contexts_resident"]) == (2, 1, 2)
        assert np.array_equal(again.words, got[0].words)
    finally:
        gpu.prove_cache_configure(0)
    assert gpu.prove_cache_stats()["contexts_resident"] == 0


def test_fqexp_2pow16_rows_arity_4(gpu, O, fqexp_case):
    """FqExpStark(128) (2^16 rows x 960 columns, witness generated on the device) at cap height 2, arity 4, final polynomial 2^3:
    seven FRI layers of 2^17, 2^15 .. 2^5 points instead of three, and a first layer of 2^15 leaves, which takes the
    one-lane-per-leaf form of the FRI leaf hash (at the default arity only a 2^18-row table reaches it)."""
    row = (2, 16, 2, 3, 84)
    assert M.fri_shape(16, row) == (7, 4)
    stark = gpu.FqExpStark(128)
    prover = gpu.Prover(stark, M.make_config(gpu, row), 16)
    try:
        assert np.array_equal(prover.generate_trace(fqexp_case["ios"]), fqexp_case["pi"])
        _, oracle_s = check_against_oracle(gpu, O, stark, O.AIR_FQ_EXP, 128, fqexp_case["trace"], fqexp_case["pi"], (row, True), prover=prover)
    finally:
        prover.close()
    print(f"FqExpStark(128) {row}: oracle {oracle_s:.1f} s")


def test_batch_prover_with_a_non_default_config(gpu, O):
    """BatchProver under an arity-2, cap-height-8 config: every unit's proof is the proof Prover gives for that instance list."""
    row = (8, 8, 1, 0, 3)
    stark = gpu.FqExpStark(128)
    cfg = M.make_config(gpu, row)
    units = [O.fqexp_inputs(128, seed)[0] for seed in (4, 44)]
    alone = []
    prover = gpu.Prover(stark, cfg, 16)
    try:
        for ios in units:
            prover.generate_trace(ios)
            alone.append(prover.prove())
    finally:
        prover.close()
    assert M.header(alone[0].words)[7:10] == (M.fri_shape(16, row)[0], 1, M.fri_shape(16, row)[1])
    gpu.verify_stark_proof(stark, alone[1], cfg)
    bp = gpu.BatchProver(stark, cfg, 16, 2)
    try:
        proofs = bp.prove_ios(np.stack([units[0], units[1], units[0]]))
    finally:
        bp.close()
    for k, want in ((0, alone[0]), (1, alone[1]), (2, alone[0])):
        assert np.array_equal(proofs[k].words, want.words), k
    assert not np.array_equal(alone[0].words, alone[1].words)


def test_split_prover_with_cap_height_1(gpu, O, g1exp_case):
    """G1ExpStark(128) over two ranks with cap_height = 1: each rank's subtree is exactly one cap digest (its tree runs down to a
    single root).  Both ranks' proofs equal the single-GPU proof of the same config, which both verifiers accept.  Four ranks cannot
    share two cap digests: refused with an error code."""
    from starky_bn254_amd import split
    gpu.lib().sbn_set_device(0)
    row = (1, 16, 4, 5, 84)
    stark = gpu.G1ExpStark(128)
    cfg = M.make_config(gpu, row)
    prover = gpu.Prover(stark, cfg, 16)
    try:
        prover.generate_trace(g1exp_case["ios"])
        single = prover.prove()
    finally:
        prover.close()
    assert M.header(single.words)[5] == 1
    assert O.verify(O.AIR_G1_EXP, 128, single.words, config=row) == (0, "")
    gpu.verify_stark_proof(stark, single, cfg)
    proofs, _ = split.prove_local(stark, cfg, 16, 2, ios=g1exp_case["ios"])
    for r in range(2):
        assert np.array_equal(proofs[r].words, single.words), f"rank {r}"
    with pytest.raises(gpu.SbnError) as e:
        split.prove_local(stark, cfg, 16, 4, ios=g1exp_case["ios"])
    assert e.value.code in (-1, -7)


# ---------------------------------------------------------------------------------------------------------------- sizes
def _lookup(gpu, O, bits, seed):
    ins, tab = O.lookup_inputs(1 << bits, seed)
    return gpu.LookupStark(), O.AIR_LOOKUP, 0, gpu.LookupStark().generate_trace(ins, tab), NO_PI


@pytest.mark.parametrize("num_io", [32, 64])
def test_flagstark_2pow14_and_2pow15_rows(gpu, O, num_io):
    """degree_bits 14 and 15, the two heights between 9 and 18 that no other proof has: hashed leaves."""
    stark = gpu.FlagStark(num_io)
    limbs, _ = O.flags_inputs(num_io, 100 + num_io)
    check_against_oracle(gpu, O, stark, O.AIR_FLAGS, num_io, stark.generate_trace(limbs), NO_PI, (M.DEFAULT, True))


@pytest.mark.parametrize("bits", [14, 15, 19, 20])
def test_lookup_table_heights(gpu, O, bits):
    """LookupStark (leaves that are their own digests) at 2^14 and 2^15 rows, and above 2^18 rows, where the commitments run their
    transforms on two streams and the generic transform pass takes 2^11-point rows."""
    _, oracle_s = check_against_oracle(gpu, O, *_lookup(gpu, O, bits, 200 + bits), (M.DEFAULT, True))
    print(f"LookupStark 2^{bits} rows: oracle {oracle_s:.1f} s")


def test_degree_bits_outside_9_to_22_are_refused(gpu):
    for bits in (8, 23):
        with pytest.raises(gpu.SbnError) as e:
            gpu.Prover(gpu.LookupStark(), gpu.LookupStark().config(), bits)
        assert e.value.code == -7


# ------------------------------------------------------------------------------------------- the slow cases, kept last
@pytest.mark.parametrize("bits", [21, 22])
def test_lookup_table_largest_heights(gpu, O, bits):
    """LookupStark at 2^21 and 2^22 rows, the largest the prover accepts (2^12-point rows in the generic transform pass).  Nearly all
    of the time is the oracle's proof on the CPU."""
    t0 = time.time()
    case = _lookup(gpu, O, bits, 200 + bits)
    t1 = time.time()
    _, oracle_s = check_against_oracle(gpu, O, *case, (M.DEFAULT, True))
    print(f"LookupStark 2^{bits} rows: inputs {t1 - t0:.1f} s, oracle {oracle_s:.1f} s, everything else {time.time() - t1 - oracle_s:.1f} s")


def test_modular_stark_2pow19_rows_through_the_verifiers(gpu, O):
    """A wide table above 2^18 rows: ModularStark at 2^19 rows (812 columns, 3.4 GB of trace; 48-column chunks on two transform
    streams).  An oracle proof of it is too slow for the suite, so the check is the two independent verifiers: both accept, and both
    reject a flipped opening and a flipped cap word."""
    stark = gpu.ModularStark()
    t0 = time.time()
    ops, _ = O.modular_inputs(1 << 12, 219)
    trace = stark.generate_trace(np.tile(ops, (1 << 7, 1)))
    t1 = time.time()
    cfg = stark.config()
    proof = gpu.prove(stark, cfg, trace, NO_PI)
    del trace
    t2 = time.time()
    assert M.header(proof.words)[:3] == (19, 812, stark.num_permutation_zs(cfg)) and M.header(proof.words)[7:10] == (M.fri_shape(19, M.DEFAULT)[0], 4, M.fri_shape(19, M.DEFAULT)[1])
    assert O.verify(O.AIR_MODULAR, 0, proof.words) == (0, "")
    gpu.verify_stark_proof(stark, proof, cfg)
    sections = M.section_words(proof.words)
    for name in ("opening", "cap"):
        bad = M.bump(proof.words, sections[name])
        assert O.verify(O.AIR_MODULAR, 0, bad)[0] != 0, name
        with pytest.raises(gpu.SbnError) as e:
            gpu.verify_stark_proof(stark, gpu.Proof(bad, 19), cfg)
        assert e.value.code == -6, name
    print(f"ModularStark 2^19 rows: host witness {t1 - t0:.1f} s, upload + prove {t2 - t1:.1f} s, verifiers {time.time() - t2:.1f} s")
