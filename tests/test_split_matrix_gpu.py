"""The split prover (sbn_split_prover_*, starky_bn254_amd/split.py) over everything create_ctx accepts for it (run on the MI355X
box with `-m gpu`): every kind of wide table at its smallest height over 2, 4, 8 and 16 ranks, every row of tests/config_matrix.py,
state carried from proof to proof, the diagnostics and the guard on a split context, and the refusals at creation.  All ranks are
threads of this process on device 0 (sbn_local_comm_create).  Every proof is compared WORD FOR WORD with the CPU oracle's proof, or
with the proof of a single-GPU Prover where the oracle would be too slow (the Exp tables; other tests pin that proof to the oracle).

What the shapes reach (tests/split_cases.py): ranks that own no trace block or no Z block (open_k is not launched, d_pairs_own is
absent), a partial last block on a rank other than the last, 64 local LDE rows (2^9 rows over 16 ranks: one leaf-sponge workgroup
a quarter full, a per-rank tree that is its own root), FRI layers shorter than the world, cap_height = log2(world) with both planes."""
import hashlib

import numpy as np
import pytest

import config_matrix as M
import split_cases as K
from starky_bn254_amd import split

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


def single_gpu_proof(gpu, stark, cfg, bits, ios):
    prover = gpu.Prover(stark, cfg, bits)
    try:
        prover.generate_trace(ios)
        return prover.prove().words
    finally:
        prover.close()


@pytest.fixture(scope="module")
def witnesses(gpu, O):
    """name -> the witness of a table of split_cases.TABLES and its reference proof under the default config, made on first use and
    shared by the worlds: {"stark", "bits", "trace" + "pi" + "kind" | "ios", "want"}."""
    made = {}

    def get(name):
        if name not in made:
            _, _, _, rows, witness, _ = K.table(name)
            stark, bits = K.make_stark(gpu, name), rows.bit_length() - 1
            if witness == "load":
                kind, inputs, seed = K.LOADED[name]
                trace = stark.generate_trace(getattr(O, inputs)(rows, seed)[0])
                w = {"kind": getattr(O, kind), "trace": trace, "pi": K.NO_PI, "want": O.prove(getattr(O, kind), 0, trace, K.NO_PI)[0]}
            else:
                inputs, seed = K.GENERATED[name]
                ios = getattr(O, inputs)(stark.num_io, seed)[0]
                w = {"ios": ios, "want": single_gpu_proof(gpu, stark, stark.config(), bits, ios)}
            made[name] = dict(w, stark=stark, bits=bits)
        return made[name]
    return get


# ------------------------------------------------------------------------------------------- 1. table x world, default config
def test_the_selection_reaches_every_edge_of_the_column_dealing(gpu):
    """From the tables' real column and Z counts (split.own_columns): the (table, world) pairs below contain a rank without a trace
    block, a rank without a Z block and a partial last block on a rank other than the last -- and the pairs chosen for an edge
    still have it."""
    reached = {(name, w): K.edge_shapes(K.make_stark(gpu, name), K.make_stark(gpu, name).config(), w) for name, w in K.TABLE_WORLDS}
    for edge in K.EDGES:
        assert any(edge in shapes for shapes in reached.values()), f"no (table, world) has {edge}"
    # FqExpStark(128) runs at world 16 only because rank 15 owns none of its 15 trace blocks there
    own = K.shares(gpu.FqExpStark(128), gpu.FqExpStark(128).config(), 16)
    assert own[15][0] == 0 and all(c > 0 for c, _ in own[:15])
    assert {K.NO_TRACE_BLOCK, K.NO_Z_BLOCK} <= reached[("fqexp-128", 16)] and {K.NO_TRACE_BLOCK, K.NO_Z_BLOCK} <= reached[("modular-512", 16)]
    assert K.NO_Z_BLOCK in reached[("modular-512", 8)] and K.PARTIAL_INSIDE in reached[("modular-512", 4)]
    assert K.PARTIAL_INSIDE in reached[("g1op-512", 8)] and K.PARTIAL_INSIDE in reached[("fq12expu64-4", 2)]
    # every rank's share adds up to the table
    for name, w in K.TABLE_WORLDS:
        stark = K.make_stark(gpu, name)
        own = K.shares(stark, stark.config(), w)
        assert (sum(c for c, _ in own), sum(z for _, z in own)) == (stark.num_columns, stark.num_permutation_zs(stark.config()))


@pytest.mark.parametrize("name,world", K.TABLE_WORLDS, ids=lambda v: str(v))
def test_every_table_over_every_world(gpu, O, witnesses, name, world):
    """Every rank's proof equals the reference word for word, and the product verifier accepts rank 0's."""
    w = witnesses(name)
    stark, bits = w["stark"], w["bits"]
    cfg = stark.config()
    with K.switches(K.TIMEOUT):
        if "ios" in w:
            proofs, _ = split.prove_local(stark, cfg, bits, world, ios=w["ios"])
        else:
            proofs, _ = split.prove_local(stark, cfg, bits, world, trace=w["trace"], public_inputs=w["pi"])
    for r in range(world):
        what = M.difference(proofs[r].words, w["want"], O.poseidon_permute)
        assert what is None, f"{name}, rank {r} of {world}: {what}"
        assert np.array_equal(proofs[r].words, w["want"])
    gpu.verify_stark_proof(stark, proofs[0], cfg)


# ------------------------------------------------------------------------------------------- 2. the config matrix
def worlds_of(row, most=16):
    """World 2 and the largest world the row's cap height admits."""
    return sorted({2, min(most, 1 << row[0])})


@pytest.fixture(scope="module")
def g1op_1024(gpu, O):
    """The G1Stark trace of test_config_matrix_gpu.py's small_tables, and a store of the oracle's proofs of it by case."""
    pts, _ = O.g1op_inputs(1024, 3)
    return {"stark": gpu.G1Stark(), "trace": gpu.G1Stark().generate_trace(pts), "oracle": {}}


def oracle_proof(O, t, case, trace=None, name="A"):
    """The oracle's proof of the fixture's trace (or of `trace`, stored under `name`) under a case's config, computed once."""
    row, times_x = case
    key = (case, name)
    if key not in t["oracle"]:
        t["oracle"][key] = O.prove(O.AIR_G1_OP, 0, t["trace"] if trace is None else trace, K.NO_PI, config=row + (times_x,))[0]
    return t["oracle"][key]


def check_ranks(O, proofs, want, bits, row, what):
    for r, p in enumerate(proofs):
        M.check_header(p.words, bits, row)
        diff = M.difference(p.words, want, O.poseidon_permute)
        if diff is not None:
            pytest.fail(f"{what}, rank {r} of {len(proofs)}: the split proof differs from the reference: {diff}")
        assert np.array_equal(p.words, want)


@pytest.mark.parametrize("case,world", [(c, w) for c in M.CASES for w in worlds_of(c[0])], ids=lambda v: M.case_id(v) if isinstance(v, tuple) else f"world{v}")
def test_g1stark_under_every_config(gpu, O, g1op_1024, case, world):
    """G1Stark at 1024 rows under every row of the matrix (the -plain ones too), over two ranks and over as many as the cap admits
    (16 from cap_height 4 up, where 4 leaves one cap digest per rank): the oracle's proof under the same config on every rank."""
    row, times_x = case
    stark, cfg = g1op_1024["stark"], M.make_config(gpu, row, times_x)
    with K.switches(K.TIMEOUT):
        proofs, _ = split.prove_local(stark, cfg, 10, world, trace=g1op_1024["trace"], public_inputs=K.NO_PI)
    check_ranks(O, proofs, oracle_proof(O, g1op_1024, case), 10, row, M.case_id(case))
    gpu.verify_stark_proof(stark, proofs[0], cfg)


@pytest.mark.parametrize("row", M.WIDE_ROWS, ids=lambda r: "-".join(map(str, r)))
def test_wide_table_under_the_wide_rows(gpu, O, witnesses, row):
    """Fq12ExpU64Stark(4) (2^9 rows x 9744 columns, 153 + 84 blocks) over four ranks -- two for the cap_height 1 row, which admits no
    more -- against the single-GPU proof under the same config."""
    w = witnesses("fq12expu64-4")
    stark, cfg, world = w["stark"], M.make_config(gpu, row), min(4, 1 << row[0])
    want = single_gpu_proof(gpu, stark, cfg, 9, w["ios"])
    gpu.verify_stark_proof(stark, gpu.Proof(want, 9), cfg)
    with K.switches(K.TIMEOUT):
        proofs, _ = split.prove_local(stark, cfg, 9, world, ios=w["ios"])
    check_ranks(O, proofs, want, 9, row, "-".join(map(str, row)))


# ------------------------------------------------------------------------------------------- 3. state carried between proofs
def test_nothing_stale_between_proofs_of_different_traces(gpu, O, g1op_1024):
    """One set of four provers: prove A, load B and prove, load A again and prove.  The first and third proofs are equal (and A's
    oracle proof), the second is B's: send slots, exchange events and the views of the receive buffer carry nothing over."""
    stark, cfg = g1op_1024["stark"], g1op_1024["stark"].config()
    case = (M.DEFAULT, True)
    a = g1op_1024["trace"]
    b = stark.generate_trace(O.g1op_inputs(1024, 33)[0])
    want_a, want_b = oracle_proof(O, g1op_1024, case), oracle_proof(O, g1op_1024, case, trace=b, name="B")
    assert not np.array_equal(want_a, want_b)
    got = []
    with K.Ranks(stark, cfg, 10, 4) as ranks:
        for trace in (a, b, a):
            loaded = ranks.each(lambda p, r: p.load_trace(trace, K.NO_PI))
            assert loaded == [None] * 4, loaded
            got.append(ranks.prove())
    for r in range(4):
        assert np.array_equal(got[0][r].words, got[2][r].words), f"rank {r}"
    check_ranks(O, got[0], want_a, 10, M.DEFAULT, "trace A")
    check_ranks(O, got[1], want_b, 10, M.DEFAULT, "trace B after A")
    check_ranks(O, got[2], want_a, 10, M.DEFAULT, "trace A after B")


# ------------------------------------------------------------------------------------------- 4. diagnostics and the guard
SEED = 5


def diagnose(prover, rows):
    return prover.check_trace(SEED, flags=True), prover.explain_rows(rows, SEED), prover.explain_trace(SEED)


def test_diagnostics_on_a_split_context_of_one_rank(gpu, golden):
    """sbn_split_prover_check_trace / explain_rows / explain_trace at world 1, G1ExpStark(128): on the clean trace and on one with a
    single main-column cell changed (both through sbn_split_prover_load_trace) they report what a single-GPU Prover reports for the
    same trace; prove() afterwards still gives the committed proof of the clean trace."""
    import check_trace_cases as T
    c = T.case("g1exp")
    stark, cfg = c["stark"], c["stark"].config()
    cell = (512 * 77 + 5, c["cols"][0])            # new_x limb 0 of the add gadget, inside instance 77
    assert cell[1] < stark.num_main_columns
    bad = T.corrupt(c["trace"], [cell])
    rows = sorted({0, 255, 256, cell[0] - 1, cell[0], cell[0] + 1, c["n"] - 1})
    want = {}
    single = gpu.Prover(stark, cfg, 16)
    try:
        for name, trace in (("bad", bad), ("clean", c["trace"])):
            single.load_trace(trace, c["pi"])
            want[name] = diagnose(single, rows)
    finally:
        single.close()
    assert want["clean"][0].ok and want["clean"][2].ok and not want["bad"][0].ok and not want["bad"][2].ok
    assert want["bad"][0].row_flags[cell[0]] and not want["bad"][1][rows.index(cell[0])].ok
    with K.Ranks(stark, cfg, 16, 1) as ranks:
        sp = ranks.provers[0]
        for name, trace in (("bad", bad), ("clean", c["trace"])):
            sp.load_trace(trace, c["pi"])
            rep, by_row, whole = diagnose(sp, rows)
            assert rep == want[name][0], (name, str(rep), str(want[name][0]))
            assert np.array_equal(rep.row_flags, want[name][0].row_flags)
            assert by_row == want[name][1] and np.array_equal(by_row.block_flags, want[name][1].block_flags) and np.array_equal(by_row.z_flags, want[name][1].z_flags)
            assert whole == want[name][2]
            for f in ("block_failing_rows", "block_first_row", "z_failing_rows", "z_first_row"):
                assert np.array_equal(getattr(whole, f), getattr(want[name][2], f)), (name, f)
        proof = ranks.prove()[0]
    g = golden["proof_digests"]["g1exp_io128_seed1"]
    assert len(proof.words) == g["proof_words"]
    assert hashlib.sha256(proof.words.astype("<u8").tobytes()).hexdigest() == g["proof_sha256"]


def refused(results, fragment):
    """Every rank raised SbnError -7 with `fragment` in its message."""
    for r, e in enumerate(results):
        assert isinstance(e, split.api.SbnError) and e.code == -7 and fragment in e.reason, (r, e)


def test_diagnostics_are_refused_on_two_ranks_and_the_guard_always(gpu, O, g1op_1024):
    """World 2: each diagnostic is SBN_ERR_UNSUPPORTED on every rank, naming the rank.  sbn_split_prover_set_guard refuses every mode
    at every world size, 1 included -- also mode 0 (None): guard.hip turns a split context away before it looks at a valid mode.
    The provers prove correctly afterwards."""
    stark, cfg = g1op_1024["stark"], g1op_1024["stark"].config()
    want = oracle_proof(O, g1op_1024, (M.DEFAULT, True))
    for world in (1, 2):
        with K.Ranks(stark, cfg, 10, world) as ranks:
            assert ranks.each(lambda p, r: p.load_trace(g1op_1024["trace"], K.NO_PI)) == [None] * world
            if world > 1:
                for call in (lambda p, r: p.check_trace(SEED, flags=True), lambda p, r: p.explain_rows([0, 1], SEED), lambda p, r: p.explain_trace(SEED)):
                    res = ranks.each(call, collective=False)
                    refused(res, "runs on single-GPU provers")
                    assert all(f"rank {r} of {world}" in e.reason for r, e in enumerate(res))
            for mode in ("device", "host", None):
                refused(ranks.each(lambda p, r: p.set_guard(mode), collective=False), "a guard covers single-GPU provers")
            with pytest.raises(gpu.SbnError) as e:   # (an unknown mode is a bad argument, not an unsupported one)
                ranks.provers[0].set_guard(3)
            assert e.value.code == -1
            check_ranks(O, ranks.prove(), want, 10, M.DEFAULT, f"world {world} after the refusals")


# ------------------------------------------------------------------------------------------- 5. refusals at creation
def good_split_proof(gpu, O, t):
    """The same process then creates a good split prover and proves."""
    stark = t["stark"]
    with K.Ranks(stark, stark.config(), 10, 2) as ranks:
        assert ranks.each(lambda p, r: p.load_trace(t["trace"], K.NO_PI)) == [None, None]
        check_ranks(O, ranks.prove(), oracle_proof(O, t, (M.DEFAULT, True)), 10, M.DEFAULT, "after a refusal")


def create_refused(gpu, stark, cfg, bits, code, fragment, sizes_from=None, trim=(0, 0), env=None):
    """sbn_split_prover_create on rank 0 of a two-rank local group is refused with `code` and `fragment` in sbn_last_error."""
    sb, rb = split.exchange_bytes(*(sizes_from or (stark, cfg, bits)), 2)
    grp = split.LocalGroup(2, sb - trim[0], rb - trim[1])
    try:
        with K.switches(env or {}):
            with pytest.raises(gpu.SbnError) as e:
                split.SplitProver(stark, cfg, bits, transport=grp.comms[0])
    finally:
        grp.close()
    assert e.value.code == code and fragment in e.value.reason, e.value


@pytest.mark.parametrize("what", ["four-columns", "no-z", "rate-bits-3", "send-buffer-short", "receive-buffer-short", "ntt-chunk-48", "ntt-chunk-8"])
def test_refusals_at_creation(gpu, O, g1op_1024, what):
    """Each host-side argument check of create_ctx for a split context: the error code, a stable fragment of sbn_last_error, and a
    good two-rank proof by the same process afterwards.  (world > 2^cap_height: test_config_matrix_gpu.py.)"""
    g1 = g1op_1024["stark"]
    default = (g1, g1.config(), 10)
    if what == "four-columns":
        create_refused(gpu, gpu.LookupStark(), gpu.LookupStark().config(), 10, -7, "covers the wide tables (this one has 4 columns and 2 permutation Zs)", sizes_from=default)
    elif what == "no-z":
        create_refused(gpu, gpu.FlagStark(2), gpu.FlagStark(2).config(), 10, -7, "covers the wide tables (this one has 25 columns and 0 permutation Zs)", sizes_from=default)
    elif what == "rate-bits-3":
        cfg3 = gpu.StarkConfig.for_rate(3)
        with pytest.raises(gpu.SbnError) as e:
            split.exchange_bytes(g1, cfg3, 10, 2)
        assert e.value.code == -7 and "rate_bits = 1 only" in e.value.reason
        create_refused(gpu, g1, cfg3, 10, -7, "rate_bits = 1 only", sizes_from=default)
    elif what == "send-buffer-short":
        create_refused(gpu, *default, -1, "staging buffers of sbn_split_exchange_bytes", trim=(1, 0))
    elif what == "receive-buffer-short":
        create_refused(gpu, *default, -1, "staging buffers of sbn_split_exchange_bytes", trim=(0, 1))
    else:
        chunk = what.rsplit("-", 1)[1]
        create_refused(gpu, *default, -7, "blocks of 64: unset SBN_NTT_CHUNK", env={"SBN_EXPERIMENTAL": "1", "SBN_NTT_CHUNK": chunk})
    good_split_proof(gpu, O, g1op_1024)


def test_ntt_chunk_64_is_the_split_block_and_is_accepted(gpu, O, g1op_1024):
    """SBN_NTT_CHUNK = 64 names the block the split deals in: accepted, and the proof is the oracle's."""
    with K.switches({"SBN_EXPERIMENTAL": "1", "SBN_NTT_CHUNK": "64"}):
        good_split_proof(gpu, O, g1op_1024)
