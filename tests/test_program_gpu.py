"""GPU tests of the field programs (run with `-m gpu` on the MI355X box).  The yardstick is the code that was there before:
Prover.generate_trace and BatchProver.prove_ios on the explicit list sbn_program_instances derives on the host, itself held against
Python in tests/test_program_host.py.  generate_trace_program must load that trace word for word -- on the Fq12 tables the links
are resolved on the device, one launch per level --, return the same public inputs, list and outputs, and prove to the same words;
prove_program gives the proofs of prove_ios on the units; a refused call leaves no trace loaded and the prover usable; and the
existing tower and chained calls give the words of the same lists written as programs.  Shapes: the smallest that reach every
path (one level, sixteen levels, both kinds of chain, a diamond, fifteen pads, pads that copy derived words)."""
import numpy as np
import pytest

import power_lists as PL
import program_lists as G
import tracegen_edges as T
from test_msm_gpu import _same_words

pytestmark = pytest.mark.gpu
BAD_ARG, NON_CANONICAL, VERIFY_FAILED = -1, -2, -6
HOST_CHAIN = {"SBN_EXPERIMENTAL": "1", "SBN_FQ12_HOST_CHAIN": "1"}
P = PL.P


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


def _same_trace(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, bad[:8].tolist()


def _compare_with_the_explicit_list(gpu, table, num_io, nodes, values, exps, envs=({},), prove=False):
    """generate_trace_program against generate_trace on the host-derived list on the same prover (trace by read_trace, public
    inputs, outs, ios), in every placement of `envs`; with prove, the proof words of both.  Returns (proof, outs, public inputs)."""
    stark = T.stark_class(gpu, table)(num_io)
    cfg = stark.config()
    bits = T.degree_bits(table, num_io)
    arr = G.arrays(table, nodes, values, exps)
    ios, outs_want = gpu.program_instances(stark, *arr)
    assert ios.shape[0] == 1
    proof = pi_want = None
    for env in envs:
        with T.placement(gpu, stark, cfg, bits, env) as pr:
            pi_want = pr.generate_trace(ios[0])
            trace_want = pr.read_trace()
            want = pr.prove().words if prove else None
            pi, outs, ios_got = pr.generate_trace_program(*arr)
            assert np.array_equal(ios_got, ios[0]) and np.array_equal(pi, pi_want), env
            assert np.array_equal(outs, outs_want), env
            _same_trace(pr.read_trace(), trace_want)
            if prove:
                proof = pr.prove()
                assert np.array_equal(proof.words, want), env
    return proof, outs_want, pi_want


FQ12_EXPS = [0, (1 << 256) - 1, 1, 2, P - 2, P] + [PL.rng(7).randrange(1 << 256) for _ in range(10)]


def _fq12_values(seed, count, zero_at=None):
    r = PL.rng(seed)
    values = [PL.random_elem("fq12", r) for _ in range(count)]
    if zero_at is not None:
        values[zero_at] = [0] * 12
    return values


SHAPES = {
    # 16 independent nodes, one level: per-node literals and exponents (0 and 2^256 - 1 among them), a zero base, a literal offset
    "sixteen_independent": lambda: ([(k, G.ONE if k % 3 else (k + 1) % 16, k) for k in range(16)], _fq12_values(3, 16, zero_at=2), FQ12_EXPS),
    # an x-chain of 16: sixteen levels, one workgroup each
    "x_chain_of_sixteen": lambda: ([(0, G.ONE, 0)] + [(G.out(k - 1), G.ONE, k % 3) for k in range(1, 16)], _fq12_values(4, 1), FQ12_EXPS[6:9]),
    # an offset-chain of 16 from a literal start
    "offset_chain_of_sixteen": lambda: (G.chain_as_program(16), _fq12_values(5, 17), FQ12_EXPS[:16][::-1]),
    # a diamond: two nodes from one literal, a third taking one as x and the other as offset, a fourth using the third twice
    "diamond": lambda: ([(0, G.ONE, 0), (0, G.ONE, 1), (G.out(0), G.out(1), 2), (G.out(2), G.out(2), 3)], _fq12_values(6, 1), FQ12_EXPS[6:10]),
    "one_node_fifteen_pads": lambda: ([(0, 1, 0)], _fq12_values(7, 2), FQ12_EXPS[10:11]),
    # 5 nodes whose last is linked in x and offset: the eleven pads copy derived words
    "five_nodes_last_linked": lambda: ([(0, G.ONE, 0), (1, 0, 1), (G.out(0), G.ONE, 2), (1, G.out(1), 0), (G.out(3), G.out(2), 1)], _fq12_values(8, 2), FQ12_EXPS[11:14]),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fq12_programs_equal_the_explicit_list(gpu, shape):
    """Fq12ExpStark(16), 2^13 rows.  The diamond is also proved and verified."""
    nodes, values, exps = SHAPES[shape]()
    want_depth = {"sixteen_independent": 1, "x_chain_of_sixteen": 16, "offset_chain_of_sixteen": 16, "diamond": 3, "one_node_fifteen_pads": 1, "five_nodes_last_linked": 3}
    assert gpu.program_levels(nodes)[1] == want_depth[shape]
    proof, outs, pi = _compare_with_the_explicit_list(gpu, "fq12", 16, nodes, values, exps, prove=shape == "diamond")
    if proof is not None:
        stark = gpu.Fq12ExpStark(16)
        gpu.verify_stark_proof(stark, proof, stark.config())
        assert np.array_equal(gpu.verify_program(stark, stark.config(), [proof], *G.arrays("fq12", nodes, values, exps)), outs)
        ev = G.evaluate("fq12", nodes, values, exps)                           # ... and the outputs are Python's
        assert [PL.elem_from_words("fq12", o.tolist()) for o in outs] == [o for _, _, o in ev]


def test_the_dag_on_fq12_u64_proves_and_checks_in_both_placements(gpu):
    """Fq12ExpU64Stark(16), 2^11 rows: the DAG of the host tests in one unit (11 nodes, 5 pads), on the device and under the
    host-chain switch: the same words, proved, verified and checked."""
    nodes, values, exps = G.dag("fq12u64")
    assert G.dag_properties(nodes, values, exps, 4) == G.DAG_PROPERTIES
    proof, outs, pi = _compare_with_the_explicit_list(gpu, "fq12u64", 16, nodes, values, exps, envs=({}, HOST_CHAIN), prove=True)
    stark = gpu.Fq12ExpU64Stark(16)
    gpu.verify_stark_proof(stark, proof, stark.config())
    arr = G.arrays("fq12u64", nodes, values, exps)
    assert np.array_equal(proof.public_inputs(), pi)
    assert np.array_equal(gpu.program_check(stark, [pi], *arr), outs)
    assert np.array_equal(outs, G.explicit_units("fq12u64", nodes, values, exps, 16)[1])


def test_fq_program_takes_the_explicit_path(gpu):
    """FqExpStark(128), 2^16 rows, the table's minimum: 40 nodes (a seeded DAG: every node links to up to two earlier ones) and 88 pads."""
    r = PL.rng(9)
    values = [0, 1, P - 1] + [r.randrange(P) for _ in range(5)]
    exps = [0, 1, P - 2, (1 << 256) - 1] + [r.randrange(1 << 256) for _ in range(4)]

    def operand(g, may_be_one):
        pick = r.randrange(3 if g else 2)
        if pick == 2:
            return G.out(r.randrange(g))
        return G.ONE if (pick == 1 and may_be_one) else r.randrange(len(values))
    nodes = [(operand(g, False), operand(g, True), r.randrange(len(exps))) for g in range(40)]
    assert gpu.program_levels(nodes)[1] > 2
    _, outs, _ = _compare_with_the_explicit_list(gpu, "fq", 128, nodes, values, exps)
    assert [PL.from_limbs(o) for o in outs] == [o for _, _, o in G.evaluate("fq", nodes, values, exps)]


def test_prove_program_equals_prove_ios_and_verifies(gpu):
    """BatchProver on Fq12ExpU64Stark(4), 2^9 rows: 9 nodes in 3 units with links across both boundaries, 3 pads."""
    r = PL.rng(10)
    values = [PL.random_elem("fq12", r) for _ in range(2)]
    exps = [PL.BN_X, 1, r.randrange(PL.GLP)]
    nodes = [(0, G.ONE, 0), (1, 0, 1), (G.out(0), G.out(1), 2), (G.out(2), G.ONE, 0),
             (G.out(3), G.out(1), 1), (G.out(4), G.out(4), 2), (1, G.out(2), 0), (G.out(6), G.out(5), 1),    # 4 <- 3, 1; 6 <- 2: the first boundary
             (G.out(7), G.out(3), 2)]                                                                            # 8 <- 7, 3: the second
    arr = G.arrays("fq12u64", nodes, values, exps)
    stark = gpu.Fq12ExpU64Stark(4)
    cfg = stark.config()
    units, outs_want = gpu.program_instances(stark, *arr)
    assert units.shape == (3, 4, 194)
    bp = gpu.BatchProver(stark, cfg, 9, inflight=2)
    ver = gpu.Verifier(stark, cfg, 9, max_batch=2)
    try:
        want = [p.words for p in bp.prove_ios(units)]
        proofs, outs, ios = bp.prove_program(*arr)
        assert np.array_equal(ios, units) and np.array_equal(outs, outs_want)
        _same_words(proofs, want)
        for v in (None, ver):
            assert np.array_equal(gpu.verify_program(stark, cfg, proofs, *arr, verifier=v), outs_want)
            with pytest.raises(gpu.SbnError) as e:                               # two unit proofs swapped: every proof verifies, a link does not
                gpu.verify_program(stark, cfg, [proofs[0], proofs[2], proofs[1]], *arr, verifier=v)
            assert e.value.code == VERIFY_FAILED and "instance 4:" in str(e.value), str(e.value)
        # a refused list (a forward link; a coefficient >= p in a used literal) leaves every proof null and the batch prover usable
        bad_nodes = arr[0].copy()
        bad_nodes[5, 0] = G.out(5)
        with pytest.raises(gpu.SbnError) as e:
            bp.prove_program(bad_nodes, arr[1], arr[2])
        assert e.value.code == BAD_ARG and "node 5: x links to node 5" in str(e.value), str(e.value)
        bad_values = arr[1].copy()
        bad_values[1, 8:16] = PL.limbs(P, 8)
        with pytest.raises(gpu.SbnError) as e:
            bp.prove_program(arr[0], bad_values, arr[2])
        assert e.value.code == BAD_ARG and "literal 1" in str(e.value), str(e.value)
        _same_words(bp.prove_program(*arr)[0], want)
    finally:
        ver.close()
        bp.close()


def test_a_refused_call_leaves_no_trace_loaded_and_the_prover_usable(gpu):
    stark = gpu.Fq12ExpU64Stark(16)
    cfg = stark.config()
    nodes, values, exps = G.dag("fq12u64")
    n, v, e = G.arrays("fq12u64", nodes, values, exps)
    too_many = np.array([(0, G.ONE, 0)] * 17, dtype=np.uint32)
    forward = n.copy()
    forward[4, 1] = G.out(4)
    too_big = v.copy()
    too_big[1, 40:48] = PL.limbs(P, 8)
    bad_exp = e.copy()
    bad_exp[3] = PL.limbs(PL.GLP, 2)
    with T.placement(gpu, stark, cfg, 11, {}) as pr:
        pi, outs, _ = pr.generate_trace_program(n, v, e)
        want = pr.prove().words
        for bad_call, code in ((lambda: pr.generate_trace_program(too_many, v, e), BAD_ARG),              # 17 nodes > 16
                               (lambda: pr.generate_trace_program(forward, v, e), BAD_ARG),
                               (lambda: pr.generate_trace_program(n, too_big, e), BAD_ARG),
                               (lambda: pr.generate_trace_program(n, v, bad_exp), NON_CANONICAL)):
            with pytest.raises(gpu.SbnError) as err:
                bad_call()
            assert err.value.code == code, str(err.value)
            with pytest.raises(gpu.SbnError) as err:
                pr.prove()
            assert err.value.code == BAD_ARG                                 # no trace is loaded
            pi2, outs2, _ = pr.generate_trace_program(n, v, e)
            assert np.array_equal(pi2, pi) and np.array_equal(outs2, outs)
        assert np.array_equal(pr.prove().words, want)
        gpu.verify_stark_proof(stark, gpu.Proof(want, 11), cfg)


def test_the_tower_and_chained_calls_give_the_words_of_their_programs(gpu):
    """Fq12ExpStark(16): generate_trace_powers (5 towers of depth 3, one pad) and generate_trace_chained (16 terms) against the same
    lists written as programs, on one prover: public inputs, list, outputs and the trace."""
    stark = gpu.Fq12ExpStark(16)
    cfg = stark.config()
    r = PL.rng(11)
    bases = [PL.random_elem("fq12", r) for _ in range(5)]
    tower_exps = [r.randrange(1 << 256) for _ in range(5)]
    start, xs = PL.random_elem("fq12", r), [PL.random_elem("fq12", r) for _ in range(16)]
    chain_exps = [r.randrange(1 << 256) for _ in range(16)]
    terms = np.array([PL.elem_words("fq12", x) + PL.limbs(e, 8) for x, e in zip(xs, chain_exps)], dtype=np.uint32)
    with T.placement(gpu, stark, cfg, 13, {}) as pr:
        pi_want, powers, ios_want = pr.generate_trace_powers(PL.base_words("fq12", bases), PL.exp_words("fq12", tower_exps), 3)
        trace_want = pr.read_trace()
        pi, outs, ios = pr.generate_trace_program(*G.arrays("fq12", G.towers_as_program(5, 3, False), bases, tower_exps))
        assert np.array_equal(pi, pi_want) and np.array_equal(ios, ios_want) and np.array_equal(outs, powers.reshape(15, 96))
        _same_trace(pr.read_trace(), trace_want)
        pi_want, ios_want = pr.generate_trace_chained(terms, np.array(PL.elem_words("fq12", start), dtype=np.uint32))
        trace_want = pr.read_trace()
        pi, outs, ios = pr.generate_trace_program(*G.arrays("fq12", G.chain_as_program(16), [start] + xs, chain_exps))
        assert np.array_equal(pi, pi_want) and np.array_equal(ios, ios_want)
        _same_trace(pr.read_trace(), trace_want)
