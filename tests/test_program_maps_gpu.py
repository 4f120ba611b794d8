"""GPU tests of the mapped links of the field programs and of the final exponentiation (run with `-m gpu` on the MI355X box).  The
yardstick is the explicit path: Prover.generate_trace and BatchProver.prove_ios on the list sbn_program_m_instances derives on the
host, itself held against Python in tests/test_program_maps_host.py.  generate_trace_program with mapped nodes must load that trace
word for word -- on the Fq12 tables a pre-pass in front of a level's launch writes the mapped words, the level kernel loads them as
literals --, return the same public inputs, list and outputs, and prove to the same words.  Shapes: the smallest that reach every
path (levels with and without a mapped operand, a level where only the offset is mapped, pads behind a mapped last node, mapped
links across unit boundaries, a map-free program through the mapped entry point, a refused call)."""
import numpy as np
import pytest

import power_lists as PL
import program_lists as G
import program_maps as PM
import tracegen_edges as T
from test_msm_gpu import _same_words

pytestmark = pytest.mark.gpu
BAD_ARG, VERIFY_FAILED = -1, -6
HOST_CHAIN = {"SBN_EXPERIMENTAL": "1", "SBN_FQ12_HOST_CHAIN": "1"}


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


def _same_trace(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, bad[:8].tolist()


def words(v):
    return np.array(PL.elem_words("fq12", v), dtype=np.uint32)


def elem(w):
    return PL.elem_from_words("fq12", np.asarray(w).reshape(-1).tolist())


def _compare_with_the_explicit_list(gpu, table, num_io, arr, envs=({},), prove=False):
    """generate_trace_program against generate_trace on the host-derived list on the same prover (trace by read_trace, public
    inputs, outs, ios), in every placement of `envs`; with prove, check_trace and the proof words of both.  Returns (proof, outs,
    public inputs)."""
    stark = T.stark_class(gpu, table)(num_io)
    cfg = stark.config()
    bits = T.degree_bits(table, num_io)
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
                assert pr.check_trace().ok, env
                proof = pr.prove()
                assert np.array_equal(proof.words, want), env
    return proof, outs_want, pi_want


@pytest.fixture(scope="module")
def inputs():
    r = PL.rng(501)
    return [PL.random_elem("fq12", r), PL.random_elem("fq12", r)]


def test_the_final_exponentiation_in_one_unit_in_both_placements(gpu, inputs):
    """Fq12ExpU64Stark(16), 2^11 rows: the 16 nodes fill the unit, ten levels, seven of them with a mapped operand."""
    f = inputs[0]
    stark = gpu.Fq12ExpU64Stark(16)
    pg = gpu.Program(stark)
    check, result = gpu.final_exponentiation(pg, words(f))
    arr = pg.arrays()
    assert arr[0].shape == (16, 4) and gpu.program_levels(arr[0])[1] == 10
    proof, outs, pi = _compare_with_the_explicit_list(gpu, "fq12u64", 16, arr, envs=({}, HOST_CHAIN), prove=True)
    gpu.verify_stark_proof(stark, proof, stark.config())
    assert np.array_equal(proof.public_inputs(), pi)
    assert np.array_equal(gpu.program_check(stark, [pi], *arr), outs)
    assert elem(outs[result.node]) == PM.final_exp_value(f) and elem(outs[check.node]) == PL.FQ12_ONE
    assert np.array_equal(gpu.verify_final_exponentiations(stark, stark.config(), [proof], words(f).reshape(1, 96)), outs[15:16])


def test_the_mapped_dag_on_fq12_equals_the_explicit_list(gpu):
    """Fq12ExpStark(16), 2^13 rows: the mapped DAG cut to 11 nodes -- five pads behind a mapped last node, levels with and without a
    mapped operand, a level where only the offset is mapped."""
    nodes, values, exps = PM.dag("fq12")
    nodes = nodes[:PM.CUT]
    assert len(nodes) == 11 and PM.CUT_PROPERTIES <= PM.dag_properties(nodes, 4)
    arr = PM.arrays("fq12", nodes, values, exps)
    _, outs, _ = _compare_with_the_explicit_list(gpu, "fq12", 16, arr)
    assert np.array_equal(outs, PM.explicit_units("fq12", nodes, values, exps, 16)[1])


def test_two_final_exponentiations_as_units_of_four(gpu, inputs):
    """BatchProver on Fq12ExpU64Stark(4), 2^9 rows: 32 nodes over 8 units, mapped links across unit boundaries."""
    stark = gpu.Fq12ExpU64Stark(4)
    cfg = stark.config()
    fs = np.stack([words(f) for f in inputs])
    want_results = np.stack([words(PM.final_exp_value(f)) for f in inputs])
    pg = gpu.Program(stark)
    for f in fs:
        gpu.final_exponentiation(pg, f)
    arr = pg.arrays()
    units, outs_want = gpu.program_instances(stark, *arr)
    assert units.shape == (8, 4, 194) and "mapped_link_crosses_unit" in PM.dag_properties([tuple(n) for n in arr[0].tolist()], 4)
    bp = gpu.BatchProver(stark, cfg, 9, inflight=2)
    ver = gpu.Verifier(stark, cfg, 9, max_batch=4)
    try:
        want = [p.words for p in bp.prove_ios(units)]
        proofs, results, ios = bp.prove_final_exponentiations(fs)
        assert np.array_equal(ios, units) and np.array_equal(results, want_results) and np.array_equal(results, outs_want[15::16])
        _same_words(proofs, want)
        for v in (None, ver):
            assert np.array_equal(gpu.verify_final_exponentiations(stark, cfg, proofs, fs, verifier=v), want_results)
        # one flipped x word in a copy of a unit's public inputs: node 6 = instance 2 of unit 1, x = frob_2(node 2)
        pis = [p.public_inputs().copy() for p in proofs]
        pis[1][577 * 2 + 5] ^= 1
        with pytest.raises(gpu.SbnError) as e:
            gpu.program_check(stark, pis, *arr)
        assert e.value.code == VERIFY_FAILED and "instance 6: x differs from frob_2 of the output of node 2" in str(e.value), str(e.value)
        # a wrong inverse for input 1: the program is proved as it stands, and the verify helper names the input
        wrong = np.stack([gpu.fq12_inverse(fs[0]), gpu.fq12_inverse(fs[0])])
        bad_proofs, _, _ = bp.prove_final_exponentiations(fs, wrong)
        with pytest.raises(gpu.SbnError) as e:
            gpu.verify_final_exponentiations(stark, cfg, bad_proofs, fs)
        assert e.value.code == VERIFY_FAILED and "input 1:" in str(e.value), str(e.value)
    finally:
        ver.close()
        bp.close()


def test_a_map_free_program_and_a_refused_call_through_the_mapped_entry_point(gpu):
    """Fq12ExpU64Stark(16): four-column nodes with zero maps load the trace of the three-column call; a refused mapped call (map
    12) leaves no trace loaded and the prover usable."""
    stark = gpu.Fq12ExpU64Stark(16)
    cfg = stark.config()
    nodes, values, exps = G.dag("fq12u64")
    n3, v, e = G.arrays("fq12u64", nodes, values, exps)
    n4 = np.concatenate([n3, np.zeros((len(n3), 1), dtype=np.uint32)], axis=1)
    bad = n4.copy()
    bad[4, 3] = PM.maps_word(12, 0)
    mapped = n4.copy()
    mapped[4, 3] = PM.maps_word(6, 1)
    with T.placement(gpu, stark, cfg, 11, {}) as pr:
        pi3, outs3, ios3 = pr.generate_trace_program(n3, v, e)
        trace3 = pr.read_trace()
        pi4, outs4, ios4 = pr.generate_trace_program(n4, v, e)
        assert np.array_equal(pi4, pi3) and np.array_equal(outs4, outs3) and np.array_equal(ios4, ios3)
        _same_trace(pr.read_trace(), trace3)
        want = pr.prove().words
        with pytest.raises(gpu.SbnError) as err:
            pr.generate_trace_program(bad, v, e)
        assert err.value.code == BAD_ARG and "node 4: the map of x is 12" in str(err.value), str(err.value)
        with pytest.raises(gpu.SbnError) as err:
            pr.prove()
        assert err.value.code == BAD_ARG                                     # no trace is loaded
        pi5, outs5, _ = pr.generate_trace_program(mapped, v, e)              # a good mapped call follows
        assert np.array_equal(outs5, gpu.program_instances(stark, mapped, v, e)[1]) and not np.array_equal(outs5, outs3)
        assert pr.check_trace().ok
        pi6, outs6, _ = pr.generate_trace_program(n4, v, e)
        assert np.array_equal(pi6, pi3) and np.array_equal(pr.prove().words, want)
