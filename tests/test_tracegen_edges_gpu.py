"""GPU tests of the device witness generator at edge inputs (tests/tracegen_edges.py), run with `-m gpu` on the MI355X box:
edge-case instance lists of all five Exp tables in every placement of the chains against the oracle and Python integers, proofs of
them, degenerate curve instances refused in every placement, a prover left unloaded by every failed generate_trace, and the BN254
field helpers of the device witness (device build) against Python's % and pow."""
import numpy as np
import pytest

import tracegen_edges as T

pytestmark = pytest.mark.gpu
TABLES = ["g1", "g2", "fq", "fq12", "fq12u64"]
FQ12_PLACEMENTS = ({}, {"SBN_EXPERIMENTAL": "1", "SBN_FQ12_HOST_CHAIN": "1"}, {"SBN_EXPERIMENTAL": "1", "SBN_FQ12_ROW_KERNEL": "1"})


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


def _same_trace(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:8].tolist())


@pytest.mark.parametrize("table,kind", [(t, "edges") for t in TABLES] + [("g1", "identical"), ("fq", "identical")])
def test_edge_lists_device_witness_and_proof(gpu, O, table, kind):
    """Device trace and public inputs == the oracle's word for word in every placement of the chains, outputs == Python integers,
    and the proof of the list verifies under the product and the oracle verifiers (for the G1 edge list: every proof word ==
    the oracle's prove())."""
    ios, insts = T.edge_list(table) if kind == "edges" else T.identical_list(table)
    trace, pi = T.oracle_trace(table, ios)
    num_io = len(insts)
    stark = T.stark_class(gpu, table)(num_io)
    cfg = stark.config()
    bits = T.degree_bits(table, num_io)
    if table in ("g1", "g2"):
        T.check_every_chain_placement(gpu, stark, cfg, bits, ios, pi, trace)
    elif table in ("fq12", "fq12u64"):
        for env in FQ12_PLACEMENTS[1:]:
            with T.placement(gpu, stark, cfg, bits, env) as pr:
                assert np.array_equal(pr.generate_trace(ios), pi), env
                _same_trace(pr.read_trace(), trace, env)
    prover = gpu.Prover(stark, cfg, bits)
    try:
        got_pi = prover.generate_trace(ios)
        assert np.array_equal(got_pi, pi)
        _same_trace(prover.read_trace(), trace, "default")
        outs = T.outputs_from_pi(table, got_pi)
        for k, inst in enumerate(insts):
            assert outs[k] == T.expected_output(table, inst), f"instance {k}"
        if kind == "identical":
            return
        proof = prover.prove()
    finally:
        prover.close()
    gpu.verify_stark_proof(stark, proof, cfg)
    assert O.verify(T.AIR[table], num_io, proof.words) == (0, "")
    if table == "g1":
        want, _ = O.prove(O.AIR_G1_EXP, num_io, trace, pi)
        assert np.array_equal(proof.words, want)


def test_g1_edge_list_2pow17_rows(gpu):
    """The G1 edge list twice (the second copy reversed): 256 instances, 2^17 rows, device witness == the host generator."""
    ios, insts = T.edge_list("g1")
    ios2 = np.ascontiguousarray(np.concatenate([ios, ios[::-1]]))
    stark = gpu.G1ExpStark(256)
    cfg = stark.config()
    t_host, pi_host = stark.generate_trace_and_public_inputs(ios2)
    prover = gpu.Prover(stark, cfg, 17)
    try:
        assert np.array_equal(prover.generate_trace(ios2), pi_host)
        _same_trace(prover.read_trace(), t_host, "2^17")
    finally:
        prover.close()
    outs = T.outputs_from_pi("g1", pi_host)
    assert outs[:128] == outs[128:][::-1] == [T.expected_output("g1", i) for i in insts]


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_degenerate_instances_refused_in_every_placement(gpu, O, curve):
    """A collision b_t = +-a_t at step t in {0, 1, 31, 32, 128, 255} in the first, a middle or the last instance is refused with
    SBN_ERR_WITNESS in every placement of the chains, and leaves no trace loaded; the control twins (bit t cleared) give the
    oracle's trace in every placement."""
    cases = T.degenerate_cases(curve)
    ios_c, _ = T.controls_list(curve, cases)
    trace, pi = T.oracle_trace(curve, ios_c)
    stark = T.stark_class(gpu, curve)(T.SHAPE[curve][0])
    cfg = stark.config()
    for env in T.PLACEMENTS:
        with T.placement(gpu, stark, cfg, 16, env) as pr:
            for t, s, pos, bad, _ in cases:
                with pytest.raises(gpu.SbnError) as e:
                    pr.generate_trace(bad)
                assert e.value.code == -8, (env, t, s, pos)
                with pytest.raises(gpu.SbnError) as e:
                    pr.prove()
                assert e.value.code == -1, (env, t, s, pos)
            assert np.array_equal(pr.generate_trace(ios_c), pi), env
            _same_trace(pr.read_trace(), trace, env)


def _bad_lists(table, ios):
    """Instance lists the device generator must refuse: a coordinate equal to p in the first instance, 2^256 - 1 in the last one,
    and for Fq12U64 an exponent equal to the Goldilocks p."""
    out = []
    for k, v in ((0, T.P), (len(ios) - 1, (1 << 256) - 1)):
        b = ios.copy()
        b[k, 0:8] = T.limbs(v, 8, 32)
        out.append((f"coordinate {v:#x} in instance {k}", b, -1))
    if table == "fq12u64":
        b = ios.copy()
        b[len(ios) - 1, 192:194] = T.limbs(T.GLP, 2, 32)
        out.append(("exponent p_gl", b, -2))
    return out


@pytest.mark.parametrize("table", TABLES)
def test_failed_generate_trace_leaves_no_trace_loaded(gpu, table):
    """After any refused sbn_prover_generate_trace (out-of-range coordinate, degenerate instance, non-canonical exponent) prove()
    fails with SBN_ERR_BAD_ARG ("no trace loaded") instead of proving the previous list; a following valid list proves as before."""
    ios, insts = T.edge_list(table)
    stark = T.stark_class(gpu, table)(len(insts))
    cfg = stark.config()
    bad = _bad_lists(table, ios)
    if table in ("g1", "g2"):
        bad.append(("degenerate", T.degenerate_cases(table)[5][3], -8))
    prover = gpu.Prover(stark, cfg, T.degree_bits(table, len(insts)))
    try:
        pi = prover.generate_trace(ios)
        first = prover.prove()
        for what, b, code in bad:
            assert np.array_equal(prover.generate_trace(ios), pi)         # a loaded trace ...
            with pytest.raises(gpu.SbnError) as e:
                prover.generate_trace(b)                                  # ... then a refused list
            assert e.value.code == code, what
            with pytest.raises(gpu.SbnError) as e:
                prover.prove()
            assert e.value.code == -1 and "no trace loaded" in str(e.value), what
        assert np.array_equal(prover.generate_trace(ios), pi)
        again = prover.prove()
    finally:
        prover.close()
    assert np.array_equal(again.words, first.words)
    gpu.verify_stark_proof(stark, again, cfg)


def test_bn254_field_helpers_device_build(gpu):
    """sbn_bn254_fq_batch on the device: the 32-bit-limb mmul, fadd / fsub, finv_fermat, batch_inverse over groups of 8 and the Fq2
    inverse through the norm, on the special operands and a 2^16-element random sweep, against Python integers."""
    T.fq_field_parity(gpu, on_device=True)
