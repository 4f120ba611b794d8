"""GPU tests of the independent scalar multiplications (run with `-m gpu` on the MI355X box): Prover.generate_trace_scalar_muls
loads, word for word, the trace generate_trace loads from the explicit list, in every placement of the curve chains, and returns
the host function's products; BatchProver.prove_scalar_muls / prove_mul_by_cofactor give the proofs of prove_ios on the
Python-derived padded units and verify_scalar_muls / verify_mul_by_cofactor return Python's products; a list the table cannot
walk is an error return naming the instance, after which prover and batch prover still work.  Lists: tests/scalar_mul_lists.py."""
import ctypes
import re

import numpy as np
import pytest

import scalar_mul_lists as SL
import tracegen_edges as T
from test_msm_gpu import _same_words, batch_prover

pytestmark = pytest.mark.gpu
BAD_ARG, VERIFY_FAILED, WITNESS = -1, -6, -8
CHAIN = [{"SBN_TRACEGEN_DEVICE_CHAIN": m} for m in "012"]
BITS = 16
TRACE_CASES = [("g1", CHAIN[0]), ("g1", CHAIN[1]), ("g1", CHAIN[2]), ("g2", CHAIN[2])]


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


def _id(case):
    return f"{case[0]}-chain={case[1]['SBN_TRACEGEN_DEVICE_CHAIN']}"


@pytest.fixture(scope="module")
def explicit_trace(gpu):
    """(pi, trace) generate_trace loads from the explicit list of instances 0..127 (per-instance scalars, then the shared scalar),
    once per curve, from a prover in the default placement."""
    cache = {}

    def get(curve, shared):
        if (curve, shared) not in cache:
            points, scalars, off, _, _, _, _ = SL.case(curve)
            stark = T.stark_class(gpu, curve)(SL.NUM_IO)
            sc = scalars[6:7] if shared else scalars[:SL.NUM_IO]
            ios, products, inf = gpu.scalar_mul_instances(stark, points[:SL.NUM_IO], sc, off)
            with T.placement(gpu, stark, stark.config(), BITS, {}) as pr:
                pi = pr.generate_trace(ios[0])
                cache[(curve, shared)] = (ios[0], products, inf, pi, pr.read_trace())
        return cache[(curve, shared)]
    return get


@pytest.mark.parametrize("shared", [False, True], ids=["per_instance", "shared_scalar"])
@pytest.mark.parametrize("case", TRACE_CASES, ids=_id)
def test_generate_trace_scalar_muls_equals_the_explicit_list(gpu, explicit_trace, case, shared):
    curve, env = case
    points, scalars, off, units, products, inf, _ = SL.case(curve)
    ios_want, prod_want, inf_want, pi_want, trace_want = explicit_trace(curve, shared)
    if not shared:   # the host function against Python (the first unit of the seeded list)
        assert np.array_equal(ios_want, units[0]) and np.array_equal(prod_want, products[:SL.NUM_IO]) and np.array_equal(inf_want, inf[:SL.NUM_IO])
    stark = T.stark_class(gpu, curve)(SL.NUM_IO)
    sc = scalars[6] if shared else scalars[:SL.NUM_IO]                       # shared: 2^256 - 1, never reduced
    with T.placement(gpu, stark, stark.config(), BITS, env) as pr:
        pi, got, flags, ios = pr.generate_trace_scalar_muls(points[:SL.NUM_IO], sc, off)
        assert np.array_equal(ios, ios_want) and np.array_equal(pi, pi_want)
        assert np.array_equal(flags, inf_want) and np.array_equal(got, prod_want)
        trace = pr.read_trace()
        bad = np.nonzero((trace != trace_want).any(axis=1))[0]
        assert bad.size == 0, bad[:8].tolist()
        if not shared and curve == "g1" and env is CHAIN[2]:                 # offset=None is the generator, the same call
            pi2, got2, flags2, _ = pr.generate_trace_scalar_muls(points[:SL.NUM_IO], sc)
            assert np.array_equal(pi2, pi) and np.array_equal(got2, got) and np.array_equal(flags2, flags)


@pytest.fixture(scope="module")
def unit_proofs(gpu):
    """The proof words of prove_ios on the Python-derived padded units, once per list."""
    cache = {}

    def get(name):
        if name not in cache:
            curve = "g2" if name == "cofactor" else name
            units = SL.cofactor_case()[1] if name == "cofactor" else SL.case(curve)[3]
            with batch_prover(gpu, curve, {}) as bp:
                cache[name] = [p.words for p in bp.prove_ios(units)]
        return cache[name]
    return get


@pytest.mark.parametrize("case", [("g1", CHAIN[2]), ("g1", CHAIN[0]), ("g2", CHAIN[2])], ids=_id)
def test_prove_scalar_muls_equals_prove_ios_and_verifies(gpu, unit_proofs, case):
    curve, env = case
    points, scalars, off, units, products, inf, _ = SL.case(curve)
    with batch_prover(gpu, curve, env, inflight=2) as bp:
        proofs, got, flags, ios = bp.prove_scalar_muls(points, scalars, off)
    assert np.array_equal(ios, units) and np.array_equal(got, products) and np.array_equal(flags, inf)
    _same_words(proofs, unit_proofs(curve))
    stark = bp.stark
    cfg = stark.config()
    ver = gpu.Verifier(stark, cfg, BITS, max_batch=4) if curve == "g1" and env is CHAIN[2] else None
    try:
        for v in ([None, ver] if ver else [None]):
            got, flags = gpu.verify_scalar_muls(stark, cfg, proofs, points, scalars, off, verifier=v)
            assert np.array_equal(got, products) and np.array_equal(flags, inf)
            # one tampered public-input word (the output of instance 129): the unit proof no longer verifies
            broken = gpu.Proof(proofs[1].words.copy(), BITS)
            per = stark.num_public_inputs // SL.NUM_IO
            broken.words[len(broken.words) - stark.num_public_inputs + per + per - 1] ^= 1
            with pytest.raises(gpu.SbnError) as e:
                gpu.verify_scalar_muls(stark, cfg, [proofs[0], broken], points, scalars, off, verifier=v)
            assert e.value.code == VERIFY_FAILED and "unit 1" in str(e.value), str(e.value)
    finally:
        if ver:
            ver.close()


def test_prove_mul_by_cofactor_clears_the_twist_points(gpu, unit_proofs):
    points, units, cleared = SL.cofactor_case()
    with batch_prover(gpu, "g2", CHAIN[2], inflight=2) as bp:
        proofs, got, flags, ios = bp.prove_mul_by_cofactor(points)
    assert np.array_equal(ios, units) and np.array_equal(got, cleared) and not flags.any()
    _same_words(proofs, unit_proofs("cofactor"))
    stark = bp.stark
    got, flags = gpu.verify_mul_by_cofactor(stark, stark.config(), proofs, points)
    assert np.array_equal(got, cleared) and not flags.any()
    with batch_prover(gpu, "g1", {}, inflight=1) as b1:                      # the cofactor forms are calls of the twist
        with pytest.raises(gpu.SbnError) as e:
            b1.prove_mul_by_cofactor(points)
        assert e.value.code == BAD_ARG


def _collide_at(curve, k):
    """The seeded list with x = offset, e = 1 at instance k: the table's first addition meets B[0] = A[0]."""
    xs, es, off, _, _ = SL.seeded_list(curve)
    cx, ce = list(xs), list(es)
    cx[k], ce[k] = off, 1
    return SL.point_words(curve, cx), SL.scalar_words(ce)


@pytest.mark.parametrize("env", [CHAIN[2], CHAIN[1]], ids=["chain=2", "chain=1"])
def test_a_refused_list_names_its_instance_and_leaves_the_prover_usable(gpu, env):
    """Error returns of the library, not faults: the device path reports a degenerate walk through its error word and the host
    walk names instance 2; no trace is loaded; the next good call proves."""
    points, scalars, off, _, products, _, _ = SL.case("g1")
    bad_points, bad_scalars = _collide_at("g1", 2)
    stark = gpu.G1ExpStark(SL.NUM_IO)
    with T.placement(gpu, stark, stark.config(), BITS, env) as pr:
        pr.generate_trace_scalar_muls(points[:SL.NUM_IO], scalars[:SL.NUM_IO], off)
        with pytest.raises(gpu.SbnError) as e:
            pr.generate_trace_scalar_muls(bad_points[:SL.NUM_IO], bad_scalars[:SL.NUM_IO], off)
        assert e.value.code == WITNESS and re.search(r"instance 2\b", str(e.value)), str(e.value)
        with pytest.raises(gpu.SbnError) as e:
            pr.prove()
        assert e.value.code == BAD_ARG                                       # no trace is loaded
        pi, got, _, _ = pr.generate_trace_scalar_muls(points[:SL.NUM_IO], scalars[:SL.NUM_IO], off)
        assert np.array_equal(got, products[:SL.NUM_IO])
        proof = pr.prove()
        gpu.verify_stark_proof(stark, proof, stark.config())


def test_a_refused_list_leaves_the_batch_prover_usable(gpu, unit_proofs):
    points, scalars, off, _, _, _, _ = SL.case("g1")
    bad_points, bad_scalars = _collide_at("g1", 2)
    L = gpu.lib()
    with batch_prover(gpu, "g1", CHAIN[2], inflight=2) as bp:
        out = (ctypes.c_void_p * 2)(1, 1)                                     # stale values the call must clear
        rc = L.sbn_batch_prover_prove_scalar_muls(bp._h, bad_points.ctypes.data, bad_scalars.ctypes.data, SL.COUNT, SL.COUNT, off.ctypes.data,
                                                  out, None, None, None)
        msg = L.sbn_last_error().decode()
        assert rc == WITNESS and re.search(r"instance 2\b", msg), (rc, msg)
        assert [out[u] for u in range(2)] == [None, None]
        proofs, _, _, _ = bp.prove_scalar_muls(points, scalars, off)
        _same_words(proofs, unit_proofs("g1"))
