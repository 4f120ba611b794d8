"""GPU tests of the complete sums (run with `-m gpu` on the MI355X box; include/sbn.h, "Complete sums"):
Prover.generate_trace_msms_complete must return what the host function returns -- list, effective terms, starts, choice, finals,
sums and flags -- with the public inputs of the host generator on that list, in every placement of the curve chains
(SBN_TRACEGEN_DEVICE_CHAIN 0, 1, 2, set before the prover is created), on a unit that mixes benign segments, the trap of the
default start, head and middle kills, masked terms, an all-masked segment and segments of length 1; the trace passes check_trace
and its proof verifies with the returned starts.  Then two failing segments in different scan blocks of a unit of 1,024, the
exhausted list (no trace stays loaded), the batch forms, and the explicit-start calls before and after a complete call."""
import ctypes
import re

import numpy as np
import pytest

import chained_lists as CL
import complete_sums as CS
import msm_batches as MB
import tracegen_edges as T
from test_msm_gpu import batch_prover

pytestmark = pytest.mark.gpu
BAD_ARG, WITNESS = -1, -8
PLACEMENTS = T.PLACEMENTS[:3]          # SBN_TRACEGEN_DEVICE_CHAIN 0, 1, 2
CHAIN2 = PLACEMENTS[2]
_chain = lambda v: v if isinstance(v, str) else "chain=" + v["SBN_TRACEGEN_DEVICE_CHAIN"]   # noqa: E731


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


@pytest.fixture(scope="module")
def host_unit(S):
    """The host function's outputs on the unit recipe and the host generator's public inputs on its list, once per curve."""
    cache = {}

    def get(curve):
        if curve not in cache:
            terms, lengths, masks, want = CS.unit_recipe(curve)
            stark = T.stark_class(S, curve)(128)
            out = S.msm_batch_instances_complete(stark, terms, lengths, masks)
            assert out[3].tolist() == want and out[0].shape[0] == 1
            cache[curve] = (out, stark.generate_public_inputs(out[0][0]))
        return cache[curve]
    return get


def _same(got, want):
    """(terms_eff, starts, choice, finals, sums, infinity) of a prover call against the host function's (behind its ios)."""
    for name, g, w in zip(("terms_eff", "starts", "choice", "finals", "sums", "infinity"), got, want[1:]):
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("curve,env", [(c, env) for c in ("g1", "g2") for env in PLACEMENTS], ids=_chain)
def test_unit_equals_the_host_function_and_proves(gpu, host_unit, curve, env):
    terms, lengths, masks, want = CS.unit_recipe(curve)
    host, want_pi = host_unit(curve)
    stark = T.stark_class(gpu, curve)(128)
    cfg = stark.config()
    with T.placement(gpu, stark, cfg, 16, env) as pr:
        pi, *outs, ios = pr.generate_trace_msms_complete(terms, lengths, masks)
        report = pr.check_trace()
        proof = pr.prove()
    bad = np.nonzero((ios != host[0][0]).any(axis=1))[0]
    assert bad.size == 0, ("ios", bad[:8].tolist())
    _same(outs, host)
    assert outs[2].tolist() == want
    assert np.array_equal(pi, want_pi)
    assert report.ok, report
    fin, sums, inf = gpu.verify_msms(stark, cfg, [proof], lengths, starts=outs[1], terms=outs[0])
    assert np.array_equal(fin, host[4]) and np.array_equal(sums, host[5]) and np.array_equal(inf, host[6])


def test_two_failing_segments_in_different_scan_blocks(gpu):
    """A unit of 1,024 G1 instances is the smallest the scan takes in blocks of 512 lanes: segment 10 (block 0) moves to candidate
    1, segment 90 (block 1) to candidate 2, every other segment keeps candidate 0, a segment straddles the two blocks."""
    terms, lengths, want = CS.block_recipe()
    stark = gpu.G1ExpStark(1024)
    host = gpu.msm_batch_instances_complete(stark, terms, lengths)
    assert host[3].tolist() == want
    with T.placement(gpu, stark, stark.config(), 19, CHAIN2) as pr:
        pi, *outs, ios = pr.generate_trace_msms_complete(terms, lengths)
        report = pr.check_trace()
    bad = np.nonzero((ios != host[0][0]).any(axis=1))[0]
    assert bad.size == 0, ("ios", bad[:8].tolist())
    _same(outs, host)
    assert report.ok, report
    assert np.array_equal(pi.reshape(1024, -1)[:, :40], ios)           # x, offset, exponent of every instance, one u32 limb per word


@pytest.mark.parametrize("curve,env", [("g1", env) for env in PLACEMENTS] + [("g2", CHAIN2)], ids=_chain)
def test_exhausted_list_leaves_no_trace_loaded(gpu, host_unit, curve, env):
    terms, lengths, masks, _ = CS.unit_recipe(curve)
    bad_terms, bad_lengths = CS.unit_exhausted(curve)
    host, want_pi = host_unit(curve)
    stark = T.stark_class(gpu, curve)(128)
    cfg = stark.config()
    with T.placement(gpu, stark, cfg, 16, env) as pr:
        pr.generate_trace_msms_complete(terms, lengths, masks)         # a loaded trace that the refusal must drop
        with pytest.raises(gpu.SbnError) as e:
            pr.generate_trace_msms_complete(bad_terms, bad_lengths)
        assert e.value.code == WITNESS and re.search(r"segment 1\b.*candidate 7 fails at instance 9\b", str(e.value)), str(e.value)
        with pytest.raises(gpu.SbnError) as e:
            pr.prove()
        assert e.value.code == BAD_ARG
        off_curve = terms.copy()
        off_curve[0, 0] ^= 1
        with pytest.raises(gpu.SbnError) as e:
            pr.generate_trace_msms_complete(off_curve, lengths, masks)
        assert e.value.code == BAD_ARG and "instance 0 (segment 0)" in str(e.value), str(e.value)
        pi, *outs, ios = pr.generate_trace_msms_complete(terms, lengths, masks)
        proof = pr.prove()
    _same(outs, host)
    assert np.array_equal(pi, want_pi)
    gpu.verify_stark_proof(stark, proof, cfg)


@pytest.mark.parametrize("env", PLACEMENTS, ids=_chain)
def test_explicit_start_calls_are_untouched(gpu, env):
    """The explicit-start calls on the same prover return, after a complete call (one that moved segments to other candidates),
    the words and the refusal they returned before it."""
    xs, es, starts, insts, finals, sums = MB.curve_unit("g1", False)
    e_terms, e_lengths, e_starts = CL.terms_words("g1", xs, es), MB.lengths_words(MB.CURVE_LENGTHS), MB.starts_words("g1", starts)
    refused = CL.terms_words("g1", *MB.refusal_lists("g1")[0]["collide"])
    terms, lengths, masks, _ = CS.unit_recipe("g1")
    stark = gpu.G1ExpStark(128)

    def explicit(pr):
        got = pr.generate_trace_msms(e_terms, e_lengths, e_starts)
        trace = pr.read_trace()
        with pytest.raises(gpu.SbnError) as e:
            pr.generate_trace_msms(refused, e_lengths, e_starts)
        return got, trace, (e.value.code, str(e.value))
    with T.placement(gpu, stark, stark.config(), 16, env) as pr:
        before, trace_before, refusal_before = explicit(pr)
        pr.generate_trace_msms_complete(terms, lengths, masks)
        after, trace_after, refusal_after = explicit(pr)
    assert np.array_equal(before[4], MB.padded("g1", insts, 128)[0])
    for b, a in zip(before, after):
        assert np.array_equal(b, a)
    assert np.array_equal(trace_before, trace_after)
    assert refusal_before == refusal_after and refusal_before[0] == WITNESS and "instance 97 (segment 6)" in refusal_before[1]


def test_batch_forms(gpu):
    """300 G1 instances are 3 units: the proofs verify with the returned starts and effective terms, the sums are the host
    function's; a refused list leaves every slot null and the batch prover usable; then the two thin forms, one unit each."""
    terms, lengths, masks, want = CS.batch_recipe()
    bad_terms, bad_lengths = CS.unit_exhausted("g1")
    L = gpu.lib()
    with batch_prover(gpu, "g1", CHAIN2) as bp:
        stark = bp.stark
        cfg = stark.config()
        host = gpu.msm_batch_instances_complete(stark, terms, lengths, masks)
        out = (ctypes.c_void_p * 1)(1)                                 # a stale value the call must clear
        rc = L.sbn_batch_prover_prove_msm_batch_complete(bp._h, bad_terms.ctypes.data, None, bad_lengths.ctypes.data, len(bad_lengths), out,
                                                         None, None, None, None, None, None, None)
        assert rc == WITNESS and "segment 1" in L.sbn_last_error().decode() and out[0] is None
        proofs, *outs, ios = bp.prove_msms_complete(terms, lengths, masks)
        assert len(proofs) == 3 and np.array_equal(ios, host[0]) and outs[2].tolist() == want
        _same(outs, host)
        fin, sums, inf = gpu.verify_msms(stark, cfg, proofs, lengths, starts=outs[1], terms=outs[0])
        assert np.array_equal(sums, host[5]) and np.array_equal(inf, host[6]) and np.array_equal(fin, host[4])
        # sk G for five keys, one of them the identity: products straight from the sums
        g = gpu.generator(stark)
        points = np.tile(g, (5, 1))
        scalars = np.array([T.limbs(k, 8, 32) for k in (1, 3, T.R - 1, 12345, 7)], dtype=np.uint32)
        pinf = np.array([0, 0, 0, 0, 1], dtype=np.uint8)
        p1, products, flags, eff, starts = bp.prove_scalar_muls_complete(points, scalars, pinf)
        assert len(p1) == 1 and flags.tolist() == [0, 0, 0, 0, 1] and np.array_equal(products[0], g)
        _, want_products, _ = gpu.scalar_mul_instances(stark, points[:4], scalars[:4], gpu.start_candidate(stark, 0))
        assert np.array_equal(products[:4], want_products)
        gpu.verify_msms(stark, cfg, p1, np.ones(5, dtype=np.uint64), starts=starts, terms=eff)
        # m G + r H with m odd: one segment
        pedersen = np.concatenate([np.stack([g, gpu.start_candidate(stark, 5)]), np.array([T.limbs(k, 8, 32) for k in (9, 4)], dtype=np.uint32)], axis=1)
        p2, total, flag, eff, start = bp.prove_msm_complete(pedersen)
        assert len(p2) == 1 and flag == 0
        _, s2, i2 = gpu.verify_msms(stark, cfg, p2, [2], starts=start, terms=eff)
        assert np.array_equal(s2[0], total) and not i2.any()
