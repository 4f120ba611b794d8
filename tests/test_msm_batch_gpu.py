"""GPU tests of the batches of short MSMs (run with `-m gpu` on the MI355X box): Prover.generate_trace_msms must leave the
segmented list Python derives (tests/msm_batches.py) and the public inputs and trace rows of the explicit-list call on that list,
word for word, in every placement of the chains -- the offsets, finals and sums built on the device where the chains run there
(G1 / G2 under SBN_TRACEGEN_DEVICE_CHAIN 1 and 2, Fq12 / Fq12U64 by default), on the host pool elsewhere.  Then the proof of a
segmented G1 unit, BatchProver.prove_msms / verify_msms on a list whose segments straddle the unit boundaries, and the refusals,
after which a prover holds no trace and a batch prover no proof."""
import ctypes
import re

import numpy as np
import pytest

import chained_lists as CL
import msm_batches as MB
import tracegen_edges as T
from test_msm_gpu import batch_prover
from test_tracegen_edges_gpu import FQ12_PLACEMENTS

pytestmark = pytest.mark.gpu
BAD_ARG, VERIFY_FAILED, WITNESS = -1, -6, -8
CURVE_PLACEMENTS = T.PLACEMENTS[:3]          # SBN_TRACEGEN_DEVICE_CHAIN 0, 1, 2
CHAIN2 = CURVE_PLACEMENTS[2]
# smallest device sizes; fq12u64 at 64 instances as well: nine segments, i.e. more workgroups than at 16; the shared default start
# where the derivation runs on the device
CASES = ([("g1", 128, env, False) for env in CURVE_PLACEMENTS] + [("g2", 128, env, False) for env in CURVE_PLACEMENTS]
         + [("g1", 128, CHAIN2, True), ("g2", 128, CHAIN2, True), ("fq", 128, {}, False)]
         + [("fq12", 16, env, False) for env in FQ12_PLACEMENTS] + [("fq12", 16, {}, True)]
         + [("fq12u64", 16, {}, False), ("fq12u64", 64, {}, False), ("fq12u64", 64, {}, True)])


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


def unit_case(table, num_io, shared):
    """(terms, lengths, starts_words or None, insts, finals, sums, ios) of the table's one-unit recipe; ios = Python's padded unit."""
    if table in ("g1", "g2"):
        xs, es, starts, insts, finals, sums = MB.curve_unit(table, shared)
        lengths = MB.CURVE_LENGTHS
    else:
        xs, es, starts, insts, finals = MB.field_unit(table, num_io, shared)
        lengths, sums = MB.field_lengths(num_io), None
    return (CL.terms_words(table, xs, es), MB.lengths_words(lengths), None if shared else MB.starts_words(table, starts), insts, finals, sums,
            MB.padded(table, insts, num_io)[0])


def assert_outputs(table, fin, sm, inf, finals, sums):
    assert np.array_equal(fin, MB.starts_words(table, finals))
    if table in ("g1", "g2"):
        assert np.array_equal(sm, MB.point_words(table, sums)) and np.array_equal(inf, MB.flags(sums))
    else:
        assert sm is None and inf is None


@pytest.fixture(scope="module")
def explicit(gpu):
    """(pi, trace) of generate_trace on Python's padded unit, once per (table, num_io, shared), on a prover of its own."""
    cache = {}

    def get(table, num_io, shared):
        key = (table, num_io, shared)
        if key not in cache:
            stark = T.stark_class(gpu, table)(num_io)
            pr = gpu.Prover(stark, stark.config(), T.degree_bits(table, num_io))
            try:
                pi = pr.generate_trace(unit_case(table, num_io, shared)[6])
                cache[key] = (pi, pr.read_trace())
            finally:
                pr.close()
        return cache[key]
    return get


def _id(case):
    table, num_io, env, shared = case
    place = "default" if not env else "+".join(f"{k[4:].lower()}={v}" for k, v in env.items() if k != "SBN_EXPERIMENTAL")
    return f"{table}-{num_io}-{place}-" + ("one_start" if shared else "starts")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_segmented_call_equals_the_explicit_call(gpu, explicit, case):
    table, num_io, env, shared = case
    terms, lengths, starts, insts, finals, sums, want_ios = unit_case(table, num_io, shared)
    want_pi, want_trace = explicit(table, num_io, shared)
    stark = T.stark_class(gpu, table)(num_io)
    with T.placement(gpu, stark, stark.config(), T.degree_bits(table, num_io), env) as pr:
        pi, fin, sm, inf, ios = pr.generate_trace_msms(terms, lengths, starts)
        got = pr.read_trace()
    bad = np.nonzero((ios != want_ios).any(axis=1))[0]
    assert bad.size == 0, ("ios", bad[:8].tolist())
    assert np.array_equal(pi, want_pi)
    bad = np.nonzero((got != want_trace).any(axis=1))[0]
    assert bad.size == 0, ("trace columns", bad[:8].tolist())
    assert_outputs(table, fin, sm, inf, finals, sums)
    outs = T.outputs_from_pi(table, pi)
    hs = MB.heads([int(n) for n in lengths])
    assert [outs[h + int(n) - 1] for h, n in zip(hs, lengths)] == finals
    assert all(o == outs[len(insts) - 1] for o in outs[len(insts):])       # the pads repeat the last real instance


def test_g1_segmented_proof(gpu, O):
    """prove() after the segmented call == prove() after the explicit call, word for word; the host verifier and the oracle
    verifier accept it."""
    terms, lengths, starts, _, _, _, want_ios = unit_case("g1", 128, False)
    stark = gpu.G1ExpStark(128)
    cfg = stark.config()
    a, b = gpu.Prover(stark, cfg, 16), gpu.Prover(stark, cfg, 16)
    try:
        pi, _, _, _, ios = a.generate_trace_msms(terms, lengths, starts)
        assert np.array_equal(ios, want_ios) and np.array_equal(b.generate_trace(ios), pi)
        proof = a.prove()
        assert np.array_equal(proof.words, b.prove().words)
    finally:
        a.close()
        b.close()
    gpu.verify_stark_proof(stark, proof, cfg)
    assert O.verify(O.AIR_G1_EXP, 128, proof.words) == (0, "")


@pytest.mark.parametrize("table,env", [("g1", CHAIN2), ("fq12", {})], ids=["g1-chain=2", "fq12-default"])
def test_prove_msms_equals_prove_ios_and_verifies(gpu, table, env):
    """The 300-term (37-term) recipe: a segment across each unit boundary, the last unit padded.  The unit proofs equal prove_ios
    on Python's units; verify_msms accepts on the host and on a Verifier(max_batch=4); a broken unit and swapped units are refused,
    naming them."""
    num_io, lengths, xs, es, starts, insts, finals, sums = MB.batch_list(table)
    terms, lw, sw = CL.terms_words(table, xs, es), MB.lengths_words(lengths), MB.starts_words(table, starts)
    units = MB.padded(table, insts, num_io)
    with batch_prover(gpu, table, env) as bp:
        proofs, fin, sm, inf, ios = bp.prove_msms(terms, lw, sw)
        want = bp.prove_ios(units)
    assert np.array_equal(ios, units) and len(proofs) == 3
    assert_outputs(table, fin, sm, inf, finals, sums)
    for u, (p, w) in enumerate(zip(proofs, want)):
        assert np.array_equal(p.words, w.words), f"unit {u}"
    stark = bp.stark
    cfg = stark.config()
    broken = gpu.Proof(proofs[1].words.copy(), proofs[1].degree_bits)
    broken.words[40] ^= 1
    ver = gpu.Verifier(stark, cfg, T.degree_bits(table, num_io), max_batch=4)
    try:
        for v in (None, ver):
            assert_outputs(table, *gpu.verify_msms(stark, cfg, proofs, lw, sw, terms, verifier=v), finals, sums)
            with pytest.raises(gpu.SbnError) as e:
                gpu.verify_msms(stark, cfg, [proofs[0], broken, proofs[2]], lw, sw, terms, verifier=v)
            assert e.value.code == VERIFY_FAILED and "unit 1" in str(e.value), str(e.value)
            with pytest.raises(gpu.SbnError) as e:
                gpu.verify_msms(stark, cfg, [proofs[1], proofs[0], proofs[2]], lw, sw, verifier=v)
            assert e.value.code == VERIFY_FAILED and "instance 0 (segment 0)" in str(e.value), str(e.value)
    finally:
        ver.close()


def _refusals(curve):
    """[(name, terms, code, pattern)], the good terms, lengths, starts and Python's list of the good terms."""
    cases, starts = MB.refusal_lists(curve)
    words = lambda name: CL.terms_words(curve, *cases[name])   # noqa: E731
    good = words("twin")
    off_curve = good.copy()
    off_curve[70, 0] ^= 1
    not_below_p = good.copy()
    not_below_p[99, :8] = T.limbs(T.P, 8, 32)
    bad = [("infinity", words("infinity"), WITNESS, r"offset of instance 65 \(segment 5\).*infinity"),
           ("collide", words("collide"), WITNESS, r"instance 97 \(segment 6\).*degenerate"),
           ("off_curve", off_curve, BAD_ARG, r"instance 70 \(segment 5\)"), ("not_below_p", not_below_p, BAD_ARG, r"instance 99, segment 6")]
    insts, finals = MB.derive(curve, *cases["twin"], MB.CURVE_LENGTHS, starts)
    return bad, good, MB.lengths_words(MB.CURVE_LENGTHS), MB.starts_words(curve, starts), starts, insts, finals


@pytest.mark.parametrize("curve,env", [("g1", env) for env in CURVE_PLACEMENTS] + [("g2", CHAIN2)],
                         ids=lambda v: v if isinstance(v, str) else "chain=" + v["SBN_TRACEGEN_DEVICE_CHAIN"])
def test_refusals_leave_no_trace_loaded(gpu, curve, env):
    """An offset at infinity in segment 5 only, a head the table's own walk cannot take, a point off the curve and a coordinate
    >= p are refused with the codes and names of the host call; prove() then fails with SBN_ERR_BAD_ARG; the accepted twin
    generates Python's list and proves.  Every refusal is an error return: the host checks or the kernels' error word."""
    bad, good, lengths, sw, starts, insts, finals = _refusals(curve)
    stark = T.stark_class(gpu, curve)(128)
    cfg = stark.config()
    with T.placement(gpu, stark, cfg, 16, env) as pr:
        for name, terms, code, pattern in bad:
            pr.generate_trace_msms(good, lengths, sw)                # a loaded trace that the refusal must drop
            with pytest.raises(gpu.SbnError) as e:
                pr.generate_trace_msms(terms, lengths, sw)
            assert e.value.code == code and re.search(pattern, str(e.value)), (name, str(e.value))
            with pytest.raises(gpu.SbnError) as e:
                pr.prove()
            assert e.value.code == BAD_ARG, name
        pi, fin, sm, inf, ios = pr.generate_trace_msms(good, lengths, sw)
        assert np.array_equal(ios, MB.padded(curve, insts, 128)[0])
        assert_outputs(curve, fin, sm, inf, finals, MB.sums_of(curve, finals, starts))
        proof = pr.prove()
    gpu.verify_stark_proof(stark, proof, cfg)


def test_refused_batch_leaves_every_slot_null_and_the_batch_prover_usable(gpu):
    bad, good, lengths, sw, starts, insts, finals = _refusals("g1")
    L = gpu.lib()
    with batch_prover(gpu, "g1", CHAIN2) as bp:
        for name, terms, code, pattern in bad:
            out = (ctypes.c_void_p * 1)(1)               # a stale value the call must clear
            rc = L.sbn_batch_prover_prove_msm_batch(bp._h, terms.ctypes.data, lengths.ctypes.data, len(lengths), sw.ctypes.data, len(lengths), out,
                                                    None, None, None, None)
            msg = L.sbn_last_error().decode()
            assert rc == code and re.search(pattern, msg), (name, rc, msg)
            assert out[0] is None, name
        proofs, fin, sm, inf, ios = bp.prove_msms(good, lengths, sw)
        want = bp.prove_ios(MB.padded("g1", insts, 128))
    assert len(proofs) == 1 and np.array_equal(proofs[0].words, want[0].words)
    assert_outputs("g1", fin, sm, inf, finals, MB.sums_of("g1", finals, starts))
