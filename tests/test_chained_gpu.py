"""GPU tests of sbn_prover_generate_trace_chained (run with `-m gpu` on the MI355X box): the chained call must leave the list
Python derives (tests/chained_lists.py), and the public inputs and trace rows of the explicit-list call on that list, word for
word, in every placement of the chains -- the offsets built on the device where the chains run there (G1 / G2 under
SBN_TRACEGEN_DEVICE_CHAIN 1 and 2, Fq12 / Fq12U64 by default), on the host pool elsewhere.  Then the proof of a chained G1 list,
the multi-scalar sum its last output carries, and the refusals, after which the prover holds no trace."""
import numpy as np
import pytest

import chained_lists as CL
import tracegen_edges as T
from test_tracegen_edges_gpu import FQ12_PLACEMENTS

pytestmark = pytest.mark.gpu
BAD_ARG, WITNESS = -1, -8
CURVE_PLACEMENTS = T.PLACEMENTS[:3]          # SBN_TRACEGEN_DEVICE_CHAIN 0, 1, 2
# smallest device sizes; fq12u64 at 64 instances (2^13 rows) as well: more than one wave of instances in the running product
CASES = ([("g1", 128, env) for env in CURVE_PLACEMENTS] + [("g2", 128, env) for env in CURVE_PLACEMENTS] + [("fq", 128, {})]
         + [("fq12", 16, env) for env in FQ12_PLACEMENTS] + [("fq12u64", 16, {}), ("fq12u64", 64, {})])


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


@pytest.fixture(scope="module")
def explicit(gpu):
    """(pi, trace) of generate_trace on the Python-derived explicit list, once per (table, count), on a prover of its own."""
    cache = {}

    def get(table, count):
        if (table, count) not in cache:
            _, _, insts, _ = CL.chained_list(table, count)
            stark = T.stark_class(gpu, table)(count)
            pr = gpu.Prover(stark, stark.config(), T.degree_bits(table, count))
            try:
                pi = pr.generate_trace(T.pack(table, insts))
                cache[(table, count)] = (pi, pr.read_trace())
            finally:
                pr.close()
        return cache[(table, count)]
    return get


def _id(case):
    table, count, env = case
    return f"{table}-{count}-" + ("default" if not env else "+".join(f"{k[4:].lower()}={v}" for k, v in env.items() if k != "SBN_EXPERIMENTAL"))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_chained_call_equals_the_explicit_call(gpu, explicit, case):
    table, count, env = case
    terms, start, insts, final = CL.chained_list(table, count)
    want_pi, want_trace = explicit(table, count)
    stark = T.stark_class(gpu, table)(count)
    with T.placement(gpu, stark, stark.config(), T.degree_bits(table, count), env) as pr:
        pi, ios = pr.generate_trace_chained(terms, start)
        got = pr.read_trace()
    bad = np.nonzero((ios != T.pack(table, insts)).any(axis=1))[0]
    assert bad.size == 0, ("ios", bad[:8].tolist())
    assert np.array_equal(pi, want_pi)
    bad = np.nonzero((got != want_trace).any(axis=1))[0]
    assert bad.size == 0, ("trace columns", bad[:8].tolist())
    assert T.outputs_from_pi(table, pi)[-1] == final


def test_g1_chained_proof_and_msm(gpu, O):
    """prove() after the chained call == prove() after the explicit call, word for word; the host verifiers accept it; the last
    output minus the generator is sum e_i x_i in Python."""
    xs, es, start, insts, final = CL.seeded_curve_list("g1")
    terms, sw = CL.terms_words("g1", xs, es), CL.value_words("g1", start)
    stark = gpu.G1ExpStark(128)
    cfg = stark.config()
    a, b = gpu.Prover(stark, cfg, 16), gpu.Prover(stark, cfg, 16)
    try:
        pi, ios = a.generate_trace_chained(terms, sw)
        assert np.array_equal(b.generate_trace(ios), pi)
        proof = a.prove()
        assert np.array_equal(proof.words, b.prove().words)
    finally:
        a.close()
        b.close()
    gpu.verify_stark_proof(stark, proof, cfg)
    assert O.verify(O.AIR_G1_EXP, 128, proof.words) == (0, "")
    msm = None
    for x, e in zip(xs, es):
        msm = O.g1_add(msm, O.g1_mul(x, e))
    assert O.g1_add(T.outputs_from_pi("g1", pi)[-1], T.g1_neg(start)) == msm


@pytest.mark.parametrize("curve,env", [("g1", env) for env in CURVE_PLACEMENTS] + [("g2", CURVE_PLACEMENTS[2])],
                         ids=lambda v: v if isinstance(v, str) else "chain=" + v["SBN_TRACEGEN_DEVICE_CHAIN"])
def test_refusals_leave_no_trace_loaded(gpu, curve, env):
    """The two SBN_ERR_WITNESS lists (an offset at infinity; an instance the table's own walk cannot take), a point off the curve
    and a coordinate >= p are refused as on the host; prove() then fails with SBN_ERR_BAD_ARG; the accepted twin generates
    Python's list and proves."""
    cases = CL.witness_refusals(curve)
    words = lambda name: (CL.terms_words(curve, cases[name][0], cases[name][1]), CL.value_words(curve, cases[name][2]))   # noqa: E731
    good_terms, good_start = words("twin")
    off_curve = good_terms.copy()
    off_curve[64, 0] ^= 1
    not_below_p = good_terms.copy()
    not_below_p[64, :8] = T.limbs(T.P, 8, 32)
    stark = T.stark_class(gpu, curve)(128)
    cfg = stark.config()
    with T.placement(gpu, stark, cfg, 16, env) as pr:
        for name, terms, code in (("opposite", words("opposite")[0], WITNESS), ("collide", words("collide")[0], WITNESS),
                                  ("off_curve", off_curve, BAD_ARG), ("not_below_p", not_below_p, BAD_ARG)):
            pr.generate_trace_chained(good_terms, good_start)        # a loaded trace that the refusal must drop
            with pytest.raises(gpu.SbnError) as e:
                pr.generate_trace_chained(terms, good_start)
            assert e.value.code == code, (name, str(e.value))
            with pytest.raises(gpu.SbnError) as e:
                pr.prove()
            assert e.value.code == BAD_ARG, name
        pi, ios = pr.generate_trace_chained(good_terms, good_start)
        insts, final = CL.derive(curve, *cases["twin"])
        assert np.array_equal(ios, T.pack(curve, insts))
        assert T.outputs_from_pi(curve, pi)[-1] == final
        proof = pr.prove()
    gpu.verify_stark_proof(stark, proof, cfg)
