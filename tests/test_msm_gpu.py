"""GPU tests of BatchProver.prove_msm / verify_msm (run with `-m gpu` on the MI355X box): a chained list of two full units and a
partial one (tests/msm_lists.py) proved as units of one table must give Python's padded list and last output, and, unit by unit,
the proof words of prove_ios on the Python-derived explicit units, in every placement of the table's chains; the unit proofs verify
and link up; a refused list leaves the batch prover usable."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest

import chained_lists as CL
import msm_lists as ML
import tracegen_edges as T
from test_tracegen_edges_gpu import FQ12_PLACEMENTS

pytestmark = pytest.mark.gpu
BAD_ARG, VERIFY_FAILED, WITNESS = -1, -6, -8
CHAIN = [{"SBN_TRACEGEN_DEVICE_CHAIN": m} for m in "012"]
CASES = ([("g1", env) for env in CHAIN] + [("g2", CHAIN[2]), ("fq", {})] + [("fq12", env) for env in FQ12_PLACEMENTS] + [("fq12u64", {})])


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


@contextlib.contextmanager
def batch_prover(gpu, table, env, inflight=2):
    """A BatchProver of the table's smallest size created under the switches `env` (restored afterwards), closed on exit."""
    num_io = ML.SIZES[table][0]
    stark = T.stark_class(gpu, table)(num_io)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        bp = gpu.BatchProver(stark, stark.config(), T.degree_bits(table, num_io), inflight=inflight)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        yield bp
    finally:
        bp.close()


@pytest.fixture(scope="module")
def explicit(gpu):
    """The proof words of prove_ios on the Python-derived explicit units, once per table, from a batch prover in the default
    placement."""
    cache = {}

    def get(table):
        if table not in cache:
            with batch_prover(gpu, table, {}) as bp:
                cache[table] = [p.words for p in bp.prove_ios(ML.msm_list(table)[4])]
        return cache[table]
    return get


def _same_words(proofs, want):
    assert len(proofs) == len(want)
    for u, (p, w) in enumerate(zip(proofs, want)):
        assert np.array_equal(p.words, w), f"unit {u}"


def _id(case):
    table, env = case
    return f"{table}-" + ("default" if not env else "+".join(f"{k[4:].lower()}={v}" for k, v in env.items() if k != "SBN_EXPERIMENTAL"))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_prove_msm_equals_prove_ios_on_the_python_list(gpu, O, explicit, case):
    table, env = case
    num_io, count = ML.SIZES[table]
    terms, start, _, final, units = ML.msm_list(table)
    with batch_prover(gpu, table, env) as bp:
        proofs, fin, ios = bp.prove_msm(terms, start)
    assert np.array_equal(ios, units)
    assert np.array_equal(fin, CL.value_words(table, final))
    _same_words(proofs, explicit(table))
    stark = bp.stark
    assert np.array_equal(gpu.verify_msm(stark, stark.config(), proofs, count, start, terms), fin)
    assert np.array_equal(gpu.verify_msm(stark, stark.config(), proofs, count, start), fin)
    assert T.outputs_from_pi(table, proofs[2].public_inputs())[count - 1 - 2 * num_io] == final
    if table == "g1":
        assert O.verify(O.AIR_G1_EXP, num_io, proofs[2].words) == (0, "")   # the padded unit


@pytest.mark.parametrize("inflight", [1, 4])
def test_g1_no_concurrency_and_more_contexts_than_units(gpu, explicit, inflight):
    terms, start, _, final, units = ML.msm_list("g1")
    with batch_prover(gpu, "g1", CHAIN[2], inflight=inflight) as bp:
        proofs, fin, ios = bp.prove_msm(terms, start)
    assert np.array_equal(ios, units) and np.array_equal(fin, CL.value_words("g1", final))
    _same_words(proofs, explicit("g1"))


@pytest.mark.parametrize("table,env", [("g1", CHAIN[2]), ("fq12", {})], ids=["g1-chain=2", "fq12-default"])
def test_refusals_leave_the_batch_prover_usable(gpu, explicit, table, env):
    """Error returns, not faults: a carry at infinity on the unit boundary (G1) and a coordinate >= p in unit 2 are refused with
    every proof slot empty; the same batch prover then proves the good list with the same words."""
    num_io, count = ML.SIZES[table]
    terms, start, _, _, _ = ML.msm_list(table)
    not_below_p = terms.copy()
    not_below_p[2 * num_io + 1, 8:16] = T.limbs(T.P, 8, 32)
    bad = [("not_below_p", not_below_p, BAD_ARG, rf"instance {2 * num_io + 1}\b")]
    if table == "g1":
        bad.insert(0, ("boundary_infinity", ML.boundary_infinity("g1")[0], WITNESS, rf"infinity.*instance {num_io}\b|instance {num_io}\b.*infinity"))
    L = gpu.lib()
    with batch_prover(gpu, table, env) as bp:
        for name, t, code, names in bad:
            out = (ctypes.c_void_p * 3)(1, 1, 1)     # stale values the call must clear
            rc = L.sbn_batch_prover_prove_msm(bp._h, t.ctypes.data, count, start.ctypes.data, out, None, None)
            msg = L.sbn_last_error().decode()
            assert rc == code and re.search(names, msg), (name, rc, msg)
            assert [out[u] for u in range(3)] == [None] * 3, name
            proofs, _, _ = bp.prove_msm(terms, start)
            _same_words(proofs, explicit(table))


def test_verify_msm_on_the_device_verifier(gpu, explicit):
    """verify_msm with a Verifier(max_batch=4) gives the host verifier's verdicts: the good list, a unit whose proof is broken,
    and good proofs in the wrong order (every unit verifies, the links do not)."""
    table = "fq12"
    num_io, count = ML.SIZES[table]
    terms, start, _, final, _ = ML.msm_list(table)
    stark = T.stark_class(gpu, table)(num_io)
    cfg = stark.config()
    proofs = [gpu.Proof(w, T.degree_bits(table, num_io)) for w in explicit(table)]
    broken = gpu.Proof(proofs[1].words.copy(), proofs[1].degree_bits)
    broken.words[40] ^= 1
    ver = gpu.Verifier(stark, cfg, T.degree_bits(table, num_io), max_batch=4)
    try:
        for v in (None, ver):
            assert np.array_equal(gpu.verify_msm(stark, cfg, proofs, count, start, terms, verifier=v), CL.value_words(table, final))
            with pytest.raises(gpu.SbnError) as e:
                gpu.verify_msm(stark, cfg, [proofs[0], broken, proofs[2]], count, start, terms, verifier=v)
            assert e.value.code == VERIFY_FAILED and "unit 1" in str(e.value), str(e.value)
            with pytest.raises(gpu.SbnError) as e:
                gpu.verify_msm(stark, cfg, [proofs[1], proofs[0], proofs[2]], count, start, terms, verifier=v)
            assert e.value.code == VERIFY_FAILED and "instance 0:" in str(e.value), str(e.value)
    finally:
        ver.close()
