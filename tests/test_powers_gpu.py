"""GPU tests of the field powers and power towers (run with `-m gpu` on the MI355X box).  The yardstick is the code that was there
before: the host generators (generate_trace_and_public_inputs), Prover.generate_trace and BatchProver.prove_ios on the explicit
list sbn_power_instances derives on the host, itself held against Python in tests/test_powers_host.py.  generate_trace_powers must
load that trace word for word -- on the Fq12 tables the towers are linked, walked and padded on the device --, return the same
public inputs, list and powers, and prove to the same words; prove_powers / prove_bn_x_powers give the proofs of prove_ios on the
units; a refused call leaves no trace loaded and the prover usable.  Shapes: the smallest that reach every path (one pad, fifteen
pads, no pad; a whole unit as one tower; towers across unit boundaries; the host-walked placements)."""
import numpy as np
import pytest

import power_lists as PL
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


def _fq12_bases(seed, count, zero_at=None):
    r = PL.rng(seed)
    bases = [PL.random_elem("fq12", r) for _ in range(count)]
    if zero_at is not None:
        bases[zero_at] = [0] * 12
    return PL.base_words("fq12", bases)


def _same_trace(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, bad[:8].tolist()


def _compare_with_the_explicit_list(gpu, table, num_io, bases, exps, depth, envs=({},), prove=False):
    """generate_trace_powers against the host generator's trace and public inputs on the host-derived list, in every placement of
    `envs`; with prove, the proof words against prove() after generate_trace(ios) on that list.  Returns (proof, powers)."""
    stark = T.stark_class(gpu, table)(num_io)
    cfg = stark.config()
    bits = T.degree_bits(table, num_io)
    ios, powers_want = gpu.power_instances(stark, bases, exps, depth)
    assert ios.shape[0] == 1
    trace_want, pi_want = stark.generate_trace_and_public_inputs(ios[0])
    proof = None
    for env in envs:
        with T.placement(gpu, stark, cfg, bits, env) as pr:
            pi, powers, ios_got = pr.generate_trace_powers(bases, exps, depth)
            assert np.array_equal(ios_got, ios[0]) and np.array_equal(pi, pi_want), env
            assert np.array_equal(powers, powers_want), env
            _same_trace(pr.read_trace(), trace_want)
            if prove:
                proof = pr.prove()
                assert np.array_equal(pr.generate_trace(ios[0]), pi_want)
                assert np.array_equal(pr.prove().words, proof.words)
    return proof, powers_want


def test_bn_x_towers_on_fq12_u64_equal_the_explicit_list_and_prove(gpu):
    """Fq12ExpU64Stark(16), 2^11 rows: 5 towers of depth 3 with the shared BN parameter, 15 instances and one pad."""
    bases = _fq12_bases(1, 5)
    proof, powers = _compare_with_the_explicit_list(gpu, "fq12u64", 16, bases, gpu.BN_X, 3, prove=True)
    stark = gpu.Fq12ExpU64Stark(16)
    assert np.array_equal(gpu.verify_powers(stark, stark.config(), [proof], bases, gpu.BN_X, 3), powers)
    assert np.array_equal(gpu.verify_bn_x_powers(stark, stark.config(), [proof], bases), powers)


def test_towers_on_fq12_u64_under_the_host_chain_switch(gpu):
    """The same words where the towers are walked on the host pool: per-tower exponents, depth 2, two pads."""
    exps = PL.exp_words("fq12u64", [0, 1, PL.GLP - 1, gpu.BN_X, 2, 1 << 63, 3])
    _compare_with_the_explicit_list(gpu, "fq12u64", 16, _fq12_bases(2, 7, zero_at=4), exps, 2, envs=(HOST_CHAIN, {}))


FQ12_EXPS = [0, (1 << 256) - 1, 1, 2, P - 2] + [PL.rng(7).randrange(1 << 256) for _ in range(11)]


@pytest.mark.parametrize("case", ["sixteen_independent", "one_tower_of_sixteen", "one_power_fifteen_pads"])
def test_fq12_powers_equal_the_explicit_list(gpu, case):
    """Fq12ExpStark(16), 2^13 rows."""
    if case == "sixteen_independent":          # depth 1, per-instance exponents with 0 and 2^256 - 1, a zero base
        args = (_fq12_bases(3, 16, zero_at=2), PL.exp_words("fq12", FQ12_EXPS), 1)
    elif case == "one_tower_of_sixteen":       # the whole unit sequential, no pad
        args = (_fq12_bases(4, 1), PL.exp_words("fq12", FQ12_EXPS[5:6]), 16)
    else:                                      # one instance, fifteen pads filled on the device
        args = (_fq12_bases(5, 1), PL.exp_words("fq12", FQ12_EXPS[6:7]), 1)
    _compare_with_the_explicit_list(gpu, "fq12", 16, *args)


def test_fq_towers_and_square_roots_equal_the_explicit_list(gpu):
    """FqExpStark(128), 2^16 rows, the table's minimum: 42 towers of depth 3 and 2 pads; then 100 square roots and 28 pads."""
    r = PL.rng(6)
    bases = [0, 1, P - 1] + [r.randrange(P) for _ in range(39)]
    exps = PL.exp_words("fq", [0, (1 << 256) - 1] + [r.randrange(1 << 256) for _ in range(40)])
    _compare_with_the_explicit_list(gpu, "fq", 128, PL.base_words("fq", bases), exps, 3)
    xs = [r.randrange(P) for _ in range(100)]
    _, roots = _compare_with_the_explicit_list(gpu, "fq", 128, PL.base_words("fq", xs), gpu.FQ_SQRT_EXP, 1)
    assert [PL.from_limbs(w) for w in roots[:, 0]] == [pow(x, (P + 1) // 4, P) for x in xs]
    flags = gpu.fq_sqrt_flags(xs, roots[:, 0])
    assert flags.tolist() == [pow(x, (P - 1) // 2, P) in (0, 1) for x in xs] and flags.any() and not flags.all()


def test_prove_bn_x_powers_equals_prove_ios_and_verifies(gpu):
    """BatchProver on Fq12ExpU64Stark(4), 2^9 rows: 3 inputs = 9 instances in 3 units, towers across the unit boundaries."""
    fs = _fq12_bases(8, 3)
    stark = gpu.Fq12ExpU64Stark(4)
    cfg = stark.config()
    units, powers_want = gpu.power_instances(stark, fs, gpu.BN_X, 3)
    assert units.shape == (3, 4, 194)
    bp = gpu.BatchProver(stark, cfg, 9, inflight=2)
    try:
        want = [p.words for p in bp.prove_ios(units)]
        proofs, powers, ios = bp.prove_bn_x_powers(fs)
        assert np.array_equal(ios, units) and np.array_equal(powers, powers_want)
        _same_words(proofs, want)
        got = gpu.verify_bn_x_powers(stark, cfg, proofs, fs)
        assert got.shape == (3, 3, 96) and np.array_equal(got, powers_want)
        # one edited public-input word (the output of instance 5, which instance 6 does not read: only the proof can tell)
        broken = gpu.Proof(proofs[1].words.copy(), 9)
        per = stark.num_public_inputs // 4
        broken.words[len(broken.words) - stark.num_public_inputs + 2 * per - 1] ^= 1
        with pytest.raises(gpu.SbnError) as e:
            gpu.verify_bn_x_powers(stark, cfg, [proofs[0], broken, proofs[2]], fs)
        assert e.value.code == VERIFY_FAILED and "unit 1" in str(e.value), str(e.value)
        # a refused list (a coefficient >= p in input 1) leaves every proof null and the batch prover usable
        bad = fs.copy()
        bad[1, 8:16] = PL.limbs(P, 8)
        with pytest.raises(gpu.SbnError) as e:
            bp.prove_bn_x_powers(bad)
        assert e.value.code == BAD_ARG and "tower 1" in str(e.value), str(e.value)
        _same_words(bp.prove_bn_x_powers(fs)[0], want)
    finally:
        bp.close()
    f12 = gpu.Fq12ExpStark(16)
    b12 = gpu.BatchProver(f12, f12.config(), 13, inflight=1)
    try:
        with pytest.raises(gpu.SbnError) as e:                               # the BN-parameter powers are a call of the u64 table
            b12.prove_bn_x_powers(fs)
        assert e.value.code == BAD_ARG
    finally:
        b12.close()


def test_a_refused_call_leaves_no_trace_loaded_and_the_prover_usable(gpu):
    stark = gpu.Fq12ExpU64Stark(16)
    cfg = stark.config()
    bases = _fq12_bases(9, 6)
    with T.placement(gpu, stark, cfg, 11, {}) as pr:
        pi, powers, _ = pr.generate_trace_powers(bases[:5], gpu.BN_X, 3)
        want = pr.prove().words
        for bad_call, code in ((lambda: pr.generate_trace_powers(bases, gpu.BN_X, 3), BAD_ARG),            # 18 instances > 16
                               (lambda: pr.generate_trace_powers(_too_big(bases[:5]), gpu.BN_X, 3), BAD_ARG),
                               (lambda: pr.generate_trace_powers(bases[:5], PL.GLP, 3), NON_CANONICAL)):
            with pytest.raises(gpu.SbnError) as e:
                bad_call()
            assert e.value.code == code, str(e.value)
            with pytest.raises(gpu.SbnError) as e:
                pr.prove()
            assert e.value.code == BAD_ARG                                   # no trace is loaded
            pi2, powers2, _ = pr.generate_trace_powers(bases[:5], gpu.BN_X, 3)
            assert np.array_equal(pi2, pi) and np.array_equal(powers2, powers)
        assert np.array_equal(pr.prove().words, want)
        gpu.verify_stark_proof(stark, gpu.Proof(want, 11), cfg)


def _too_big(bases):
    bad = bases.copy()
    bad[3, 40:48] = PL.limbs(P, 8)
    return bad
