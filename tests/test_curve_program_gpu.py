"""GPU tests of the curve programs (run with `-m gpu` on the MI355X box), on G1ExpStark(128) and G2ExpStark(128), one unit each:
the smallest height the curve tables exist at.  The yardstick is the code that was there before: Prover.generate_trace and
BatchProver.prove_ios on the explicit list sbn_curve_program_instances derives on the host, itself held against Python in
tests/test_curve_program_host.py.  generate_trace_curve_program must return that list, its public inputs, outputs, values, flags
and choice, and prove to the same words, in every placement of the curve chains: 1 and 2 resolve the links on the device, one
launch per level, 0 derives on the host pool.  A program whose candidate 0 meets a bad event goes through the status word and
the host fallback; a refused call leaves no trace loaded and the prover usable; prove_curve_program gives proofs that
verify_curve_program accepts, and rejects with two units swapped.  Programs have at most 128 nodes and 3 levels."""
import numpy as np
import pytest

import curve_programs as G
import tracegen_edges as T

pytestmark = pytest.mark.gpu
BAD_ARG, VERIFY_FAILED, WITNESS = -1, -6, -8
PLACEMENTS = T.PLACEMENTS[:3]                                                # SBN_TRACEGEN_DEVICE_CHAIN = 0, 1, 2


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


def _five_nodes(curve):
    """5 nodes, 123 pads; the last node is linked in x and offset, so the pads copy derived words."""
    nodes, points, exps = G.cases(curve)["lincomb"]
    return nodes[:4] + [(G.out(1), G.out(3), 4)], points, exps


PROGRAMS = {
    "diamond": lambda c: G.cases(c)["diamond"],
    "tower": lambda c: G.cases(c)["tower"],
    "independent_128": lambda c: G.independent(c, 128),
    "five_nodes": _five_nodes,
    "narrow_waist": G.narrow_waist,
}
DEPTH = {"diamond": 3, "tower": 3, "independent_128": 1, "five_nodes": 3, "narrow_waist": 3}


def _same(got, want, env):
    """(pi, outs, values, infinity, choice, ios) of generate_trace_curve_program against the host derivation and its public inputs."""
    ios, outs, values, infinity, choice = want[:5]
    assert np.array_equal(got[0], want[5]), env
    assert np.array_equal(got[1], outs) and np.array_equal(got[2], values) and np.array_equal(got[3], infinity) and got[4] == choice, env
    assert np.array_equal(got[5], ios[0]), env


def _explicit(gpu, curve, arr):
    """The host derivation of a one-unit program, and the public inputs and proof words of the explicit path on a prover of its own."""
    stark = T.stark_class(gpu, curve)(128)
    cfg = stark.config()
    want = gpu.curve_program_instances(stark, *arr)
    assert want[0].shape[0] == 1
    with T.placement(gpu, stark, cfg, 16, {}) as ref:
        pi = ref.generate_trace(want[0][0])
        words = ref.prove().words
    return stark, cfg, want + (pi,), words


@pytest.mark.parametrize("name", list(PROGRAMS))
@pytest.mark.parametrize("curve", G.CURVES)
def test_programs_equal_the_explicit_list_in_every_placement(gpu, curve, name):
    prog = PROGRAMS[name](curve)
    assert G.levels(prog[0])[1] == DEPTH[name] and len(prog[0]) <= 128
    arr = G.arrays(curve, *prog)
    stark, cfg, want, words = _explicit(gpu, curve, arr)
    assert want[4] == 0
    for env in PLACEMENTS:
        with T.placement(gpu, stark, cfg, 16, env) as pr:
            _same(pr.generate_trace_curve_program(*arr), want, env)
            assert np.array_equal(pr.prove().words, words), env
    if name == "diamond":
        gpu.verify_stark_proof(stark, gpu.Proof(words, 16), cfg)
        values, infinity = gpu.verify_curve_program(stark, cfg, [gpu.Proof(words, 16)], *arr, 0)
        assert np.array_equal(values, want[2]) and not infinity.any()


@pytest.mark.parametrize("curve", G.CURVES)
def test_a_bad_event_under_candidate_0_falls_back_to_the_host_derivation(gpu, curve):
    """The choice = 1 program of the host tests: on the device candidate 0 sets the status word, the host derivation walks on to
    candidate 1 and the explicit path loads its list; the words are the model's, and the prover is usable afterwards."""
    prog = G.killing(curve, 1)
    arr = G.arrays(curve, *prog)
    ios, outs, values, infinity, choice = G.model(curve, *prog, 128)
    assert choice == 1
    stark, cfg, want, words = _explicit(gpu, curve, arr)
    assert all(np.array_equal(a, b) for a, b in zip(want[:4], (ios, outs, values, infinity))) and want[4] == 1
    benign = G.arrays(curve, *G.cases(curve)["diamond"])
    for env in PLACEMENTS:
        with T.placement(gpu, stark, cfg, 16, env) as pr:
            _same(pr.generate_trace_curve_program(*arr), want, env)
            assert np.array_equal(pr.prove().words, words), env
            assert pr.generate_trace_curve_program(*benign)[4] == 0          # the next call starts from candidate 0 again
            pr.prove()


EXPLICIT_STAGES = ["flags+pulses", "chains", "affine+lambda", "row_witness", "range_check", "total"]
DEVICE_STAGES = ["curve_program_levels", "flags+pulses", "affine+lambda", "curve_program_values", "row_witness", "range_check", "total"]


@pytest.mark.parametrize("mode", ["1", "2"])
def test_the_stage_lines_tell_the_device_route_from_the_fallback(gpu, capfd, mode):
    """Under SBN_TRACE_TIMING a benign program prints the spans of the device route (no `chains` span: the level launches walked
    them), the choice = 1 program the abandoned level span and then the stages of the explicit path; placement 0 only those."""
    stark = gpu.G1ExpStark(128)
    benign = G.arrays("g1", *G.cases("g1")["diamond"])
    crafted = G.arrays("g1", *G.killing("g1", 1))

    def stages(pr, arr):
        capfd.readouterr()
        choice = pr.generate_trace_curve_program(*arr)[4]
        return choice, [ln.split()[2] for ln in capfd.readouterr().err.splitlines() if ln.startswith("[device tracegen]")]
    with T.placement(gpu, stark, stark.config(), 16, {"SBN_TRACE_TIMING": "1", "SBN_TRACEGEN_DEVICE_CHAIN": mode}) as pr:
        assert stages(pr, benign) == (0, DEVICE_STAGES)
        assert stages(pr, crafted) == (1, ["curve_program_levels", "total"] + EXPLICIT_STAGES)
    if mode == "1":
        with T.placement(gpu, stark, stark.config(), 16, {"SBN_TRACE_TIMING": "1", "SBN_TRACEGEN_DEVICE_CHAIN": "0"}) as pr:
            assert stages(pr, benign) == (0, EXPLICIT_STAGES)


@pytest.mark.parametrize("curve", G.CURVES)
def test_a_refused_call_leaves_no_trace_loaded_and_the_prover_usable(gpu, curve):
    stark = T.stark_class(gpu, curve)(128)
    cfg = stark.config()
    n, p, e = G.arrays(curve, *G.cases(curve)["diamond"])
    too_many = np.array([(0, G.START, 0)] * 129, dtype=np.uint32)
    forward = n.copy()
    forward[2, 0] = G.out(2)
    start_as_x = n.copy()
    start_as_x[1, 0] = G.START
    off_curve = p.copy()
    off_curve[1, 0] ^= 1
    exhausting = G.arrays(curve, *G.killing(curve, 8))
    for env in PLACEMENTS[1:]:
        with T.placement(gpu, stark, cfg, 16, env) as pr:
            got = pr.generate_trace_curve_program(n, p, e)
            want = pr.prove().words
            for bad_call, code, names in ((lambda: pr.generate_trace_curve_program(too_many, p, e), BAD_ARG, "129 nodes"),
                                          (lambda: pr.generate_trace_curve_program(forward, p, e), BAD_ARG, "node 2: x links to node 2"),
                                          (lambda: pr.generate_trace_curve_program(start_as_x, p, e), BAD_ARG, "node 1: x is SBN_NODE_START"),
                                          (lambda: pr.generate_trace_curve_program(n, off_curve, e), BAD_ARG, "literal 1 is not a point"),
                                          (lambda: pr.generate_trace_curve_program(*exhausting), WITNESS, "candidate 7 fails at node 8")):
                with pytest.raises(gpu.SbnError) as err:
                    bad_call()
                assert err.value.code == code and names in str(err.value), str(err.value)
                with pytest.raises(gpu.SbnError) as err:
                    pr.prove()
                assert err.value.code == BAD_ARG                             # no trace is loaded
                again = pr.generate_trace_curve_program(n, p, e)
                assert all(np.array_equal(a, b) for a, b in zip(again, got))
            assert np.array_equal(pr.prove().words, want)


def test_prove_curve_program_verifies_and_two_swapped_units_do_not(gpu):
    """BatchProver on G1ExpStark(128): 300 nodes in 3 units, links across both boundaries, 84 pads; the values are the model's."""
    prog = G.wide("g1", 300)
    arr = G.arrays("g1", *prog)
    ios, outs, values, infinity, choice = G.model("g1", *prog, 128)
    stark = gpu.G1ExpStark(128)
    cfg = stark.config()
    bp = gpu.BatchProver(stark, cfg, 16, inflight=2)
    try:
        proofs, outs_got, values_got, infinity_got, choice_got, ios_got = bp.prove_curve_program(*arr)
        assert len(proofs) == 3 and choice_got == choice == 0
        assert np.array_equal(ios_got, ios) and np.array_equal(outs_got, outs) and np.array_equal(values_got, values) and np.array_equal(infinity_got, infinity)
        got = gpu.verify_curve_program(stark, cfg, proofs, *arr, choice)
        assert np.array_equal(got[0], values) and np.array_equal(got[1], infinity)
        with pytest.raises(gpu.SbnError) as e:                               # every proof verifies, a link does not
            gpu.verify_curve_program(stark, cfg, [proofs[0], proofs[2], proofs[1]], *arr, choice)
        assert e.value.code == VERIFY_FAILED and "instance 128:" in str(e.value), str(e.value)
        bad = arr[0].copy()                                                  # a refused list leaves every proof null and the batch prover usable
        bad[5, 1] = G.out(5)
        with pytest.raises(gpu.SbnError) as e:
            bp.prove_curve_program(bad, arr[1], arr[2])
        assert e.value.code == BAD_ARG and "node 5: offset links to node 5" in str(e.value), str(e.value)
        assert len(bp.prove_curve_program(*G.arrays("g1", *G.cases("g1")["diamond"]))[0]) == 1
    finally:
        bp.close()
