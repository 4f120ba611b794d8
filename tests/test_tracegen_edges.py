"""CPU tests of the witness generators at edge inputs (tests/tracegen_edges.py): the product's host generator against the C++ oracle
and against Python integers on edge-case instance lists of all five Exp tables; degenerate curve instances refused and their
control twins accepted; and the BN254 field helpers of the device witness (host build) against Python's % and pow."""
import ctypes as C

import numpy as np
import pytest

import tracegen_edges as T

TABLES = ["g1", "g2", "fq", "fq12", "fq12u64"]


def _lists():
    return [(t, "edges") for t in TABLES] + [("g1", "identical"), ("fq", "identical")]


@pytest.fixture(scope="module", params=_lists(), ids=lambda p: f"{p[0]}-{p[1]}")
def edge_case(request, O):
    table, kind = request.param
    ios, insts = T.edge_list(table) if kind == "edges" else T.identical_list(table)
    trace, pi = T.oracle_trace(table, ios)
    return table, ios, insts, trace, pi


def _check_rows(O, table, trace, pi, rows):
    n = trace.shape[1]
    num_io = T.SHAPE[table][0]
    alphas = [0x0123456789abcdef, 0x1111111122222222]
    for i in sorted(set(r % n for r in rows)):
        zl, lf, ll = T.trace_domain_consumer_args(n, i)
        assert O.eval_constraints(T.AIR[table], num_io, trace[:, i], trace[:, (i + 1) % n], pi, alphas, zl, lf, ll) == [0, 0], f"row {i}"


def test_edge_lists_host_generator_matches_oracle_and_python(S, O, edge_case):
    """Host generator == oracle, word for word; the outputs in the public inputs == offset + e x / offset * x^e in Python integers;
    the AIR holds on the first and last rows, at instance boundaries and on the steps around the limb seams of the exponent."""
    table, ios, insts, trace, pi = edge_case
    stark = T.stark_class(S, table)(len(insts))
    t_host, pi_host = stark.generate_trace_and_public_inputs(ios)
    assert np.array_equal(pi_host, pi)
    bad = np.nonzero((t_host != trace).any(axis=1))[0]
    assert bad.size == 0, f"first differing columns: {bad[:8].tolist()}"
    got = T.outputs_from_pi(table, pi)
    for k, inst in enumerate(insts):
        assert got[k] == T.expected_output(table, inst), f"instance {k}"
    if table in ("g1", "g2") and insts[0][2] == 0:
        assert got[0] == insts[0][1]                                     # exponent 0: the offset itself
    rpi, n = T.SHAPE[table][4], trace.shape[1]
    rows = [0, 1, n - 2, n - 1]
    for k in (0, 1, len(insts) // 2, len(insts) - 1):
        rows += [rpi * k - 1, rpi * k, rpi * k + 1] + [rpi * k + 2 * t + d for t in (1, 31, 32, 63, 64, 127, 128, 255) for d in (0, 1)
                                                        if 2 * t + 1 < rpi]
    _check_rows(O, table, trace, pi, rows)


def test_g1_edge_list_exponent_r_gives_the_offset():
    """r x = O on G1: every instance with exponent r outputs its offset (a Python check of the list itself)."""
    _, insts = T.edge_list("g1")
    hit = [inst for inst in insts if inst[2] == T.R]
    assert hit
    for x, off, e in hit:
        assert T.expected_output("g1", (x, off, e)) == off


@pytest.fixture(scope="module", params=["g1", "g2"])
def degenerate(request, O):
    curve = request.param
    cases = T.degenerate_cases(curve)
    return curve, cases, T.controls_list(curve, cases)


def _host_chains(S, E, ios, form):
    words = ios.shape[0] * 257 * 3 * E * 4
    ja, jb = np.zeros(words, dtype=np.uint64), np.zeros(words, dtype=np.uint64)
    ios = np.ascontiguousarray(ios, dtype=np.uint32)
    return S.lib().sbn_host_curve_chains(E, ios.ctypes.data_as(C.c_void_p), ios.shape[0], ja.ctypes.data_as(C.c_void_p),
                                         jb.ctypes.data_as(C.c_void_p), form)


def test_degenerate_instances_refused_on_the_host(S, O, degenerate):
    """A collision b_t = +-a_t at step t in {0, 1, 31, 32, 128, 255}, in the first, a middle or the last instance: the host generator and
    both forms of the host chains (one instance at a time, eight per IFMA register where the CPU has it) refuse with SBN_ERR_WITNESS."""
    curve, cases, _ = degenerate
    E = 1 if curve == "g1" else 2
    stark = T.stark_class(S, curve)(T.SHAPE[curve][0])
    for t, s, pos, bad, _ in cases:
        with pytest.raises(S.SbnError) as e:
            stark.generate_trace_and_public_inputs(bad)
        assert e.value.code == -8, (t, s, pos)
        lo = max(0, pos - 8)
        for form in (1, 2):
            rc = _host_chains(S, E, bad[lo:pos + 9], form)
            if form == 2 and rc == -7:
                continue                                            # no AVX-512 IFMA on this CPU
            assert rc == -8, (t, s, pos, form)
    with pytest.raises(AssertionError):                             # the guard keeps degenerate lists away from the oracle
        T.oracle_trace(curve, cases[0][3])


def test_degenerate_control_twins_accepted_on_the_host(S, O, degenerate):
    """The same offsets with bit t cleared are valid witnesses: the host generator accepts them and matches the oracle and Python,
    and the AIR holds on the add / double rows of step t of each control instance."""
    curve, cases, (ios, insts) = degenerate
    trace, pi = T.oracle_trace(curve, ios)
    stark = T.stark_class(S, curve)(len(insts))
    t_host, pi_host = stark.generate_trace_and_public_inputs(ios)
    assert np.array_equal(pi_host, pi)
    assert np.array_equal(t_host, trace)
    got = T.outputs_from_pi(curve, pi)
    rows = []
    for j, (t, _, _, _, twin) in enumerate(cases):
        k = (j * 37) % len(insts)
        assert insts[k] == twin and got[k] == T.expected_output(curve, twin)
        rows += [512 * k + 2 * t - 1, 512 * k + 2 * t, 512 * k + 2 * t + 1]
    _check_rows(O, curve, trace, pi, rows)
    E = 1 if curve == "g1" else 2
    for form in (1, 2):
        assert _host_chains(S, E, ios, form) in ((0, -7) if form == 2 else (0,))


# ---------------------------------------------------------------- BN254 field helpers, host build
def test_bn254_field_helpers_host_build(S):
    """sbn_bn254_fq_batch with on_device = 0: the host build of mmul / fadd / fsub / inv_std / batch_inverse / the Fq2 inverse."""
    T.fq_field_parity(S, on_device=False)
