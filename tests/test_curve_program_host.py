"""Host tests of the curve programs (sbn_curve_program_instances, sbn_curve_program_check and the CurveProgram builder; run with
`-m "not gpu"`), on both curve tables: the derivation equals the node-by-node evaluation over Python integers of
tests/curve_programs.py word for word (list, outputs, values, flags, choice); a program crafted with complete_sums.kill gets the
choice the kills dictate, and one that exhausts the candidates is refused naming the node; every refusal returns its code in the
order the header states; the check accepts the public inputs of the model's list and names the instance and field of every
single corruption."""
import ctypes
import re

import numpy as np
import pytest

import chained_lists as CL
import complete_sums as CS
import curve_programs as G
import tracegen_edges as T

BAD_ARG, VERIFY_FAILED, UNSUPPORTED, WITNESS = -1, -6, -7, -8
P = T.P


def refused(S, code, names, fn, *args, **kw):
    with pytest.raises(S.SbnError) as e:
        fn(*args, **kw)
    assert e.value.code == code and re.search(names, str(e.value)), str(e.value)


def agrees(S, curve, prog, num_io):
    """curve_program_instances equals the model; returns (stark, arrays, the library's tuple)."""
    stark = T.stark_class(S, curve)(num_io)
    arr = G.arrays(curve, *prog)
    got = S.curve_program_instances(stark, *arr)
    want = G.model(curve, *prog, num_io)
    for name, g, w in zip(("ios", "outs", "values", "infinity"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), name
    assert got[4] == want[4]
    return stark, arr, got


def test_exports_and_constants(S):
    for name in ("sbn_curve_program_instances", "sbn_prover_generate_trace_curve_program", "sbn_batch_prover_prove_curve_program", "sbn_curve_program_check"):
        assert name in S.EXPORTS and hasattr(S.lib(), name), name
    assert S.NODE_START == G.START == 0x7FFFFFFE and S.NODE_OUTPUT == G.OUT
    for name in ("CurveProgram", "curve_program_instances", "curve_program_check", "verify_curve_program"):
        assert hasattr(S, name), name
    assert hasattr(S.Prover, "generate_trace_curve_program") and hasattr(S.BatchProver, "prove_curve_program")


# ---------------------------------------------------------------- agreement with the model
@pytest.mark.parametrize("name", ["single", "chain", "tower", "diamond", "lincomb", "infinity", "literal"])
@pytest.mark.parametrize("curve", G.CURVES)
def test_the_small_programs_equal_the_model(S, curve, name):
    prog = G.cases(curve)[name]
    stark, arr, (ios, outs, values, infinity, choice) = agrees(S, curve, prog, 4)
    assert choice == 0                                                       # benign: a nonzero choice elsewhere is crafted, never luck
    nodes, points, exps = prog
    add, neg, mul = T._ops(curve)
    if name == "chain":                                                      # the chained list from candidate `choice`
        terms = CL.terms_words(curve, points, exps)
        want, finals, sums, inf = S.msm_batch_instances(stark, terms, [5], S.start_candidate(stark, choice))
        assert np.array_equal(ios, want) and np.array_equal(outs[4], finals[0]) and np.array_equal(values[4], sums[0]) and not inf[0]
    if name == "tower":
        e = exps[0] * exps[1] * exps[2]
        assert np.array_equal(values[2], CL.value_words(curve, mul(points[0], e % T.R if curve == "g1" else e)))
    if name == "lincomb":
        s1 = add(mul(points[0], exps[0]), mul(points[1], exps[1]))
        s2 = add(mul(points[2], exps[2]), mul(points[3], exps[3]))
        assert np.array_equal(values[5], CL.value_words(curve, add(mul(s2, exps[5]), mul(s1, exps[4]))))
    if name == "infinity" and curve == "g1":
        assert infinity.tolist() == [0, 1] and not values[1].any()
        assert np.array_equal(outs[1], S.start_candidate(stark, 0))          # out = S + r P = S
    if name == "literal":                                                    # T = O: value = out, and the link carries no start
        assert np.array_equal(values[0], outs[0]) and np.array_equal(values[0], CL.value_words(curve, add(points[1], mul(points[0], exps[0]))))
    # null optional outputs
    n, p, e = arr
    assert S.lib().sbn_curve_program_instances(stark.kind, n.ctypes.data, len(n), p.ctypes.data, len(p), e.ctypes.data, len(e), 4, None, None, None, None, None) == 0


@pytest.mark.parametrize("curve", G.CURVES)
def test_300_nodes_cross_two_unit_boundaries(S, curve):
    prog = G.wide(curve, 300)
    nodes = prog[0]
    crossing = {(j // 128, g // 128) for g, nd in enumerate(nodes) for v in nd[:2] if G.is_link(v) for j in [v & ~G.OUT]}
    assert {(0, 1), (0, 2), (1, 2)} <= crossing and G.levels(nodes)[1] == 3
    _, _, (ios, outs, _, _, choice) = agrees(S, curve, prog, 128)
    assert choice == 0 and ios.shape[0] == 3
    assert all(np.array_equal(ios[2, k], ios[2, 300 - 256 - 1]) for k in range(300 - 256, 128))   # the pads copy row count - 1


# ---------------------------------------------------------------- the choice
@pytest.mark.parametrize("j", [1, 2, 7])
@pytest.mark.parametrize("curve", G.CURVES)
def test_killed_candidates_move_the_choice(S, curve, j):
    _, _, got = agrees(S, curve, G.killing(curve, j), 4)
    assert got[4] == j


@pytest.mark.parametrize("curve", G.CURVES)
def test_exhausting_the_candidates_is_a_witness_error_naming_the_node(S, curve):
    stark = T.stark_class(S, curve)(4)
    refused(S, WITNESS, r"candidate 7 fails at node 8\)", S.curve_program_instances, stark, *G.arrays(curve, *G.killing(curve, 8)))
    # events at literal operands are the caller's: no candidate mends them, and the message says so
    prog = G.literal_trap(curve)
    assert G.choose(curve, *prog) == (None, 1)
    refused(S, WITNESS, r"candidate 7 fails at node 1\).*no candidate can mend", S.curve_program_instances, stark, *G.arrays(curve, *prog))


# ---------------------------------------------------------------- refusals, in the order of the header
@pytest.mark.parametrize("curve", G.CURVES)
def test_refusals_in_header_order(S, curve):
    L = S.lib()
    kind = T.stark_class(S, curve)(4).kind
    w = G.W[curve]
    rng = np.random.default_rng(5)
    good = G._rnd(curve, rng)
    pts = np.array([G.point_words(curve, good)] * 4, dtype=np.uint32)
    pts[1, 0:8] = T.limbs(P, 8, 32)                                           # literal 1: a coordinate >= p
    pts[2, 0] ^= 1                                                           # literal 2: off the curve
    pts[3, w - 8:w] = T.limbs(P, 8, 32)                                       # literal 3: the last coordinate >= p
    exps = np.array([T.limbs(7, 8, 32), T.limbs(9, 8, 32)], dtype=np.uint32)

    def call(kind, nodes, points, n_points, e, n_exps, num_io, count=None):
        arr = np.array(nodes, dtype=np.uint32).reshape(-1, 3) if nodes is not None else None
        rc = L.sbn_curve_program_instances(kind, arr.ctypes.data if arr is not None else None, len(arr) if count is None else count,
                                           points.ctypes.data if points is not None else None, n_points, e.ctypes.data if e is not None else None, n_exps, num_io,
                                           None, None, None, None, None)
        return rc, L.sbn_last_error().decode()

    assert call(kind, [(0, G.START, 0), (0, G.out(0), 1)], pts, 4, exps, 2, 4)[0] == 0   # literals 1 .. 3 are unused: not read, not refused
    # 1. the kind, before anything else (null arguments included)
    for other in (S.AIR_FQ_EXP, S.AIR_FQ12_EXP, S.AIR_FQ12_EXP_U64, S.AIR_G1_OP, 99):
        assert call(other, None, None, 0, None, 0, 0, count=0)[0] == UNSUPPORTED, other
    refused(S, UNSUPPORTED, "curve tables", S.curve_program_instances, S.FqExpStark(4), [(0, G.START, 0)], np.zeros((1, 8), dtype=np.uint32), [1])
    # 2. the arguments, before any node is read (node 0 below holds a forward link)
    forward = [(G.out(0), G.START, 0), (2, G.out(0), 1)]
    for args in ((None, pts, 4, exps, 2, 4, 2), (forward, None, 4, exps, 2, 4), (forward, pts, 4, None, 2, 4), (forward, pts, 4, exps, 2, 4, 0),
                 (forward, pts, 4, exps, 2, 0)):
        rc, msg = call(kind, *args)
        assert rc == BAD_ARG and "null argument" in msg, (args[2:], msg)
    for args in ((forward, pts, 4, exps, 2, 4, 0x7FFFFFFF), (forward, pts, 0x7FFFFFFF, exps, 2, 4), (forward, pts, 4, exps, 0x7FFFFFFF, 4)):
        rc, msg = call(kind, *args)
        assert rc == BAD_ARG and "below 2^31 - 1" in msg, (args[2:], msg)
    # 3. node by node: the link, the literal index, SBN_NODE_ONE, SBN_NODE_START as x, the exponent index; of two adjacent refusals
    #    in one node the earlier one wins, and an earlier node wins over a later one
    for nodes, names in (([(G.out(0), 9, 0)], r"node 0: x links to node 0\b"),
                         ([(0, G.START, 0), (9, G.out(5), 0)], r"node 1: offset links to node 5\b"),
                         ([(G.ONE, 4, 0)], r"node 0: offset is literal 4 of 4\b"),
                         ([(4, G.ONE, 0)], r"node 0: x is literal 4 of 4\b"),
                         ([(G.ONE, G.START, 2)], r"node 0: x is SBN_NODE_ONE"),
                         ([(G.START, G.ONE, 2)], r"node 0: offset is SBN_NODE_ONE"),
                         ([(G.START, 0, 2)], r"node 0: x is SBN_NODE_START"),
                         ([(0, 0, 2)], r"node 0: exponent is index 2 of 2\b"),
                         ([(0, 0, 2), (G.out(1), 0, 0)], r"node 0: exponent"),
                         ([(0, G.START, 0), (1, G.START, 2)], r"node 1: exponent")):   # a bad node before any value (literal 1 is >= p)
        rc, msg = call(kind, nodes, pts, 4, exps, 2, 4)
        assert rc == BAD_ARG and re.search(names, msg), (nodes, msg)
    # 4. the used literals in index order: a coordinate >= p (of any used literal) before a point off the curve
    rc, msg = call(kind, [(3, G.START, 0), (2, 1, 0)], pts, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"coordinate >= p \(literal 1\)", msg), msg
    rc, msg = call(kind, [(3, G.START, 0), (2, 0, 0)], pts, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"coordinate >= p \(literal 3\)", msg), msg
    rc, msg = call(kind, [(0, 2, 0)], pts, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"literal 2 is not a point of the curve", msg), msg
    # 5. the witness refusal comes last: a crafted program with an unused bad literal is a witness error, with a used one a bad argument
    nodes, points, e = G.arrays(curve, *G.killing(curve, 8))
    bad = np.concatenate([points, pts[2:3]])
    n_bad = len(bad)
    assert call(kind, nodes, bad, n_bad, e, len(e), 4)[0] == WITNESS
    used = np.concatenate([nodes, np.array([[n_bad - 1, G.START, 0]], dtype=np.uint32)])
    assert call(kind, used, bad, n_bad, e, len(e), 4)[0] == BAD_ARG
    # the check refuses the same way, before it reads a public input
    ptrs = (ctypes.c_void_p * 1)()
    n1 = np.array([(0, G.START, 0)], dtype=np.uint32)
    chk = L.sbn_curve_program_check
    assert chk(S.AIR_FQ_EXP, 4, ptrs, 1, n1.ctypes.data, 1, pts.ctypes.data, 4, exps.ctypes.data, 2, 0, None, None, None) == UNSUPPORTED
    assert chk(kind, 4, ptrs, 1, n1.ctypes.data, 0, pts.ctypes.data, 4, exps.ctypes.data, 2, 0, None, None, None) == BAD_ARG
    assert chk(kind, 4, None, 1, n1.ctypes.data, 1, pts.ctypes.data, 4, exps.ctypes.data, 2, 0, None, None, None) == BAD_ARG
    nf = np.array([(G.out(0), G.START, 0)], dtype=np.uint32)
    assert chk(kind, 4, None, 1, nf.ctypes.data, 1, pts.ctypes.data, 4, exps.ctypes.data, 2, 0, None, None, None) == BAD_ARG
    assert "node 0: x links" in L.sbn_last_error().decode()
    assert chk(kind, 4, ptrs, 1, n1.ctypes.data, 1, pts.ctypes.data, 4, exps.ctypes.data, 2, 8, None, None, None) == BAD_ARG
    assert "start candidates" in L.sbn_last_error().decode()
    assert chk(kind, 4, ptrs, 1, n1.ctypes.data, 1, pts.ctypes.data, 4, exps.ctypes.data, 2, 0, None, None, None) == BAD_ARG   # a null unit


# ---------------------------------------------------------------- curve_program_check
@pytest.fixture(scope="module")
def checked(S):
    """Per curve: a program of 10 nodes in units of 4 (3 units, 2 pads) with literals, START offsets, links within a unit and across
    both unit boundaries, from candidate 1 (the first kill of `killing`), with the public inputs of the model's list."""
    cache = {}

    def get(curve):
        if curve not in cache:
            nodes, points, exps = G.killing(curve, 1)                        # nodes 0 .. 2: START, a kill of candidate 0, a benign node
            exps = list(exps) + [5]
            nodes = list(nodes) + [(G.out(1), G.START, 3), (1, G.out(2), 3), (G.out(3), G.out(1), 2), (0, 1, 3), (G.out(6), G.out(4), 3),
                                   (1, G.START, 2), (G.out(7), G.out(5), 3)]
            stark = T.stark_class(S, curve)(4)
            ios, outs, values, infinity, choice = G.model(curve, nodes, points, exps, 4)
            assert choice == 1 and ios.shape[0] == 3
            cache[curve] = (stark, nodes, G.arrays(curve, nodes, points, exps), outs, values, infinity, G.unit_public_inputs(ios, outs))
        return cache[curve]
    return get


@pytest.mark.parametrize("curve", G.CURVES)
def test_check_accepts_the_model_and_returns_the_values(S, checked, curve):
    stark, nodes, arr, outs, values, infinity, pis = checked(curve)
    got = S.curve_program_check(stark, pis, *arr, 1)
    assert np.array_equal(got[0], outs) and np.array_equal(got[1], values) and np.array_equal(got[2], infinity)
    n, p, e = arr
    ptrs = (ctypes.c_void_p * 3)(*[q.ctypes.data for q in pis])
    assert S.lib().sbn_curve_program_check(stark.kind, 4, ptrs, 3, n.ctypes.data, len(n), p.ctypes.data, len(p), e.ctypes.data, len(e), 1, None, None, None) == 0


# fields of an instance in the public inputs: x, offset (W each), exponent (8), output (W)
def _at(curve, g, field, i=0):
    w = G.W[curve]
    return (3 * w + 8) * (g % 4) + {"x": 0, "offset": w, "exponent": 2 * w, "output": 2 * w + 8}[field] + i


@pytest.mark.parametrize("g,field,i,value,names", [
    (0, "x", 5, None, r"instance 0: x differs from the caller's literal 0\b"),
    (6, "offset", 0, None, r"instance 6: offset differs from the caller's literal 1\b"),
    (4, "exponent", 0, None, r"instance 4: exponent"),
    (0, "offset", 3, None, r"instance 0: offset differs from start candidate 1\b"),
    (8, "offset", 0, None, r"instance 8: offset differs from start candidate 1\b"),
    (1, "offset", 2, None, r"instance 1: offset differs from the output of node 0\b"),
    (3, "x", 0, None, r"instance 3: x differs from the output of node 1\b"),
    (5, "x", 1, None, r"instance 5: x differs from the output of node 3\b"),          # across the first unit boundary
    (9, "offset", 7, None, r"instance 9: offset differs from the output of node 5\b"),  # across the second one
    (10, "x", 0, None, r"instance 10 \(pad\): x differs from instance 9\b"),
    (11, "output", 2, None, r"instance 11 \(pad\): output"),
    (2, "output", 0, 1 << 32, r"instance 2: output limb 0\b"),
    (9, "output", 15, 1 << 32, r"instance 9: output limb 15\b"),
    (9, "output", 0, None, r"instance 9: output is not a point of the curve"),
], ids=["literal_x", "literal_offset", "exponent", "start_first", "start_last", "link_in_unit", "x_link_in_unit", "link_across_first_boundary",
        "link_across_second_boundary", "pad_x", "pad_output", "output_limb_first", "output_limb_last", "output_off_curve"])
@pytest.mark.parametrize("curve", G.CURVES)
def test_check_names_the_tampered_instance_and_field(S, checked, curve, g, field, i, value, names):
    stark, nodes, arr, _, _, _, pis = checked(curve)
    bad = [p.copy() for p in pis]
    at = _at(curve, g, field, i)
    bad[g // 4][at] = value if value is not None else int(bad[g // 4][at]) ^ 1
    refused(S, VERIFY_FAILED, names, S.curve_program_check, stark, bad, *arr, 1)


@pytest.mark.parametrize("curve", G.CURVES)
def test_check_counts_the_units_and_pins_the_choice(S, checked, curve):
    stark, nodes, arr, _, _, _, pis = checked(curve)
    refused(S, VERIFY_FAILED, r"2 units given", S.curve_program_check, stark, pis[:2], *arr, 1)
    refused(S, VERIFY_FAILED, r"4 units given", S.curve_program_check, stark, pis + pis[:1], *arr, 1)
    refused(S, VERIFY_FAILED, r"instance 0: x differs", S.curve_program_check, stark, [pis[1], pis[0], pis[2]], *arr, 1)   # two units swapped
    for choice in (0, 2, 7):                                                 # another choice than the list was derived from
        refused(S, VERIFY_FAILED, rf"instance 0: offset differs from start candidate {choice}\b", S.curve_program_check, stark, pis, *arr, choice)
    refused(S, BAD_ARG, r"start candidates", S.curve_program_check, stark, pis, *arr, 8)
    g = 9                                                                    # output x = 2^256 - 1 >= p; nothing reads it before
    bad = [p.copy() for p in pis]
    at = _at(curve, g, "output")
    bad[g // 4][at:at + 8] = 0xFFFFFFFF
    refused(S, VERIFY_FAILED, rf"instance {g}: output has a coordinate >= p", S.curve_program_check, stark, bad, *arr, 1)
    n, p, e = arr                                                            # the same checks from the caller's side
    p2 = p.copy()
    p2[1, 0] ^= 1
    refused(S, VERIFY_FAILED, r"instance 2: x differs from the caller's literal 1\b", S.curve_program_check, stark, pis, n, p2, e, 1)
    e2 = e.copy()
    e2[3, 0] ^= 1
    refused(S, VERIFY_FAILED, r"instance 3: exponent", S.curve_program_check, stark, pis, n, p, e2, 1)


# ---------------------------------------------------------------- the builder
@pytest.mark.parametrize("curve", G.CURVES)
def test_the_builder_states_multiples_sums_and_combinations(S, curve):
    stark = T.stark_class(S, curve)(4)
    rng = np.random.default_rng(7)
    add, neg, mul = T._ops(curve)
    p, q = G._rnd(curve, rng), G._rnd(curve, rng)
    pw, qw = CL.value_words(curve, p), CL.value_words(curve, q)
    pg = S.CurveProgram(stark)
    assert pg.point(pw).ref == pg.point(list(pw)).ref == 0
    a = pg.mul(pw, 5)                                                        # 5 P
    b = pg.mul(a, 7)                                                         # 7 (5 P): a multiple of a result
    c = pg.add(a, b)                                                         # 40 P
    d = pg.lincomb([(3, qw), (11, c), (5, pw)])                              # 3 Q + 440 P + 5 P
    nodes, points, exps = pg.arrays()
    assert len(pg) == 6 and points.shape == (2, G.W[curve]) and exps.shape == (5, 8) and d.node == 5   # 5, 7, 1, 3, 11: the second 5 shares a slot
    assert nodes[0].tolist() == [0, S.NODE_START, 0] and nodes[1].tolist() == [S.NODE_OUTPUT | 0, S.NODE_START, 1] and nodes[2].tolist() == [S.NODE_OUTPUT | 1, S.NODE_OUTPUT | 0, 2]
    _, _, values, infinity, choice = S.curve_program_instances(stark, nodes, points, exps)
    assert choice == 0 and not infinity.any()
    for h, want in ((a, mul(p, 5)), (b, mul(p, 35)), (c, mul(p, 40)), (d, add(mul(q, 3), mul(p, 445)))):
        assert np.array_equal(values[h.node], CL.value_words(curve, want))
    with pytest.raises(S.SbnError):
        pg.mul(S.CurveProgram.START, 3)
