"""Host tests of the field programs (sbn_program_levels, sbn_program_instances, sbn_program_check and the Program builder; run
with `-m "not gpu"`): a program written as towers or as a chained list equals sbn_power_instances / sbn_chain_instances word for
word, a fixed DAG with every kind of link equals the node-by-node evaluation over Python integers of tests/program_lists.py on all
three tables, the schedule equals a ten-line recomputation, every refusal returns its code in the order the header states, the
check accepts the host generator's public inputs and names the instance and field of every single edit, and the builder's Horner
chains, Frobenius maps and products equal Python's."""
import ctypes
import re

import numpy as np
import pytest

import power_lists as PL
import program_lists as G
import tracegen_edges as T

BAD_ARG, NON_CANONICAL, VERIFY_FAILED, UNSUPPORTED = -1, -2, -6, -7
P = PL.P
TABLES = ["fq", "fq12", "fq12u64"]


def refused(S, code, names, fn, *args, **kw):
    with pytest.raises(S.SbnError) as e:
        fn(*args, **kw)
    assert e.value.code == code and re.search(names, str(e.value)), str(e.value)


def test_exports_and_constants(S):
    for name in ("sbn_program_levels", "sbn_program_instances", "sbn_prover_generate_trace_program", "sbn_batch_prover_prove_program", "sbn_program_check"):
        assert name in S.EXPORTS and hasattr(S.lib(), name), name
    assert (S.NODE_OUTPUT, S.NODE_ONE) == (G.OUT, G.ONE) == (0x80000000, 0x7FFFFFFF)
    for name in ("Program", "program_levels", "program_instances", "program_check", "verify_program"):
        assert hasattr(S, name), name
    assert hasattr(S.Prover, "generate_trace_program") and hasattr(S.BatchProver, "prove_program")


# ---------------------------------------------------------------- the two hard-coded link patterns, written as programs
def _exps_for(table, r, n):
    top = PL.GLP if table == "fq12u64" else 1 << 256
    return [r.randrange(top) for _ in range(n)]


@pytest.mark.parametrize("table", TABLES)
def test_towers_as_a_program_equal_power_instances(S, table):
    """3 towers of depth 3 in units of 4: 9 instances, 3 pads, towers across both unit boundaries; per-tower, then shared, exponents."""
    r = PL.rng(101)
    stark = T.stark_class(S, table)(4)
    bases = [PL.random_elem(table, r) for _ in range(3)]
    for exps in (_exps_for(table, r, 3), _exps_for(table, r, 1)):
        ios_want, powers_want = S.power_instances(stark, PL.base_words(table, bases), PL.exp_words(table, exps), 3)
        nodes, values, ews = G.arrays(table, G.towers_as_program(3, 3, len(exps) == 1), bases, exps)
        ios, outs = S.program_instances(stark, nodes, values, ews)
        assert ios.shape == ios_want.shape == (3, 4, sum(PL.WORDS[table]) + PL.WORDS[table][0])
        assert np.array_equal(ios, ios_want) and np.array_equal(outs, powers_want.reshape(9, -1))


@pytest.mark.parametrize("table", TABLES)
def test_a_chain_as_a_program_equals_chain_instances(S, table):
    """offset[k+1] = output[k] from a literal start: the explicit list of sbn_chain_instances (one unit of 4, no pad)."""
    r = PL.rng(102)
    w, ew = PL.WORDS[table]
    stark = T.stark_class(S, table)(4)
    start, xs, exps = PL.random_elem(table, r), [PL.random_elem(table, r) for _ in range(4)], _exps_for(table, r, 4)
    terms = np.array([PL.elem_words(table, x) + PL.limbs(e, ew) for x, e in zip(xs, exps)], dtype=np.uint32)
    ios_want, final = S.chain_instances(stark, terms, np.array(PL.elem_words(table, start), dtype=np.uint32))
    nodes, values, ews = G.arrays(table, G.chain_as_program(4), [start] + xs, exps)
    ios, outs = S.program_instances(stark, nodes, values, ews)
    assert np.array_equal(ios[0], ios_want) and np.array_equal(outs[3], np.asarray(final).reshape(-1))


# ---------------------------------------------------------------- the DAG against the Python evaluator
@pytest.fixture(scope="module")
def dag_case(S):
    """(nodes, values, exps as Python values; their arrays; ios, outs of the library; the Python units and outs), once per table."""
    cache = {}

    def get(table):
        if table not in cache:
            nodes, values, exps = G.dag(table)
            arr = G.arrays(table, nodes, values, exps)
            stark = T.stark_class(S, table)(4)
            ios, outs = S.program_instances(stark, *arr)
            cache[table] = (stark, nodes, values, exps, arr, ios, outs, G.explicit_units(table, nodes, values, exps, 4))
        return cache[table]
    return get


@pytest.mark.parametrize("table", TABLES)
def test_the_dag_equals_the_python_evaluation(S, dag_case, table):
    stark, nodes, values, exps, arr, ios, outs, (units_want, outs_want) = dag_case(table)
    # a condition on the chosen input: x-link, offset-link, both links to different nodes and to the same node, an output and a
    # literal used twice, a link across a unit boundary and one more than one back, zero base, zero exponent, exponent one, one
    assert len(nodes) == 11 and G.dag_properties(nodes, values, exps, 4) == G.DAG_PROPERTIES
    assert ios.shape == units_want.shape and ios.shape[:2] == (3, 4)
    assert np.array_equal(outs, outs_want)
    assert np.array_equal(ios, units_want)
    assert np.array_equal(ios[2, 3], ios[2, 2])                              # the pad
    ev = G.evaluate(table, nodes, values, exps)
    assert ev[6][2] == G.zero(table) and ev[7][2] == G.one(table) and ev[8][2] == ev[5][2]   # 0^e = 0, x^0 = 1, 0^0 = 1
    # null optional outputs
    n, v, e = arr
    assert S.lib().sbn_program_instances(stark.kind, n.ctypes.data, 11, v.ctypes.data, 3, e.ctypes.data, 4, 4, None, None) == 0


# ---------------------------------------------------------------- the schedule
def test_levels_equal_the_recomputation(S):
    independent = [(k, G.ONE, 0) for k in range(7)]
    level, depth = S.program_levels(independent)
    assert level.tolist() == [0] * 7 and depth == 1 and G.levels(independent) == ([0] * 7, 1)
    chain = [(0, G.ONE, 0)] + [(G.out(k - 1), G.ONE, 0) for k in range(1, 16)]
    level, depth = S.program_levels(chain)
    assert level.tolist() == list(range(16)) and depth == 16 and G.levels(chain) == (list(range(16)), 16)
    nodes, _, _ = G.dag("fq12")
    level, depth = S.program_levels(nodes)
    assert (level.tolist(), depth) == G.levels(nodes) and level.tolist() == [0, 0, 1, 1, 2, 3, 1, 4, 4, 5, 6] and depth == 7
    # optional outputs, and the structural refusals
    arr = np.array(nodes, dtype=np.uint32)
    assert S.lib().sbn_program_levels(arr.ctypes.data, 11, None, None) == 0
    assert S.lib().sbn_program_levels(None, 11, None, None) == BAD_ARG and S.lib().sbn_program_levels(arr.ctypes.data, 0, None, None) == BAD_ARG
    refused(S, BAD_ARG, r"node 1: x links to node 1\b", S.program_levels, [(0, G.ONE, 0), (G.out(1), G.ONE, 0)])
    refused(S, BAD_ARG, r"node 0: offset links to node 0\b", S.program_levels, [(0, G.out(0), 0)])
    refused(S, BAD_ARG, r"node 1: x is SBN_NODE_ONE", S.program_levels, [(0, G.ONE, 0), (G.ONE, G.ONE, 0)])


# ---------------------------------------------------------------- refusals, in the order of the header
def test_refusals_in_header_order(S):
    L = S.lib()
    big = PL.base_words("fq", [3, P, 5, P])                                  # literals 1 and 3 are >= p
    exps = PL.exp_words("fq", [7, 9])

    def call(kind, nodes, values, n_values, e, n_exps, num_io, count=None):
        arr = np.array(nodes, dtype=np.uint32).reshape(-1, 3) if nodes is not None else None
        rc = L.sbn_program_instances(kind, arr.ctypes.data if arr is not None else None, len(arr) if count is None else count,
                                     values.ctypes.data if values is not None else None, n_values, e.ctypes.data if e is not None else None, n_exps, num_io, None, None)
        return rc, L.sbn_last_error().decode()

    ok = [(0, G.ONE, 0), (2, G.out(0), 1)]
    assert call(S.AIR_FQ_EXP, ok, big, 4, exps, 2, 4)[0] == 0                 # literals 1 and 3 are unused: not read, not refused
    # 1. the kind, before anything else (null arguments included)
    for kind in (S.AIR_G1_EXP, S.AIR_G2_EXP, S.AIR_G1_OP, S.AIR_FQ12_MUL, 99):
        assert call(kind, None, None, 0, None, 0, 0, count=0)[0] == UNSUPPORTED, kind
    refused(S, UNSUPPORTED, "field tables", S.program_instances, S.G1ExpStark(128), [(0, G.ONE, 0)], np.zeros((1, 16), dtype=np.uint32), [1])
    # 2. the arguments, before any node is read (node 0 below holds a forward link)
    forward = [(G.out(0), G.ONE, 0), (2, G.out(0), 1)]
    for args in ((None, big, 4, exps, 2, 4, 2), (forward, None, 4, exps, 2, 4), (forward, big, 4, None, 2, 4), (forward, big, 4, exps, 2, 4, 0),
                 (forward, big, 4, exps, 2, 0)):
        rc, msg = call(S.AIR_FQ_EXP, *args)
        assert rc == BAD_ARG and "null argument" in msg, (args[2:], msg)
    for args in ((forward, big, 4, exps, 2, 4, 0x7FFFFFFF), (forward, big, 0x7FFFFFFF, exps, 2, 4), (forward, big, 4, exps, 0x7FFFFFFF, 4)):
        rc, msg = call(S.AIR_FQ_EXP, *args)
        assert rc == BAD_ARG and "below 2^31 - 1" in msg, (args[2:], msg)
    # 3. node by node: the link before the literal index before one as x before the exponent index; every pair of adjacent
    #    refusals in one node, the earlier one wins; then an earlier node wins over a later one
    rc, msg = call(S.AIR_FQ_EXP, [(G.out(0), 9, 0)], big, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"node 0: x links to node 0\b", msg), msg
    rc, msg = call(S.AIR_FQ_EXP, [(0, G.ONE, 0), (9, G.out(5), 0)], big, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"node 1: offset links to node 5\b", msg), msg
    rc, msg = call(S.AIR_FQ_EXP, [(G.ONE, 4, 0)], big, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"node 0: offset is literal 4 of 4\b", msg), msg
    rc, msg = call(S.AIR_FQ_EXP, [(4, 0, 0)], big, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"node 0: x is literal 4 of 4\b", msg), msg
    rc, msg = call(S.AIR_FQ_EXP, [(G.ONE, 0, 2)], big, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"node 0: x is SBN_NODE_ONE", msg), msg
    rc, msg = call(S.AIR_FQ_EXP, [(0, 0, 2)], big, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"node 0: exponent is index 2 of 2\b", msg), msg
    rc, msg = call(S.AIR_FQ_EXP, [(0, 0, 2), (G.out(1), 0, 0)], big, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"node 0: exponent", msg), msg
    # ... and a bad node before any value (node 1 uses literal 1, which is >= p)
    rc, msg = call(S.AIR_FQ_EXP, [(0, G.ONE, 0), (1, G.ONE, 2)], big, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"node 1: exponent", msg), msg
    # 4. the used literals in index order, then the used exponents
    rc, msg = call(S.AIR_FQ_EXP, [(3, G.ONE, 0), (0, 1, 0)], big, 4, exps, 2, 4)
    assert rc == BAD_ARG and re.search(r"value >= p \(literal 1\)", msg), msg
    f12 = np.zeros((3, 96), dtype=np.uint32)
    f12[2, 88:96] = PL.limbs(P, 8)                                           # the last coefficient of literal 2
    for kind in (S.AIR_FQ12_EXP, S.AIR_FQ12_EXP_U64):
        rc, msg = call(kind, [(0, 2, 0)], f12, 3, exps, 1, 16)
        assert rc == BAD_ARG and re.search(r"coefficient >= p \(literal 2\)", msg), msg
        assert call(kind, [(0, 1, 0)], f12, 3, exps, 1, 16)[0] == 0          # unused: not read
    e64 = PL.exp_words("fq12u64", [PL.BN_X, PL.GLP, PL.GLP - 1, PL.GLP])
    rc, msg = call(S.AIR_FQ12_EXP_U64, [(0, 2, 1)], f12, 3, e64, 4, 16)       # a literal before an exponent
    assert rc == BAD_ARG and re.search(r"literal 2", msg), msg
    rc, msg = call(S.AIR_FQ12_EXP_U64, [(0, 1, 3), (0, 1, 1)], f12, 3, e64, 4, 16)
    assert rc == NON_CANONICAL and re.search(r"exponent 1\b", msg), msg
    assert call(S.AIR_FQ12_EXP_U64, [(0, 1, 2), (0, 1, 0)], f12, 3, e64, 4, 16)[0] == 0   # the unused exponents are not read
    assert call(S.AIR_FQ12_EXP, [(0, 1, 1)], f12, 3, PL.exp_words("fq12", [1, (1 << 256) - 1]), 2, 16)[0] == 0   # 256 bits: any exponent
    # the check refuses the same way, before it reads a public input
    ptrs = (ctypes.c_void_p * 1)()
    n1 = np.array([(0, G.ONE, 0)], dtype=np.uint32)
    assert L.sbn_program_check(S.AIR_G1_EXP, 4, ptrs, 1, n1.ctypes.data, 1, big.ctypes.data, 4, exps.ctypes.data, 2, None) == UNSUPPORTED
    assert L.sbn_program_check(S.AIR_FQ_EXP, 4, ptrs, 1, n1.ctypes.data, 0, big.ctypes.data, 4, exps.ctypes.data, 2, None) == BAD_ARG
    assert L.sbn_program_check(S.AIR_FQ_EXP, 4, None, 1, n1.ctypes.data, 1, big.ctypes.data, 4, exps.ctypes.data, 2, None) == BAD_ARG
    nf = np.array([(G.out(0), G.ONE, 0)], dtype=np.uint32)
    assert L.sbn_program_check(S.AIR_FQ_EXP, 4, None, 1, nf.ctypes.data, 1, big.ctypes.data, 4, exps.ctypes.data, 2, None) == BAD_ARG
    assert "node 0: x links" in L.sbn_last_error().decode()
    assert L.sbn_program_check(S.AIR_FQ_EXP, 4, ptrs, 1, n1.ctypes.data, 1, big.ctypes.data, 4, exps.ctypes.data, 2, None) == BAD_ARG   # a null unit


# ---------------------------------------------------------------- program_check
U64_PER, U64_X, U64_OFF, U64_EXP, U64_OUT = 577, 0, 192, 384, 385


@pytest.fixture(scope="module")
def checked(S, dag_case):
    """The DAG on Fq12ExpU64Stark(4) with the public inputs of its three units from the unchanged host generator."""
    stark, nodes, values, exps, arr, ios, outs, _ = dag_case("fq12u64")
    return stark, nodes, arr, outs, [stark.generate_public_inputs(u) for u in ios]


def test_program_check_accepts_the_honest_public_inputs(S, checked):
    stark, nodes, arr, outs, pis = checked
    assert np.array_equal(S.program_check(stark, pis, *arr), outs)
    n, v, e = arr
    ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in pis])
    assert S.lib().sbn_program_check(stark.kind, 4, ptrs, 3, n.ctypes.data, 11, v.ctypes.data, 3, e.ctypes.data, 4, None) == 0   # outs_out is optional


@pytest.mark.parametrize("table", ["fq", "fq12"])
def test_program_check_on_the_other_tables(S, dag_case, table):
    stark, nodes, values, exps, arr, ios, outs, _ = dag_case(table)
    padded = np.concatenate([outs, outs[-1:]])                               # the pad repeats the last output
    pis = [G.public_inputs(table, u, padded[4 * i:4 * i + 4]) for i, u in enumerate(ios)]
    if table == "fq12":                                                      # the unchanged host generator states the same words
        assert all(np.array_equal(stark.generate_public_inputs(u), p) for u, p in zip(ios, pis))
    assert np.array_equal(S.program_check(stark, pis, *arr), outs)
    per = stark.num_public_inputs // 4
    bad = [p.copy() for p in pis]
    bad[1][per * 0 + 0] ^= 1                                                 # instance 4: x, linked to node 2
    refused(S, VERIFY_FAILED, r"instance 4: x differs from the output of node 2\b", S.program_check, stark, bad, *arr)


# the DAG's fields by kind (program_lists.dag): literal x at 0, 1, 3, 6, 8; literal offset at 1; one at 0, 2, 7; x-links at 2, 4, 5,
# 7, 9, 10; offset-links at 3, 4, 5, 6, 8, 9, 10; the pad is instance 11.  Each edit at the first and at the last instance it applies to.
@pytest.mark.parametrize("g,at,value,names", [
    (0, U64_X + 5, None, r"instance 0: x differs from the caller's literal 0\b"),
    (8, U64_X, 1, r"instance 8: x differs from the caller's literal 2\b"),
    (1, U64_OFF + 191, None, r"instance 1: offset differs from the caller's literal 0\b"),
    (0, U64_OFF, None, r"instance 0: offset is not one"),
    (7, U64_OFF + 1, 1, r"instance 7: offset is not one"),
    (0, U64_EXP, None, r"instance 0: exponent"),
    (10, U64_EXP, None, r"instance 10: exponent"),
    (2, U64_X + 3, None, r"instance 2: x differs from the output of node 0\b"),
    (10, U64_X + 100, None, r"instance 10: x differs from the output of node 9\b"),
    (3, U64_OFF, None, r"instance 3: offset differs from the output of node 0\b"),
    (10, U64_OFF + 7, None, r"instance 10: offset differs from the output of node 2\b"),
    (11, U64_X, None, r"instance 11 \(pad\): x differs from instance 10\b"),
    (11, U64_OFF, None, r"instance 11 \(pad\): offset"),
    (11, U64_EXP, None, r"instance 11 \(pad\): exponent"),
    (11, U64_OUT + 191, None, r"instance 11 \(pad\): output"),
    (0, U64_OUT, 1 << 16, r"instance 0: output limb 0\b"),
    (10, U64_OUT + 191, 1 << 16, r"instance 10: output limb 191\b"),
], ids=["literal_x_first", "literal_x_last", "literal_offset", "one_first", "one_last", "exponent_first", "exponent_last", "x_link_first",
        "x_link_last", "offset_link_first", "offset_link_last", "pad_x", "pad_offset", "pad_exponent", "pad_output", "output_limb_first",
        "output_limb_last"])
def test_program_check_names_the_tampered_instance_and_field(S, checked, g, at, value, names):
    stark, nodes, arr, _, pis = checked
    bad = [p.copy() for p in pis]
    w = bad[g // 4]
    i = U64_PER * (g % 4) + at
    w[i] = value if value is not None else int(w[i]) ^ 1
    refused(S, VERIFY_FAILED, names, S.program_check, stark, bad, *arr)


def test_program_check_names_a_wrong_caller_side(S, checked):
    """The same checks from the other side: honest public inputs, a caller whose literal or exponent differs."""
    stark, nodes, (n, v, e), _, pis = checked
    v2 = v.copy()
    v2[1, 0] ^= 1                                                            # literal 1: x of nodes 1 and 3
    refused(S, VERIFY_FAILED, r"instance 1: x differs from the caller's literal 1\b", S.program_check, stark, pis, n, v2, e)
    e2 = e.copy()
    e2[3, 0] ^= 1                                                            # exponent 3: nodes 2, 5, 10
    refused(S, VERIFY_FAILED, r"instance 2: exponent", S.program_check, stark, pis, n, v, e2)


def test_program_check_counts_and_orders_the_units_and_bounds_the_coefficients(S, checked):
    stark, nodes, arr, _, pis = checked
    refused(S, VERIFY_FAILED, r"2 units given", S.program_check, stark, pis[:2], *arr)          # one unit too few
    refused(S, VERIFY_FAILED, r"4 units given", S.program_check, stark, pis + pis[:1], *arr)
    refused(S, VERIFY_FAILED, r"instance 0: x differs", S.program_check, stark, [pis[1], pis[0], pis[2]], *arr)   # two units swapped
    refused(S, VERIFY_FAILED, r"instance 4: x differs from the output of node 2\b", S.program_check, stark, [pis[0], pis[2], pis[1]], *arr)
    for g in (1, 10):                                                        # output coefficient 0 = 2^256 - 1 >= p; nothing reads these before
        bad = [p.copy() for p in pis]
        at = U64_PER * (g % 4) + U64_OUT
        bad[g // 4][at:at + 16] = 0xFFFF
        refused(S, VERIFY_FAILED, rf"instance {g}: output has a coefficient >= p", S.program_check, stark, bad, *arr)


# ---------------------------------------------------------------- the builder
def _frobenius(x):
    """x^p in the flat basis, as a power over Python integers."""
    return PL.fq12_pow(x, P)


def test_the_builder_shares_slots_and_counts_nodes_by_bit_length(S):
    stark = S.Fq12ExpStark(16)
    r = PL.rng(201)
    f = PL.elem_words("fq12", PL.random_elem("fq12", r))
    pg = S.Program(stark)
    a, b = pg.value(f), pg.value(list(f))
    assert a.ref == b.ref == 0 and pg.limb_bits == 255 and S.Program(S.Fq12ExpU64Stark(16)).limb_bits == 63
    h = pg.pow(f, 5)
    h2 = pg.pow(h, 5, offset=f)
    nodes, values, exps = pg.arrays()
    assert nodes.tolist() == [[0, S.NODE_ONE, 0], [S.NODE_OUTPUT | 0, 0, 0]] and values.shape == (1, 96) and exps.shape == (1, 8) and h2.node == 1
    for e in (1 << 599, (1 << 600) - 1, 1 << 510):                            # 3 limbs of 255 bits: 1 + 2 * 2 nodes, zero limbs included
        q = S.Program(stark)
        q.pow_big(f, e)
        assert len(q) == 5, e
    q = S.Program(stark)
    q.pow_big(f, 0)
    assert len(q) == 1


def test_pow_big_frobenius_and_products_on_fq12(S):
    """Fq12ExpStark: a 600-bit exponent by Horner, the Frobenius map as the exponent p, and a product of two earlier results."""
    stark = S.Fq12ExpStark(4)
    r = PL.rng(202)
    f, g = PL.random_elem("fq12", r), PL.random_elem("fq12", r)
    e = r.randrange(1 << 599, 1 << 600)
    pg = S.Program(stark)
    big = pg.pow_big(PL.elem_words("fq12", f), e)
    frob = pg.pow(PL.elem_words("fq12", f), P)
    prod = pg.mul(PL.elem_words("fq12", f), PL.elem_words("fq12", g))
    both = pg.mul(big, frob)
    nodes, values, exps = pg.arrays()
    assert len(pg) == 5 + 3 and values.shape[0] == 2
    ios, outs = S.program_instances(stark, nodes, values, exps)
    assert ios.shape == (2, 4, 200)
    want_big, want_frob = PL.fq12_pow(f, e), _frobenius(f)
    assert PL.elem_from_words("fq12", outs[big.node].tolist()) == want_big
    assert PL.elem_from_words("fq12", outs[frob.node].tolist()) == want_frob
    assert PL.elem_from_words("fq12", outs[prod.node].tolist()) == PL.fq12_mul(f, g)
    assert PL.elem_from_words("fq12", outs[both.node].tolist()) == PL.fq12_mul(want_big, want_frob)
    # a check f * f_inv = 1, read off the output (in Fq, where the inverse is one power)
    fq = S.FqExpStark(4)
    pq = S.Program(fq)
    x = r.randrange(1, P)
    chk = pq.mul(x, pq.pow(x, P - 2))
    _, o = S.program_instances(fq, *pq.arrays())
    assert PL.from_limbs(o[chk.node]) == 1


def test_pow_big_on_fq12_u64(S):
    """Fq12ExpU64Stark: a 150-bit exponent is three limbs of 63 bits."""
    stark = S.Fq12ExpU64Stark(4)
    r = PL.rng(203)
    f = PL.random_elem("fq12", r)
    e = r.randrange(1 << 149, 1 << 150)
    pg = S.Program(stark)
    h = pg.pow_big(PL.elem_words("fq12", f), e)
    assert len(pg) == 5 and h.node == 4
    nodes, values, exps = pg.arrays()
    assert (1 << 63) in [PL.from_limbs(w) for w in exps]
    _, outs = S.program_instances(stark, nodes, values, exps)
    assert PL.elem_from_words("fq12", outs[h.node].tolist()) == PL.fq12_pow(f, e)
    level, depth = S.program_levels(nodes)
    assert depth == 5 and G.levels([tuple(n) for n in nodes.tolist()]) == (level.tolist(), depth)
