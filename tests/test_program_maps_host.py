"""Host tests of the mapped links of the field programs and of the final exponentiation (include/sbn.h, "Mapped links and the final
exponentiation"; run with `-m "not gpu"`): the committed constants are what their generator writes and what pow() of xi gives, the
host map equals the power p^m over Python integers and composes mod 12, the inverse times its argument is one, a mapped DAG equals
the node-by-node evaluation of tests/program_maps.py on both Fq12 tables, every `_m` call with zero maps equals its twin word for
word, the added refusals fire in the header's order, the check recomputes the map on the output public inputs and names instance,
field, node and map of every edit, and the 16-node program gives f^((p^12 - 1) / r).  Every comparison is exact equality."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import power_lists as PL
import program_lists as G
import program_maps as PM
import tracegen_edges as T

BAD_ARG, VERIFY_FAILED, UNSUPPORTED = -1, -6, -7
P = PL.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_CALLS = ("sbn_program_m_levels", "sbn_program_m_instances", "sbn_prover_generate_trace_program_m", "sbn_batch_prover_prove_program_m", "sbn_program_m_check")


def refused(S, code, names, fn, *args, **kw):
    with pytest.raises(S.SbnError) as e:
        fn(*args, **kw)
    assert e.value.code == code and re.search(names, str(e.value)), str(e.value)


def words(v):
    return np.array(PL.elem_words("fq12", v), dtype=np.uint32)


def elem(w):
    return PL.elem_from_words("fq12", np.asarray(w).reshape(-1).tolist())


# ---------------------------------------------------------------- 1. constants and the map
def test_exports_and_constants(S):
    for name in M_CALLS + ("sbn_fq12_frobenius", "sbn_fq12_inverse"):
        assert name in S.EXPORTS and hasattr(S.lib(), name), name
    for name in ("fq12_frobenius", "fq12_conjugate", "fq12_inverse", "final_exponentiation", "verify_final_exponentiations"):
        assert hasattr(S, name), name
    assert S.FINAL_EXP_NODES == PM.FINAL_EXP_NODES == 16
    assert hasattr(S.Program, "frobenius") and hasattr(S.Program, "conj") and hasattr(S.BatchProver, "prove_final_exponentiations")


def test_the_generator_reproduces_the_committed_header(tmp_path):
    env = dict(os.environ, SBN_GEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_fq12_frobenius.py")], env=env, stdout=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "starky_bn254_amd", "csrc", "fq12_frobenius_consts.hpp")) as f, open(tmp_path / "fq12_frobenius_consts.hpp") as g:
        assert f.read() == g.read()
    assert not [n for n in os.listdir(os.path.join(ROOT, "starky_bn254_amd", "csrc")) if "frobenius" in n and n.endswith(".inc")]


def test_the_committed_table_is_pow_of_xi():
    with open(os.path.join(ROOT, "starky_bn254_amd", "csrc", "fq12_frobenius_consts.hpp")) as f:
        nums = [int(t, 16) for t in re.findall(r"0x([0-9a-f]{16})ULL", f.read())]
    assert len(nums) == 12 * 6 * 2 * 4
    vals = [sum(nums[4 * i + j] << (64 * j) for j in range(4)) for i in range(12 * 6 * 2)]
    for m in range(12):
        for k in range(6):
            at = 2 * (6 * m + k)
            assert (vals[at], vals[at + 1]) == PM.f2pow(PM.XI, k * (P ** m - 1) // 6) == PM.gamma(m, k), (m, k)
    assert all(PM.gamma(6, k) == ((1, 0) if k % 2 == 0 else (P - 1, 0)) for k in range(6))


@pytest.fixture(scope="module")
def elements():
    r = PL.rng(301)
    return [PL.random_elem("fq12", r), PL.random_elem("fq12", r), [0] * 12, list(PL.FQ12_ONE), [P - 1] * 12]


def test_the_host_map_is_the_power_p_to_the_m(S, elements):
    for f in elements:
        want = f
        for m in range(12):
            got = elem(S.fq12_frobenius(words(f), m))
            assert got == want == PM.frob(f, m), m
            want = PL.fq12_pow(want, P)                                       # f^(p^(m+1))
        assert want == f                                                      # p^12 is the identity
        assert elem(S.fq12_conjugate(words(f))) == PM.frob(f, 6)


def test_maps_compose_mod_12(S, elements):
    f = words(elements[0])
    for a in range(12):
        fa = S.fq12_frobenius(f, a)
        for b in range(12):
            assert np.array_equal(S.fq12_frobenius(fa, b), S.fq12_frobenius(f, (a + b) % 12)), (a, b)
    assert np.array_equal(S.fq12_frobenius(f, 0), f)


def test_the_map_works_in_place(S, elements):
    f = words(elements[1])
    want = S.fq12_frobenius(f, 5)
    buf = f.copy()
    assert S.lib().sbn_fq12_frobenius(buf.ctypes.data, 5, buf.ctypes.data) == 0 and np.array_equal(buf, want)


# ---------------------------------------------------------------- 2. the inverse
def test_the_inverse_times_f_is_one(S, elements):
    for f in elements[:2] + elements[3:]:
        fi = elem(S.fq12_inverse(words(f)))
        assert PL.fq12_mul(f, fi) == PL.FQ12_ONE and fi == PM.fq12_inverse(f)


def test_refusals_of_the_helpers(S, elements):
    L = S.lib()
    f, out = words(elements[0]), np.zeros(96, dtype=np.uint32)
    refused(S, BAD_ARG, "zero has no inverse", S.fq12_inverse, words([0] * 12))
    big = f.copy()
    big[88:96] = PL.limbs(P, 8)
    refused(S, BAD_ARG, "coefficient >= p", S.fq12_inverse, big)
    refused(S, BAD_ARG, "coefficient >= p", S.fq12_frobenius, big, 1)
    refused(S, BAD_ARG, "0 .. 11", S.fq12_frobenius, f, 12)
    assert L.sbn_fq12_frobenius(None, 1, out.ctypes.data) == BAD_ARG and L.sbn_fq12_frobenius(f.ctypes.data, 1, None) == BAD_ARG
    assert L.sbn_fq12_inverse(None, out.ctypes.data) == BAD_ARG and L.sbn_fq12_inverse(f.ctypes.data, None) == BAD_ARG


# ---------------------------------------------------------------- 3. a mapped DAG against the Python evaluation
@pytest.fixture(scope="module")
def dag_case(S):
    cache = {}

    def get(table):
        if table not in cache:
            nodes, values, exps = PM.dag(table)
            arr = PM.arrays(table, nodes, values, exps)
            stark = T.stark_class(S, table)(4)
            ios, outs = S.program_instances(stark, *arr)
            cache[table] = (stark, nodes, values, exps, arr, ios, outs, PM.explicit_units(table, nodes, values, exps, 4))
        return cache[table]
    return get


@pytest.mark.parametrize("table", ["fq12", "fq12u64"])
def test_the_mapped_dag_equals_the_python_evaluation(S, dag_case, table):
    stark, nodes, values, exps, arr, ios, outs, (units_want, outs_want) = dag_case(table)
    # a condition on the chosen input: every m in 1..11 at x and at offset, both operands the same node under different maps, a
    # mapped link across a unit boundary, a mapped last node, an output used both mapped and unmapped
    assert len(nodes) == 15 and arr[0].shape == (15, 4) and PM.DAG_PROPERTIES <= PM.dag_properties(nodes, 4)
    assert ios.shape == units_want.shape and ios.shape[:2] == (4, 4)
    assert np.array_equal(outs, outs_want)
    assert np.array_equal(ios, units_want)
    assert np.array_equal(ios[3, 3], ios[3, 2]) and nodes[14][3]             # the pad copies the mapped words of the last node
    level, depth = S.program_levels(arr[0])
    assert (level.tolist(), depth) == PM.levels(nodes) and depth == 12       # a map adds no level
    n, v, e = arr
    assert S.lib().sbn_program_m_instances(stark.kind, n.ctypes.data, 15, v.ctypes.data, 2, e.ctypes.data, 4, 4, None, None) == 0
    assert S.lib().sbn_program_m_levels(n.ctypes.data, 15, None, None) == 0


# ---------------------------------------------------------------- 4. all maps zero: every _m call is its twin
@pytest.mark.parametrize("table", ["fq", "fq12", "fq12u64"])
def test_zero_maps_equal_the_twin_word_for_word(S, table):
    L = S.lib()
    nodes, values, exps = G.dag(table)
    n3, v, e = G.arrays(table, nodes, values, exps)
    n4 = np.concatenate([n3, np.zeros((11, 1), dtype=np.uint32)], axis=1)
    assert n4.shape == (11, 4) and n4.flags["C_CONTIGUOUS"]
    stark = T.stark_class(S, table)(4)
    w, ew = PL.WORDS[table]
    got = []
    for fn, arr in ((L.sbn_program_instances, n3), (L.sbn_program_m_instances, n4)):
        ios, outs = np.zeros((3, 4, 2 * w + ew), dtype=np.uint32), np.zeros((11, w), dtype=np.uint32)
        assert fn(stark.kind, arr.ctypes.data, 11, v.ctypes.data, len(v), e.ctypes.data, len(e), 4, ios.ctypes.data, outs.ctypes.data) == 0
        got.append((ios, outs))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    lv = []
    for fn, arr in ((L.sbn_program_levels, n3), (L.sbn_program_m_levels, n4)):
        level, depth = np.zeros(11, dtype=np.uint32), ctypes.c_uint32(0)
        assert fn(arr.ctypes.data, 11, level.ctypes.data, ctypes.addressof(depth)) == 0
        lv.append((level.tolist(), depth.value))
    assert lv[0] == lv[1] == G.levels(nodes)
    # the check: the same verdict and outputs on the honest public inputs, the same words of the same refusal on an edit
    ios, outs = got[0]
    padded = np.concatenate([outs, outs[-1:]])
    pis = [G.public_inputs(table, u, padded[4 * i:4 * i + 4]) for i, u in enumerate(ios)]
    bad = [p.copy() for p in pis]
    bad[1][0] ^= 1
    for these in (pis, bad):
        ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in these])
        res = []
        for fn, arr in ((L.sbn_program_check, n3), (L.sbn_program_m_check, n4)):
            o = np.zeros((11, w), dtype=np.uint32)
            rc = fn(stark.kind, 4, ptrs, 3, arr.ctypes.data, 11, v.ctypes.data, len(v), e.ctypes.data, len(e), o.ctypes.data)
            res.append((rc, L.sbn_last_error().decode() if rc else "", o.tolist() if rc == 0 else None))
        assert res[0] == res[1] and res[0][0] == (0 if these is pis else VERIFY_FAILED), res[0][:2]
    # the Python calls route a 4-column array to the _m calls
    i4, o4 = S.program_instances(stark, n4, v, e)
    assert np.array_equal(i4, ios) and np.array_equal(o4, outs)
    assert np.array_equal(S.program_check(stark, pis, n4, v, e), outs)
    assert S.program_levels(n4)[1] == lv[0][1]
    refused(S, BAD_ARG, "nodes must be", S.program_instances, stark, np.zeros((11, 5), dtype=np.uint32), v, e)
    refused(S, BAD_ARG, "nodes must be", S.program_levels, np.zeros((11, 2), dtype=np.uint32))


def test_zero_maps_refuse_as_the_twin(S):
    """The refusals of the twin, by the same words, through the _m call (kind, arguments, nodes, values)."""
    L = S.lib()
    v, e = np.zeros((2, 96), dtype=np.uint32), PL.exp_words("fq12u64", [1, PL.GLP])
    cases = [(S.AIR_G1_EXP, [(0, G.ONE, 0)], 1, 4), (S.AIR_FQ12_EXP_U64, None, 1, 4), (S.AIR_FQ12_EXP_U64, [(0, G.ONE, 0)], 0, 4),
             (S.AIR_FQ12_EXP_U64, [(0, G.ONE, 0)], 0x7FFFFFFF, 4), (S.AIR_FQ12_EXP_U64, [(0, G.ONE, 0)], 1, 0),
             (S.AIR_FQ12_EXP_U64, [(G.out(0), G.ONE, 0)], 1, 4), (S.AIR_FQ12_EXP_U64, [(2, G.ONE, 0)], 1, 4), (S.AIR_FQ12_EXP_U64, [(G.ONE, 0, 0)], 1, 4),
             (S.AIR_FQ12_EXP_U64, [(0, 0, 2)], 1, 4), (S.AIR_FQ12_EXP_U64, [(0, 0, 1)], 1, 4)]
    for kind, nodes, count, num_io in cases:
        res = []
        for cols, fn in ((3, L.sbn_program_instances), (4, L.sbn_program_m_instances)):
            arr = None if nodes is None else np.array([nd + (0,) * (cols - 3) for nd in nodes], dtype=np.uint32)
            rc = fn(kind, None if arr is None else arr.ctypes.data, count, v.ctypes.data, 2, e.ctypes.data, 2, num_io, None, None)
            res.append((rc, L.sbn_last_error().decode()))
        assert res[0] == res[1] and res[0][0] != 0, (kind, nodes, count, res)


# ---------------------------------------------------------------- 5. the added refusals, in the stated order
def test_added_refusals_in_order(S):
    L = S.lib()
    v = np.zeros((2, 96), dtype=np.uint32)
    v8 = np.zeros((2, 8), dtype=np.uint32)
    e = PL.exp_words("fq12", [1, 2])
    M = PM.maps_word

    def call(kind, nodes, fn=None):
        arr = np.array(nodes, dtype=np.uint32).reshape(-1, 4)
        vals = v8 if kind == S.AIR_FQ_EXP else v
        if fn == "levels":
            rc = L.sbn_program_m_levels(arr.ctypes.data, len(arr), None, None)
        else:
            rc = L.sbn_program_m_instances(kind, arr.ctypes.data, len(arr), vals.ctypes.data, 2, e.ctypes.data, 2, 4, None, None)
        return rc, L.sbn_last_error().decode()

    ok = (0, G.ONE, 0, 0)
    for kind in (S.AIR_FQ12_EXP, S.AIR_FQ12_EXP_U64, S.AIR_FQ_EXP):
        # the existing checks of the node come first: a bad exponent index beside every kind of bad map
        rc, msg = call(kind, [ok, (G.out(0), G.ONE, 2, 0x10000 | M(12, 0))])
        assert rc == BAD_ARG and re.search(r"node 1: exponent is index 2 of 2\b", msg), msg
        # bits 16..31, then a map above 11, then a map on a non-link; FQ_EXP's refusal is the last
        rc, msg = call(kind, [ok, (G.out(0), 1, 0, 0x10000 | M(12, 3))])
        assert rc == BAD_ARG and re.search(r"node 1: maps has bits 16\.\.31 set", msg), msg
        rc, msg = call(kind, [ok, (G.out(0), 1, 0, M(12, 3))])
        assert rc == BAD_ARG and re.search(r"node 1: the map of x is 12\b", msg), msg
        rc, msg = call(kind, [ok, (G.out(0), G.out(0), 0, M(11, 200))])
        assert rc == BAD_ARG and re.search(r"node 1: the map of offset is 200\b", msg), msg
        rc, msg = call(kind, [ok, (G.out(0), 1, 0, M(2, 3))])
        assert rc == BAD_ARG and re.search(r"node 1: offset carries map 3 and is no link", msg), msg
        rc, msg = call(kind, [ok, (1, G.out(0), 0, M(2, 3))])
        assert rc == BAD_ARG and re.search(r"node 1: x carries map 2 and is no link", msg), msg
        rc, msg = call(kind, [ok, (G.out(0), G.ONE, 0, M(2, 3))])
        assert rc == BAD_ARG and re.search(r"node 1: offset carries map 3 and is no link", msg), msg
        # an earlier node wins over a later one
        rc, msg = call(kind, [(0, G.ONE, 0, M(1, 0)), (G.out(0), G.ONE, 0, 0x10000)])
        assert rc == BAD_ARG and re.search(r"node 0: x carries map 1", msg), msg
    # the structural call knows no table: the three BAD_ARG refusals, and never FQ_EXP's
    rc, msg = call(None, [ok, (G.out(0), 1, 0, 0x80000000)], "levels")
    assert rc == BAD_ARG and re.search(r"node 1: maps has bits", msg), msg
    rc, msg = call(None, [ok, (G.out(0), 1, 0, M(0, 12))], "levels")
    assert rc == BAD_ARG and re.search(r"node 1: the map of offset is 12\b", msg), msg
    rc, msg = call(None, [ok, (G.out(0), 1, 0, M(0, 1))], "levels")
    assert rc == BAD_ARG and re.search(r"node 1: offset carries map 1", msg), msg
    assert call(None, [ok, (G.out(0), G.out(0), 0, M(1, 11))], "levels")[0] == 0
    # FQ_EXP: any non-zero map on a link is SBN_ERR_UNSUPPORTED, naming node and field; zero maps are accepted
    rc, msg = call(S.AIR_FQ_EXP, [ok, (G.out(0), G.ONE, 0, M(1, 0))])
    assert rc == UNSUPPORTED and re.search(r"node 1: x carries map 1", msg), msg
    rc, msg = call(S.AIR_FQ_EXP, [ok, (1, G.out(0), 0, M(0, 6))])
    assert rc == UNSUPPORTED and re.search(r"node 1: offset carries map 6", msg), msg
    assert call(S.AIR_FQ_EXP, [ok, (G.out(0), G.out(0), 1, 0)])[0] == 0
    for kind in (S.AIR_FQ12_EXP, S.AIR_FQ12_EXP_U64):
        assert call(kind, [ok, (G.out(0), G.out(0), 1, M(1, 11))])[0] == 0
    # a bad node before any value: literal 1 is >= p and node 1 has a bad map
    big = v.copy()
    big[1, 0:8] = PL.limbs(P, 8)
    arr = np.array([(1, G.ONE, 0, 0), (G.out(0), G.ONE, 0, M(12, 0))], dtype=np.uint32)
    assert L.sbn_program_m_instances(S.AIR_FQ12_EXP, arr.ctypes.data, 2, big.ctypes.data, 2, e.ctypes.data, 2, 4, None, None) == BAD_ARG
    assert re.search(r"node 1: the map of x is 12\b", L.sbn_last_error().decode())
    # the check refuses the same way, before it reads a public input
    assert L.sbn_program_m_check(S.AIR_FQ12_EXP, 4, None, 1, arr.ctypes.data, 2, v.ctypes.data, 2, e.ctypes.data, 2, None) == BAD_ARG
    assert re.search(r"node 1: the map of x is 12\b", L.sbn_last_error().decode())


# ---------------------------------------------------------------- 6. sbn_program_m_check
U64_PER, U64_X, U64_OFF, U64_EXP, U64_OUT = 577, 0, 192, 384, 385


@pytest.fixture(scope="module")
def checked(S, dag_case):
    """The mapped DAG on Fq12ExpU64Stark(4) with the public inputs of its four units from the unchanged host generator."""
    stark, nodes, values, exps, arr, ios, outs, _ = dag_case("fq12u64")
    return stark, nodes, values, exps, arr, outs, [stark.generate_public_inputs(u) for u in ios]


def pi_words(v):
    """The 192 public inputs (16-bit limbs) of an Fq12 value."""
    w = np.asarray(PL.elem_words("fq12", v), dtype=np.uint64)
    return np.stack([w & np.uint64(0xFFFF), w >> np.uint64(16)], axis=-1).reshape(-1)


def test_m_check_accepts_the_honest_public_inputs(S, checked):
    stark, nodes, values, exps, arr, outs, pis = checked
    assert np.array_equal(S.program_check(stark, pis, *arr), outs)
    assert all(np.array_equal(p, q) for p, q in zip(pis, PM.unit_public_inputs("fq12u64", *PM.explicit_units("fq12u64", nodes, values, exps, 4), 4)))
    n, v, e = arr
    ptrs = (ctypes.c_void_p * 4)(*[p.ctypes.data for p in pis])
    assert S.lib().sbn_program_m_check(stark.kind, 4, ptrs, 4, n.ctypes.data, 15, v.ctypes.data, 2, e.ctypes.data, 4, None) == 0


def test_m_check_recomputes_the_map(S, checked):
    stark, nodes, values, exps, arr, outs, pis = checked
    ev = PM.evaluate(nodes, values, exps)

    def with_field(g, at, value):
        bad = [p.copy() for p in pis]
        bad[g // 4][U64_PER * (g % 4) + at:U64_PER * (g % 4) + at + 192] = pi_words(value)
        return bad
    # node 2: x = frob_1(node 0).  The unmapped output, and the output mapped by m + 1, are both refused
    refused(S, VERIFY_FAILED, r"instance 2: x differs from frob_1 of the output of node 0\b", S.program_check, stark, with_field(2, U64_X, ev[0][2]), *arr)
    refused(S, VERIFY_FAILED, r"instance 2: x differs from frob_1 of the output of node 0\b", S.program_check, stark, with_field(2, U64_X, PM.frob(ev[0][2], 2)), *arr)
    # node 8: offset = frob_9(node 2), across a unit boundary; node 14: x = frob_7(node 13)
    refused(S, VERIFY_FAILED, r"instance 8: offset differs from frob_9 of the output of node 2\b", S.program_check, stark, with_field(8, U64_OFF, ev[2][2]), *arr)
    refused(S, VERIFY_FAILED, r"instance 8: offset differs from frob_9 of the output of node 2\b", S.program_check, stark, with_field(8, U64_OFF, PM.frob(ev[2][2], 10)), *arr)
    refused(S, VERIFY_FAILED, r"instance 14: x differs from frob_7 of the output of node 13\b", S.program_check, stark, with_field(14, U64_X, PM.frob(ev[13][2], 8)), *arr)
    # an unmapped link beside mapped ones still compares the words: node 7, x = node 4
    refused(S, VERIFY_FAILED, r"instance 7: x differs from the output of node 4\b", S.program_check, stark, with_field(7, U64_X, PM.frob(ev[4][2], 1)), *arr)
    # a caller who states another map than the prover used
    n2 = arr[0].copy()
    n2[2, 3] = PM.maps_word(2, 0)
    refused(S, VERIFY_FAILED, r"instance 2: x differs from frob_2 of the output of node 0\b", S.program_check, stark, pis, n2, arr[1], arr[2])
    n2[2, 3] = 0
    refused(S, VERIFY_FAILED, r"instance 2: x differs from the output of node 0\b", S.program_check, stark, pis, n2, arr[1], arr[2])


@pytest.mark.parametrize("g,at,value,names", [
    (0, U64_OUT + 7, None, r"instance 2: x differs from frob_1 of the output of node 0\b"),      # a tampered output: its first reader
    (13, U64_OUT, None, r"instance 14: x differs from frob_7 of the output of node 13\b"),
    (2, U64_OUT, 1 << 16, r"instance 2: output limb 0\b"),
    (15, U64_X + 3, None, r"instance 15 \(pad\): x differs from instance 14\b"),
    (15, U64_OFF + 190, None, r"instance 15 \(pad\): offset"),
    (15, U64_EXP, None, r"instance 15 \(pad\): exponent"),
    (15, U64_OUT + 1, None, r"instance 15 \(pad\): output"),
    (3, U64_X + 100, None, r"instance 3: x differs from frob_2 of the output of node 0\b"),
    (3, U64_OFF + 100, None, r"instance 3: offset differs from frob_3 of the output of node 0\b"),
], ids=["output_first", "output_late", "output_limb", "pad_x", "pad_offset", "pad_exponent", "pad_output", "mapped_x", "mapped_offset"])
def test_m_check_names_the_tampered_instance_field_node_and_map(S, checked, g, at, value, names):
    stark, _, _, _, arr, _, pis = checked
    bad = [p.copy() for p in pis]
    i = U64_PER * (g % 4) + at
    bad[g // 4][i] = value if value is not None else int(bad[g // 4][i]) ^ 1
    refused(S, VERIFY_FAILED, names, S.program_check, stark, bad, *arr)


# ---------------------------------------------------------------- the builder
def test_the_builder_composes_maps_and_maps_literals_natively(S, elements):
    stark = S.Fq12ExpU64Stark(4)
    f = elements[0]
    pg = S.Program(stark)
    lit = pg.value(words(f))
    h = pg.pow(lit, 3)
    assert pg.arrays()[0].shape == (1, 3)                                     # no map used: three columns, as before
    h5 = pg.frobenius(h, 5)
    assert (h5.ref, h5.node, h5.map) == (h.ref, 0, 5) and pg.frobenius(h5, 9).map == 2 and pg.conj(pg.conj(h)).map == 0 and pg.conj(h).map == 6
    c = pg.conj(lit)                                                          # a literal: mapped here, interned
    assert c.map == 0 and c.ref == 1 and pg.frobenius(lit, 6).ref == 1 and pg.frobenius(lit, 12).ref == lit.ref
    n1 = pg.pow(h5, 1, offset=pg.frobenius(h, 7))
    n2 = pg.mul(pg.conj(n1), c)
    nodes, values, exps = pg.arrays()
    assert nodes.shape == (3, 4) and nodes[:, 3].tolist() == [0, PM.maps_word(5, 7), PM.maps_word(6, 0)]
    assert elem(values[1]) == PM.frob(f, 6)
    _, outs = S.program_instances(stark, nodes, values, exps)
    f3 = PL.fq12_pow(f, 3)
    want1 = PL.fq12_mul(PM.frob(f3, 7), PM.frob(f3, 5))
    assert elem(outs[n1.node]) == want1 and elem(outs[n2.node]) == PL.fq12_mul(PM.frob(f, 6), PM.frob(want1, 6))
    refused(S, UNSUPPORTED, "Fq12", S.Program(S.FqExpStark(4)).frobenius, 5, 1)


# ---------------------------------------------------------------- 7. the final exponentiation
@pytest.fixture(scope="module")
def final_case(S):
    r = PL.rng(401)
    fs = [PL.random_elem("fq12", r), PL.random_elem("fq12", r)]
    stark = S.Fq12ExpU64Stark(16)
    progs = []
    for f in fs:
        pg = S.Program(stark)
        check, result = S.final_exponentiation(pg, words(f))
        progs.append((pg, check, result))
    return stark, fs, progs


def test_the_final_exponentiation_is_the_power(S, final_case):
    stark, fs, progs = final_case
    for f, (pg, check, result) in zip(fs, progs):
        assert len(pg) == S.FINAL_EXP_NODES == 16 and (check.node, result.node) == (0, 15)
        nodes, values, exps = pg.arrays()
        assert nodes.shape == (16, 4) and sorted(PL.from_limbs(e) for e in exps) == sorted(PM.FINAL_EXP_EXPS)
        ios, outs = S.program_instances(stark, nodes, values, exps)
        assert ios.shape == (1, 16, 194)
        assert elem(outs[result.node]) == PM.final_exp_value(f) == PL.fq12_pow(f, (P ** 12 - 1) // PM.R)
        assert elem(outs[check.node]) == PL.FQ12_ONE
        # the helper's table, node by node: the same rows and outputs, the same schedule
        hn, hv, he = PM.final_exp_program([f])
        units_want, outs_want = PM.explicit_units("fq12u64", hn, hv, he, 16)
        assert np.array_equal(ios, units_want) and np.array_equal(outs, outs_want)
        level, depth = S.program_levels(nodes)
        assert (level.tolist(), depth) == PM.levels(hn)
        # the maps of the normative table
        assert nodes[:, 3].tolist() == [nd[3] for nd in hn]


def test_the_final_exponentiation_is_a_program_of_the_u64_table(S, elements):
    for stark in (S.Fq12ExpStark(16), S.FqExpStark(16)):
        with pytest.raises(S.SbnError):
            S.final_exponentiation(S.Program(stark), words(elements[0]))


def test_a_wrong_inverse_shows_at_node_zero(S, final_case):
    """f_inv is a claim: with another element the program is still a program, node 0 is not one, and the check of the public inputs
    -- hand-built here from the library's own list -- accepts them as what they are (the verify helper then names the input)."""
    stark, fs, _ = final_case
    f, wrong = fs[0], PM.fq12_inverse(fs[1])
    pg = S.Program(stark)
    check, result = S.final_exponentiation(pg, words(f), words(wrong))
    arr = pg.arrays()
    ios, outs = S.program_instances(stark, *arr)
    assert elem(outs[check.node]) == PL.fq12_mul(f, wrong) != PL.FQ12_ONE
    pis = [G.public_inputs("fq12u64", ios[0], outs)]
    assert np.array_equal(pis[0], stark.generate_public_inputs(ios[0]))
    assert np.array_equal(S.program_check(stark, pis, *arr), outs)
    assert elem(S.program_check(stark, pis, *arr)[0]) != PL.FQ12_ONE
    # the x public inputs of node 0 are the claimed inverse, which is how the verify helper reads it back
    x = pis[0][:192]
    assert elem((x[0::2] | (x[1::2] << np.uint64(16))).astype(np.uint32)) == wrong
    # the honest program against these public inputs: the literal of node 0 differs
    honest = S.Program(stark)
    S.final_exponentiation(honest, words(f))
    refused(S, VERIFY_FAILED, r"instance 0: x differs from the caller's literal", S.program_check, stark, pis, *honest.arrays())
