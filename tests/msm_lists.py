"""Chained lists longer than one table (two full units and a partial one) for the five Exp tables, derived in plain Python
integers through chained_lists.derive.  Shared by test_msm_host.py and test_msm_gpu.py.

Curves and Fq: num_io = 128, count = 261; Fq12 and Fq12U64: num_io = 16, count = 35.  The padded list is the reference's
g1_exp_circuit shape (src/curves/g1/circuit.rs:273-277): the last unit is filled with copies of the last real instance."""
import functools

import numpy as np

import chained_lists as CL
import oracle_lib as O
import tracegen_edges as T

P, R = T.P, T.R
SIZES = {"g1": (128, 261), "g2": (128, 261), "fq": (128, 261), "fq12": (16, 35), "fq12u64": (16, 35)}   # (num_io, count)


def num_units(count, num_io):
    return -(-count // num_io)


@functools.lru_cache(maxsize=None)
def curve_list(curve):
    """261 instances (np.random.default_rng(23)): random points and exponents mod r, with
      e = 0 at instance 3; x, -x with equal exponents at instances 5, 6 (unit 0);
      unit 1 (instances 128 .. 255) = 64 such pairs, so its total is the identity and offset[256] = offset[128];
      a last real instance (260) with e = 0.
    Returns (xs, es, start, insts, final); the recipe's properties and a clean walk are asserted here."""
    num_io, count = SIZES[curve]
    rng = np.random.default_rng(23)
    rnd = O.g1_random if curve == "g1" else O.g2_random
    neg = T.g1_neg if curve == "g1" else T.g2_neg
    start = CL.START[curve]
    xs = [rnd(rng) for _ in range(count)]
    es = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(count)]
    es[3] = 0
    xs[6], es[6] = neg(xs[5]), es[5]
    for k in range(num_io, 2 * num_io, 2):
        xs[k + 1], es[k + 1] = neg(xs[k]), es[k]
    es[count - 1] = 0
    insts, final = CL.derive(curve, xs, es, start)
    assert CL.walk_all(curve, insts) is None and final is not None
    assert insts[2 * num_io][1] == insts[num_io][1] and insts[7][1] == insts[5][1]    # the carry passes through + O
    assert insts[4][1] == insts[3][1] and final == insts[count - 1][1]
    return xs, es, start, insts, final


@functools.lru_cache(maxsize=None)
def field_list(table):
    """A field list of SIZES[table] (np.random.default_rng(29)): random bases, the edge exponents of the table and random ones;
    a zero base with exponent 0 in unit 0 (instance 2: 0^0 = 1) and a zero base with a non-zero exponent in the last unit,
    after the second boundary (instance 2 num_io + 1: the running product is zero from there on)."""
    num_io, count = SIZES[table]
    rng = np.random.default_rng(29)
    rand = lambda: int.from_bytes(rng.bytes(32), "little") % P   # noqa: E731
    u64 = table == "fq12u64"
    edge = T.EXPONENTS_U64 if u64 else T.EXPONENTS
    zero = 0 if table == "fq" else [0] * 12
    base = rand if table == "fq" else (lambda: [rand() for _ in range(12)])
    xs = [base() for _ in range(count)]
    es = [edge[k % len(edge)] if k % 3 else (rand() % (T.GLP if u64 else 1 << 256)) for k in range(count)]
    start = base()
    xs[2], es[2] = zero, 0
    z = 2 * num_io + 1
    xs[z], es[z] = zero, 3
    insts, final = CL.derive(table, xs, es, start)
    assert insts[3][1] == insts[2][1] and insts[z][1] != zero and insts[z + 1][1] == zero and final == zero
    return xs, es, start, insts, final


def msm_list(table):
    """(terms, start_words, insts, final, ios_units): the seeded list of the table in the words of the C ABI, Python's explicit list
    and last output, and the padded, unit-cut list (units, num_io, words) Python expects."""
    xs, es, start, insts, final = curve_list(table) if table in ("g1", "g2") else field_list(table)
    return CL.terms_words(table, xs, es), CL.value_words(table, start), insts, final, padded_units(table, insts, SIZES[table][0])


def padded_units(table, insts, num_io):
    ios = T.pack(table, insts)
    pad = num_units(len(insts), num_io) * num_io - len(insts)
    if pad:
        ios = np.concatenate([ios, np.repeat(ios[-1:], pad, axis=0)])
    return np.ascontiguousarray(ios.reshape(-1, num_io, ios.shape[1]))


@functools.lru_cache(maxsize=None)
def boundary_infinity(curve):
    """The curve list with x[127] = -offset[127], e[127] = 1: offset[128], the carry into unit 1, is the point at infinity."""
    xs, es, start, insts, _ = curve_list(curve)
    neg = T.g1_neg if curve == "g1" else T.g2_neg
    num_io = SIZES[curve][0]
    xs, es = list(xs), list(es)
    xs[num_io - 1], es[num_io - 1] = neg(insts[num_io - 1][1]), 1
    bad, _ = CL.derive(curve, xs[:num_io], es[:num_io], start)
    assert bad[num_io - 1][1] == insts[num_io - 1][1]
    add, _, mul = T._ops(curve)
    assert add(bad[-1][1], mul(xs[num_io - 1], 1)) is None
    return CL.terms_words(curve, xs, es), CL.value_words(curve, start)
