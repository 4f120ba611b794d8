"""Chained instance lists (offset[0] = start, offset[k+1] = output[k]: the reference's *_msm call shape) for the five Exp tables,
derived in plain Python integers.  Shared by test_chained_host.py and test_chained_gpu.py.

Python integers (oracle_lib's g1_add / g2_add / fq12_mul and pow, through tracegen_edges) are the reference for every offset and
output, never the code under test.  The offsets are derived by Python's own scalar multiplication and addition (complete: None is
the point at infinity); whether the TABLE can walk the resulting explicit list is a separate question, answered by curve_walk."""
import functools

import numpy as np

import oracle_lib as O
import tracegen_edges as T

P, R, U256 = T.P, T.R, T.U256
START = {"g1": T.G1_GEN, "g2": T.G2_GEN}
ONE12 = [1] + [0] * 11


def _flat(table, v):
    """A value (point or field element) of the table as the list of its Fq components, in io order."""
    if table == "g1":
        return [v[0], v[1]]
    if table == "g2":
        return [v[0][0], v[0][1], v[1][0], v[1][1]]
    return [v] if table == "fq" else list(v)


def value_words(table, v):
    row = []
    for c in _flat(table, v):
        row += T.limbs(c, 8, 32)
    return np.array(row, dtype=np.uint32)


def terms_words(table, xs, es):
    """[count][T] u32: an instance row without its offset words (x, then exp_val)."""
    ew = 2 if table == "fq12u64" else 8
    return np.array([list(value_words(table, x)) + T.limbs(e, ew, 32) for x, e in zip(xs, es)], dtype=np.uint32)


def derive(table, xs, es, start):
    """(insts, final): the explicit list [(x, offset, e)] and the last output, in Python integers.  A curve offset of None is the
    point at infinity (such a list has no explicit form)."""
    insts, off = [], start
    for x, e in zip(xs, es):
        insts.append((x, off, e))
        if table in ("g1", "g2"):
            add, _, mul = T._ops(table)
            off = add(off, mul(x, e))
        elif table == "fq":
            off = off * pow(x, e, P) % P
        else:
            off = O.fq12_mul(off, O.fq12_pow(x, e))
    return insts, off


def walk_all(curve, insts):
    """First (instance, step) at which the table's own walk of the explicit list is degenerate, or None."""
    for k, inst in enumerate(insts):
        if inst[1] is None:
            return (k, -1)
        t = T.curve_walk(curve, *inst)[1]
        if t is not None:
            return (k, t)
    return None


@functools.lru_cache(maxsize=None)
def seeded_curve_list(curve):
    """The 128-instance list of the issue (np.random.default_rng(7)): random points and exponents mod r from the generator, with
    e = 0, x = start, a repeated instance, an instance and its negative, e = r, e = 2^256 - 1, e = 1 and a last instance with e = 0.
    Returns (xs, es, start, insts, final); the walk of the explicit list is asserted clean here, so a changed recipe cannot
    silently drop a case."""
    rng = np.random.default_rng(7)
    rnd = O.g1_random if curve == "g1" else O.g2_random
    neg = T.g1_neg if curve == "g1" else T.g2_neg
    start = START[curve]
    xs, es = [], []
    for _ in range(128):
        xs.append(rnd(rng))
        es.append(int.from_bytes(rng.bytes(32), "little") % R)
    es[1] = 0
    xs[2] = start
    xs[4], es[4] = xs[3], es[3]
    xs[6], es[6] = neg(xs[5]), es[5]
    es[7] = R
    es[8] = U256
    es[9] = 1
    xs[127], es[127] = xs[0], 0
    insts, final = derive(curve, xs, es, start)
    assert walk_all(curve, insts) is None and final is not None
    _, _, mul = T._ops(curve)
    identity = [k for k in range(128) if mul(xs[k], es[k]) is None]
    assert identity == ([1, 7, 127] if curve == "g1" else [1, 127]), identity   # r x = O on G1 only: the twist points are off the subgroup
    return xs, es, start, insts, final


@functools.lru_cache(maxsize=None)
def seeded_field_list(table, count=16):
    """`count` instances of a field table: x among 0, one, p-1 in one coefficient and random values; exponents 0, 1 and the
    edge exponents of the table."""
    rng = np.random.default_rng(11)
    rand = lambda: int.from_bytes(rng.bytes(32), "little") % P   # noqa: E731
    exps = [0, 1] + (T.EXPONENTS_U64 if table == "fq12u64" else T.EXPONENTS)
    if table == "fq":
        bases = [0, 1, P - 1, rand(), rand(), 2, rand()]
        start = rand()
    else:
        single = lambda j, c: [c if i == j else 0 for i in range(12)]   # noqa: E731
        bases = [[0] * 12, ONE12, single(0, P - 1), single(7, P - 1), [rand() for _ in range(12)], [rand() for _ in range(12)],
                 single(6, 1)]
        start = [rand() for _ in range(12)]
    xs = [bases[k % len(bases)] for k in range(count)]
    es = [exps[(3 * k + k // len(bases)) % len(exps)] for k in range(count)]
    xs[0], es[0] = bases[0], 0            # 0^0 = 1: the running product survives a zero base
    # keep the product non-zero for most of the list: a zero base with a non-zero exponent only near the end
    for k in range(1, count - 2):
        if es[k] and xs[k] == bases[0]:
            xs[k] = bases[4]
    xs[count - 2], es[count - 2] = bases[0], 3
    insts, final = derive(table, xs, es, start)
    return xs, es, start, insts, final


def chained_list(table, count=None):
    """(terms, start_words, insts, final) of the table's seeded list."""
    if table in ("g1", "g2"):
        xs, es, start, insts, final = seeded_curve_list(table)
    else:
        xs, es, start, insts, final = seeded_field_list(table, count or T.SHAPE[table][0])
    return terms_words(table, xs, es), value_words(table, start), insts, final


@functools.lru_cache(maxsize=None)
def witness_refusals(curve):
    """Lists the derivation must refuse with SBN_ERR_WITNESS, and an accepted twin: from the seeded list
      'opposite'  x[0] = -start, e[0] = 1: offset[1] is the point at infinity;
      'collide'   instance k = 5 takes x[k] = offset[k] (in Python) and an odd exponent: the table's first addition meets B = A;
      'twin'      the same with bit 0 of that exponent cleared: walked clean by curve_walk, accepted.
    Returns {name: (xs, es, start)}."""
    xs, es, start, insts, _ = seeded_curve_list(curve)
    neg = T.g1_neg if curve == "g1" else T.g2_neg
    out = {"opposite": ([neg(start)] + list(xs[1:]), [1] + list(es[1:]), start)}
    for k in range(5, 128):   # the first instance from 5 on whose twin walks clean
        odd = es[k] | 1
        cx = list(xs)
        cx[k] = insts[k][1]
        ce, te = list(es), list(es)
        ce[k], te[k] = odd, odd & ~1
        twin, final = derive(curve, cx, te, start)
        if final is not None and walk_all(curve, twin) is None:
            break
    else:
        raise AssertionError("no instance with a clean twin")
    bad, _ = derive(curve, cx, ce, start)
    assert walk_all(curve, bad) == (k, 0)
    out["collide"] = (cx, ce, start)
    out["twin"] = (cx, te, start)
    return out
