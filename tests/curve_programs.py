"""Curve programs (include/sbn.h, "Curve programs") over Python integers, for tests/test_curve_program_host.py and
tests/test_curve_program_gpu.py: a program is evaluated node by node with the affine curve arithmetic, the start candidates and
kill() of tests/complete_sums.py (out, value and blind per node; a bad event is judged by Python's own walk of the table), the
one start of the program is the smallest candidate without a bad event, and the result is laid out as the explicit padded list it
stands for.  Nodes are (x, offset, exp) tuples: x an index into `points` (Python points) or OUT | j, offset an index, OUT | j or
START; exp an index into `exps` (Python ints).  Python integers are the reference, never the code under test."""
import functools

import numpy as np

import chained_lists as CL
import complete_sums as CS
import oracle_lib as O
import program_lists as PG
import tracegen_edges as T

OUT, START, ONE = 0x80000000, 0x7FFFFFFE, 0x7FFFFFFF
R = T.R
CURVES = ["g1", "g2"]
W = {"g1": 16, "g2": 32}


def out(j):
    return OUT | j


def is_link(v):
    return bool(v & OUT)


def levels(nodes):
    """The level rule of tests/program_lists.py; START is no link."""
    return PG.levels(nodes)


def evaluate(curve, nodes, points, exps, start):
    """(rows, bad): rows[g] = (x, offset, out, v, T) in Python points (None: the point at infinity) for the nodes before the first
    bad event, bad = the first node with one (an offset or an output at infinity, an addition of the table's walk with B = +-A) or
    None."""
    add, _, mul = T._ops(curve)
    rows = []
    for g, (x, off, e) in enumerate(nodes):
        assert all(not is_link(v) or (v & ~OUT) < g for v in (x, off)) and x not in (START, ONE) and off != ONE, g
        xv, vx, tx = (rows[x & ~OUT][2], rows[x & ~OUT][3], rows[x & ~OUT][4]) if is_link(x) else (points[x], points[x], None)
        if is_link(off):
            ov, vo, to = rows[off & ~OUT][2], rows[off & ~OUT][3], rows[off & ~OUT][4]
        elif off == START:
            ov, vo, to = start, None, start
        else:
            ov, vo, to = points[off], points[off], None
        if ov is None:
            return rows, g
        o, t = T.curve_walk(curve, xv, ov, exps[e])
        if t is not None or o is None:
            return rows, g
        rows.append((xv, ov, o, add(vo, mul(vx, exps[e]) if vx is not None else None), add(to, mul(tx, exps[e]) if tx is not None else None)))
    return rows, None


def choose(curve, nodes, points, exps):
    """(choice, rows) with the smallest candidate from which no node has a bad event; (None, first bad node of candidate 7)."""
    bad = None
    for j, h in enumerate(CS.candidates(curve)):
        rows, bad = evaluate(curve, nodes, points, exps, h)
        if bad is None:
            return j, rows
    return None, bad


def point_words(curve, p):
    return [0] * W[curve] if p is None else [int(t) for t in CL.value_words(curve, p)]


def arrays(curve, nodes, points, exps):
    """(nodes (count, 3), points (n, W), exps (n, 8)) uint32, as the calls take them."""
    return (np.array(nodes, dtype=np.uint32).reshape(-1, 3), np.array([point_words(curve, p) for p in points], dtype=np.uint32).reshape(-1, W[curve]),
            np.array([T.limbs(e, 8, 32) for e in exps], dtype=np.uint32).reshape(-1, 8))


def model(curve, nodes, points, exps, num_io):
    """(ios (units, num_io, 2W + 8), outs, values (count, W), infinity (count,), choice) in words."""
    add, neg, _ = T._ops(curve)
    choice, rows = choose(curve, nodes, points, exps)
    assert choice is not None, "the program exhausts the candidates"
    ios = [point_words(curve, xv) + point_words(curve, ov) + T.limbs(exps[nd[2]], 8, 32) for nd, (xv, ov, _, _, _) in zip(nodes, rows)]
    while len(ios) % num_io:
        ios.append(ios[-1])
    vals = [add(o, neg(t)) if t is not None else o for _, _, o, _, t in rows]
    assert vals == [r[3] for r in rows]   # out - T is the value the program means
    return (np.array(ios, dtype=np.uint32).reshape(-1, num_io, 2 * W[curve] + 8), np.array([point_words(curve, r[2]) for r in rows], dtype=np.uint32),
            np.array([point_words(curve, v) for v in vals], dtype=np.uint32), np.array([v is None for v in vals], dtype=np.uint8), choice)


def public_inputs(unit_ios, unit_outs):
    """The public inputs of one unit from its rows and outputs in words: x, offset, exponent, output per instance as u32 limbs (what
    the generators of the curve tables state)."""
    return np.ascontiguousarray(np.concatenate([np.asarray(unit_ios, dtype=np.uint64), np.asarray(unit_outs, dtype=np.uint64)], axis=1).reshape(-1))


def unit_public_inputs(ios, outs):
    """One array per unit; the pads repeat the last output."""
    num_io = ios.shape[1]
    padded = np.concatenate([outs] + [outs[-1:]] * (ios.shape[0] * num_io - len(outs)))
    return [public_inputs(u, padded[num_io * i:num_io * (i + 1)]) for i, u in enumerate(ios)]


# ---------------------------------------------------------------- the case recipes
def _rnd(curve, rng):
    return O.g1_random(rng) if curve == "g1" else O.g2_random(rng)


def _exp(rng):
    return int.from_bytes(rng.bytes(32), "little") % R


@functools.lru_cache(maxsize=None)
def cases(curve):
    """{name: (nodes, points, exps)}, benign (every one must come out with choice 0: asserted by the host tests on the CPU):
      single     one node from START;
      chain      offset = OUT(g - 1), the chained list;
      tower      e3 (e2 (e1 P)), x-links of depth 3;
      diamond    two multiples of one node, then their combination with both operands linked;
      lincomb    a S1 + b S2 of two earlier sums, each a chain of two terms;
      infinity   P, then (r - 1) P + OUT(0): a value at infinity (G1: the twist points are off the subgroup, there the value is a point);
      literal    a node whose x and offset are literals (T = O, value = out), and a multiple of it."""
    rng = np.random.default_rng({"g1": 61, "g2": 62}[curve])
    p = [_rnd(curve, rng) for _ in range(6)]
    e = [_exp(rng) for _ in range(6)]
    c = {}
    c["single"] = ([(0, START, 0)], p[:1], e[:1])
    c["chain"] = ([(k, START if k == 0 else out(k - 1), k) for k in range(5)], p[:5], e[:5])
    c["tower"] = ([(0, START, 0), (out(0), START, 1), (out(1), START, 2)], p[:1], e[:3])
    c["diamond"] = ([(0, START, 0), (out(0), START, 1), (out(0), 1, 2), (out(1), out(2), 3)], p[:2], e[:4])
    c["lincomb"] = ([(0, START, 0), (1, out(0), 1), (2, START, 2), (3, out(2), 3), (out(1), START, 4), (out(3), out(4), 5)], p[:4], e)
    c["infinity"] = ([(0, START, 0), (0, out(0), 1)], p[:1], [1, R - 1])
    c["literal"] = ([(0, 1, 0), (out(0), START, 1), (2, out(0), 2)], p[:3], e[:3])
    return c


def wide(curve, count, seed=71):
    """`count` nodes in three levels: a level of literals from START, a middle level that continues each from a partner, one last
    node per pair that multiplies a result; with count = 300 and num_io = 128 links cross both unit boundaries."""
    rng = np.random.default_rng(seed)
    a = count // 3
    b = (count - a) // 2
    pts = [_rnd(curve, rng) for _ in range(8)]
    exps = [_exp(rng) for _ in range(8)]
    nodes = [(g % 8, START, (3 * g) % 8) for g in range(a)]
    nodes += [((g + 1) % 8, out((7 * g) % a), (g + 2) % 8) for g in range(b)]
    nodes += [(out(a + (5 * g) % b), out((11 * g) % a), (g + 5) % 8) for g in range(count - a - b)]
    return nodes, pts, exps


def independent(curve, count, seed=72):
    """`count` nodes without links: one level."""
    rng = np.random.default_rng(seed)
    pts = [_rnd(curve, rng) for _ in range(4)]
    exps = [_exp(rng) for _ in range(5)]
    return [(g % 4, START if g % 3 else (g + 1) % 4, g % 5) for g in range(count)], pts, exps


def narrow_waist(curve, seed=73):
    """A level holding exactly one node between two wide levels: 20 nodes, one node that links to two of them, 20 nodes behind it."""
    rng = np.random.default_rng(seed)
    pts = [_rnd(curve, rng) for _ in range(4)]
    exps = [_exp(rng) for _ in range(4)]
    nodes = [(g % 4, START, g % 4) for g in range(20)]
    nodes.append((out(3), out(17), 1))
    nodes += [(g % 4, out(20), (g + 1) % 4) if g % 2 else (out(20), START, g % 4) for g in range(20)]
    assert levels(nodes)[0] == [0] * 20 + [1] + [2] * 20
    return nodes, pts, exps


@functools.lru_cache(maxsize=None)
def killing(curve, j):
    """A program whose candidates 0 .. j - 1 each meet a bad event at a node of level 1, so that its choice is j (j = 8: every
    candidate fails, candidate 7 at node 8).  Node 0 = e0 P from START; node k = 1 .. j adds the literal x_k = H_(k-1) + e0 P
    (complete_sums.kill) to OUT(0) with exponent 1: under candidate k - 1 the table's first addition meets B = A.  A benign node
    follows the kills."""
    rng = np.random.default_rng(80 + j)
    p, q, e0 = _rnd(curve, rng), _rnd(curve, rng), _exp(rng)
    points = [p, q] + [CS.kill(curve, k, [p], [e0]) for k in range(j)]
    exps = [e0, 1, _exp(rng)]
    nodes = [(0, START, 0)] + [(2 + k, out(0), 1) for k in range(j)] + [(1, out(0), 2)]
    assert all(lv == (0 if g == 0 else 1) for g, lv in enumerate(levels(nodes)[0]))
    choice, rows = choose(curve, nodes, points, exps)
    if j < CS.CANDIDATES:
        assert choice == j
        for k in range(j):                                       # candidate k fails at node k + 1, a node of level 1
            assert evaluate(curve, nodes, points, exps, CS.candidates(curve)[k])[1] == k + 1
    else:
        assert choice is None and rows == CS.CANDIDATES
    return nodes, points, exps


def literal_trap(curve):
    """A node whose operands are literals and whose table walk no start can mend: x + x with exponent 1 (B = A), behind a benign node."""
    rng = np.random.default_rng(91)
    p, q = _rnd(curve, rng), _rnd(curve, rng)
    return [(0, START, 0), (1, 1, 1)], [p, q], [_exp(rng), 1]
