"""Field programs over Python integers, for tests/test_program_host.py and tests/test_program_gpu.py: a program is evaluated node
by node with the Fq and Fq12 arithmetic of tests/power_lists.py (output = offset * x^e), laid out as the explicit padded list it
stands for, and scheduled by the ten-line level rule.  Nodes are (x, offset, exp) tuples: x / offset an index into `values`
(Python field elements), OUT | j for the output of node j, offset also ONE; exp an index into `exps` (Python ints)."""
import numpy as np

import power_lists as PL

OUT, ONE = 0x80000000, 0x7FFFFFFF


def out(j):
    return OUT | j


def is_link(v):
    return bool(v & OUT)


def one(table):
    return 1 if table == "fq" else list(PL.FQ12_ONE)


def mul(table, a, b):
    return a * b % PL.P if table == "fq" else PL.fq12_mul(a, b)


def resolve(table, v, values, outs):
    if is_link(v):
        return outs[v & ~OUT]
    return one(table) if v == ONE else values[v]


def evaluate(table, nodes, values, exps):
    """[(x, offset, output)] per node, as Python values."""
    rows, outs = [], []
    for g, (x, off, e) in enumerate(nodes):
        assert all(not is_link(v) or (v & ~OUT) < g for v in (x, off)) and x != ONE, g
        xv, ov = resolve(table, x, values, outs), resolve(table, off, values, outs)
        outs.append(mul(table, ov, PL.power(table, xv, exps[e])))
        rows.append((xv, ov, outs[-1]))
    return rows


def levels(nodes):
    """(level per node, depth): 0 without links, otherwise 1 + the largest level linked to."""
    level = []
    for x, off, _ in nodes:
        linked = [level[v & ~OUT] for v in (x, off) if is_link(v)]
        level.append(1 + max(linked) if linked else 0)
    return level, 1 + max(level)


def arrays(table, nodes, values, exps):
    """(nodes (count, 3), values (n, W), exps (n, ew)) uint32, as the calls take them."""
    w, ew = PL.WORDS[table]
    return (np.array(nodes, dtype=np.uint32).reshape(-1, 3), np.array([PL.elem_words(table, v) for v in values], dtype=np.uint32).reshape(-1, w),
            np.array([PL.limbs(e, ew) for e in exps], dtype=np.uint32).reshape(-1, ew))


def explicit_units(table, nodes, values, exps, num_io):
    """(units, outs) in words: row g = (x, offset, exponent of node g) with every link resolved, the last unit padded with copies of
    the last row; outs (count, W)."""
    w, ew = PL.WORDS[table]
    ev = evaluate(table, nodes, values, exps)
    rows = [PL.elem_words(table, xv) + PL.elem_words(table, ov) + PL.limbs(exps[nd[2]], ew) for nd, (xv, ov, _) in zip(nodes, ev)]
    while len(rows) % num_io:
        rows.append(rows[-1])
    return (np.array(rows, dtype=np.uint32).reshape(-1, num_io, 2 * w + ew), np.array([PL.elem_words(table, o) for _, _, o in ev], dtype=np.uint32))


def public_inputs(table, unit_ios, unit_outs):
    """The public inputs of one unit from its rows and outputs in words: x, offset, exponent, output per instance; u32 limbs in Fq,
    16-bit limbs in Fq12, the exponent as eight u32 words or one u64 (what the host generators state; FqExpStark has none below 2^16
    rows)."""
    w, ew = PL.WORDS[table]

    def limbs(a):
        a = np.asarray(a, dtype=np.uint64)
        return a if table == "fq" else np.stack([a & np.uint64(0xFFFF), a >> np.uint64(16)], axis=-1).reshape(a.shape[0], -1)
    rows, outs = np.asarray(unit_ios, dtype=np.uint64), np.asarray(unit_outs)
    e = rows[:, 2 * w:]
    if ew == 2:
        e = (e[:, 0] | (e[:, 1] << np.uint64(32))).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([limbs(rows[:, :w]), limbs(rows[:, w:2 * w]), e, limbs(outs)], axis=1).reshape(-1))


def zero(table):
    return 0 if table == "fq" else [0] * 12


def dag(table, seed=77):
    """The fixed DAG of the tests: 11 nodes (3 units of 4 with one pad).  Literals 0 and 1 are random, literal 2 is zero; exponent 0
    is zero, exponent 1 is one, exponents 2 and 3 fill the exponent field (3 is p itself, the Frobenius map, where it fits).
    dag_properties() states what the shape must hold."""
    r = PL.rng(seed)
    values = [PL.random_elem(table, r), PL.random_elem(table, r), zero(table)]
    exps = [0, 1, PL.BN_X, r.randrange(1 << 63, PL.GLP)] if table == "fq12u64" else [0, 1, r.randrange(1 << 255, 1 << 256), PL.P]
    nodes = [
        (0, ONE, 2),            # 0: a literal and one
        (1, 0, 1),              # 1: literal 0 again, exponent one: a plain product
        (out(0), ONE, 3),       # 2: an x-link
        (1, out(0), 2),         # 3: an offset-link, three back
        (out(2), out(3), 1),    # 4: both links, to different nodes, across the unit boundary
        (out(4), out(4), 3),    # 5: both links to the same node
        (2, out(1), 2),         # 6: a zero base
        (out(5), ONE, 0),       # 7: a zero exponent
        (2, out(5), 0),         # 8: 0^0 = 1, across the second boundary
        (out(6), out(8), 1),    # 9: a derived zero as x
        (out(9), out(2), 3),    # 10: far back
    ]
    return nodes, values, exps


def dag_properties(nodes, values, exps, num_io):
    """The set of properties the fixed DAG holds, by name (the tests assert that none is missing)."""
    have = set()
    uses, literal_uses = {}, {}
    for g, (x, off, e) in enumerate(nodes):
        lx, lo = is_link(x), is_link(off)
        if lx and not lo:
            have.add("x_link")
        if lo and not lx:
            have.add("offset_link")
        if lx and lo:
            have.add("both_links_same" if x == off else "both_links_different")
        for v in {x, off}:
            if is_link(v):
                j = v & ~OUT
                uses.setdefault(j, set()).add(g)
                if j // num_io != g // num_io:
                    have.add("crosses_unit")
                if g - j > 1:
                    have.add("more_than_one_back")
        for v in (x, off):
            if not is_link(v) and v != ONE:
                literal_uses[v] = literal_uses.get(v, 0) + 1
        if off == ONE:
            have.add("one")
        if not lx and values[x] in (0, [0] * 12):
            have.add("zero_base")
        if exps[e] == 0:
            have.add("zero_exponent")
        if exps[e] == 1:
            have.add("exponent_one")
    if any(len(u) >= 2 for u in uses.values()):
        have.add("output_used_twice")
    if any(n >= 2 for n in literal_uses.values()):
        have.add("literal_used_twice")
    return have


DAG_PROPERTIES = {"x_link", "offset_link", "both_links_different", "both_links_same", "output_used_twice", "literal_used_twice", "crosses_unit",
                  "more_than_one_back", "zero_base", "zero_exponent", "exponent_one", "one"}


def towers_as_program(count, depth, shared_exp):
    """The nodes of `count` towers of `depth` (tower-major), literal k the base of tower k, exponent k (or 0 when shared)."""
    return [(k if l == 0 else out(k * depth + l - 1), ONE, 0 if shared_exp else k) for k in range(count) for l in range(depth)]


def chain_as_program(count):
    """The nodes of a chained list: x = literal 1 + k, offset = the literal start (0), then the previous output; exponent k."""
    return [(1 + k, 0 if k == 0 else out(k - 1), k) for k in range(count)]
