"""Mapped field programs over Python integers, for tests/test_program_maps_host.py and tests/test_program_maps_gpu.py, on top of
tests/program_lists.py and tests/power_lists.py: the Frobenius maps of Fq12 by their closed form in the flat basis, programs whose
links carry a map (nodes are (x, offset, exp, maps) tuples, maps = map of x | map of offset << 8), the normative 16-node final
exponentiation of include/sbn.h, and a seeded mapped DAG with the properties the tests name."""
import numpy as np

import power_lists as PL
import program_lists as PG

P, OUT, ONE, out = PL.P, PG.OUT, PG.ONE, PG.out
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
XI = (9, 1)
FINAL_EXP_NODES = 16


def f2pow(a, e):
    acc = (1, 0)
    for t in range(e.bit_length() - 1, -1, -1):
        acc = PL._f2mul(acc, acc)
        if (e >> t) & 1:
            acc = PL._f2mul(acc, a)
    return acc


_G = {}


def gamma(m, k):
    """G[m][k] = xi^(k (p^m - 1) / 6) in Fq2."""
    if (m, k) not in _G:
        _G[(m, k)] = f2pow(XI, k * (P ** m - 1) // 6)
    return _G[(m, k)]


def frob(f, m):
    """f^(p^m), m in 0..11, by the closed form: coefficient k becomes conj^m(a_k) * G[m][k], a_k = c[k] + c[k+6] i."""
    assert 0 <= m < 12
    res = [0] * 12
    for k in range(6):
        a = (f[k], (-f[k + 6]) % P if m & 1 else f[k + 6])
        res[k], res[k + 6] = PL._f2mul(a, gamma(m, k))
    return res


def maps_word(mx=0, mo=0):
    return mx | (mo << 8)


def evaluate(nodes, values, exps):
    """[(x, offset, output)] per node as Python values, x and offset AFTER their maps (the words of the explicit list)."""
    rows, outs = [], []
    for g, (x, off, e, maps) in enumerate(nodes):
        ops = []
        for v, m in ((x, maps & 0xFF), (off, (maps >> 8) & 0xFF)):
            assert maps >> 16 == 0 and m < 12 and (m == 0 or PG.is_link(v)), g
            assert not PG.is_link(v) or (v & ~OUT) < g, g
            w = PG.resolve("fq12", v, values, outs)
            ops.append(frob(w, m) if m else w)
        outs.append(PL.fq12_mul(ops[1], PL.fq12_pow(ops[0], exps[e])))
        rows.append((ops[0], ops[1], outs[-1]))
    return rows


def levels(nodes):
    return PG.levels([nd[:3] for nd in nodes])


def arrays(table, nodes, values, exps):
    """(nodes (count, 4), values (n, 96), exps (n, ew)) uint32, as the calls take them."""
    _, v, e = PG.arrays(table, [nd[:3] for nd in nodes], values, exps)
    return np.array(nodes, dtype=np.uint32).reshape(-1, 4), v, e


def explicit_units(table, nodes, values, exps, num_io):
    """(units, outs) in words: row g = (mapped x, mapped offset, exponent of node g), the last unit padded with copies of the last
    row; outs (count, 96)."""
    w, ew = PL.WORDS[table]
    ev = evaluate(nodes, values, exps)
    rows = [PL.elem_words(table, xv) + PL.elem_words(table, ov) + PL.limbs(exps[nd[2]], ew) for nd, (xv, ov, _) in zip(nodes, ev)]
    while len(rows) % num_io:
        rows.append(rows[-1])
    return (np.array(rows, dtype=np.uint32).reshape(-1, num_io, 2 * w + ew), np.array([PL.elem_words(table, o) for _, _, o in ev], dtype=np.uint32))


def unit_public_inputs(table, units, outs, num_io):
    """The public inputs of every unit of explicit_units (pads carry the last output again)."""
    rows = units.shape[0] * num_io
    o = np.concatenate([outs, np.repeat(outs[-1:], rows - len(outs), axis=0)]).reshape(units.shape[0], num_io, -1)
    return [PG.public_inputs(table, units[u], o[u]) for u in range(units.shape[0])]


# ---------------------------------------------------------------- the final exponentiation, f -> f^((p^12 - 1) / r)
FINAL_EXP_EXPS = [1, PL.BN_X, 2, 6, 12, 18, 30, 36]


def final_exp_nodes(base, f, fc, fi):
    """The normative 16 nodes (include/sbn.h) at node index `base`: f, fc = conj(f), fi = f^-1 are literal indices; exponent
    indices are into FINAL_EXP_EXPS.  The check is node base + 0, the result node base + 15."""
    n = lambda j: out(base + j)   # noqa: E731
    M = maps_word
    return [
        (fi, f, 0, 0),                  # 0: f * f_inv, must be one
        (fi, fc, 0, 0),                 # 1: conj(f) * f_inv = f^(p^6 - 1)
        (n(1), n(1), 0, M(0, 2)),       # 2: e = frob_2(n1) * n1
        (n(2), ONE, 1, 0),              # 3: fx
        (n(3), ONE, 1, 0),              # 4: fx2
        (n(4), ONE, 1, 0),              # 5: fx3
        (n(2), n(2), 0, M(2, 1)),       # 6: frob_1(e) * frob_2(e)
        (n(2), n(6), 0, M(3, 0)),       # 7: y0 = n6 * frob_3(e)
        (n(4), n(3), 0, M(1, 0)),       # 8: fx * frob_1(fx2)
        (n(5), n(5), 0, M(1, 0)),       # 9: fx3 * frob_1(fx3)
        (n(2), n(7), 2, M(6, 0)),       # 10: n7 * conj(e)^2
        (n(4), n(10), 3, M(2, 0)),      # 11: n10 * frob_2(fx2)^6
        (n(3), n(11), 4, M(7, 0)),      # 12: n11 * frob_7(fx)^12
        (n(8), n(12), 5, M(6, 0)),      # 13: n12 * conj(n8)^18
        (n(4), n(13), 6, M(6, 0)),      # 14: n13 * conj(fx2)^30
        (n(9), n(14), 7, M(6, 0)),      # 15: n14 * conj(n9)^36
    ]


def fq12_inverse(f):
    """f^-1 = fbar / (f * fbar), fbar = the product of the eleven non-trivial conjugates; f * fbar is the norm, in Fq."""
    fbar = list(PL.FQ12_ONE)
    for m in range(1, 12):
        fbar = PL.fq12_mul(fbar, frob(f, m))
    n = PL.fq12_mul(f, fbar)
    assert n[1:] == [0] * 11 and n[0] != 0
    ni = pow(n[0], P - 2, P)
    return [c * ni % P for c in fbar]


def final_exp_program(fs, f_invs=None):
    """(nodes, values, exps) of the final exponentiations of `fs`, 16 nodes each, literals f, conj(f), f^-1 per input."""
    nodes, values = [], []
    for t, f in enumerate(fs):
        fi = f_invs[t] if f_invs is not None else fq12_inverse(f)
        values += [f, frob(f, 6), fi]
        nodes += final_exp_nodes(16 * t, 3 * t, 3 * t + 1, 3 * t + 2)
    return nodes, values, list(FINAL_EXP_EXPS)


def final_exp_value(f):
    return PL.fq12_pow(f, (P ** 12 - 1) // R)


# ---------------------------------------------------------------- a seeded mapped DAG
def dag(table, seed=91):
    """The fixed mapped DAG of the tests: 15 nodes (num_io = 4: four units, one pad).  dag_properties() states what it must hold;
    the first 11 nodes (three units of 4 with one pad, a mapped last node) are the cut the device test walks."""
    r = PL.rng(seed)
    values = [PL.random_elem("fq12", r), PL.random_elem("fq12", r)]
    exps = [1, 3, PL.BN_X, 0] if table == "fq12u64" else [1, 3, r.randrange(1 << 255, 1 << 256), 0]
    M = maps_word
    nodes = [
        (0, ONE, 1, 0),                       # 0: level 0
        (1, 0, 0, 0),                         # 1: level 0, a plain product
        (out(0), ONE, 1, M(1, 0)),            # 2: x mapped
        (out(0), out(0), 2, M(2, 3)),         # 3: both operands the same node under different maps
        (out(1), out(1), 0, M(3, 4)),         # 4: the same again, across the unit boundary
        (out(2), out(3), 1, 0),               # 5: a level with links and no map
        (out(4), out(5), 0, M(5, 6)),         # 6
        (out(4), out(6), 1, M(0, 7)),         # 7: a level where only the offset is mapped; node 4 unmapped here, mapped in node 6
        (out(7), out(2), 0, M(8, 9)),         # 8: across the second boundary
        (out(8), out(7), 3, M(10, 11)),       # 9: a zero exponent under a map
        (out(9), out(8), 1, M(11, 10)),       # 10: the mapped last node of the cut
        (out(3), out(10), 0, M(9, 1)),        # 11
        (out(11), out(11), 0, M(4, 2)),       # 12
        (out(12), out(5), 1, M(6, 5)),        # 13
        (out(13), out(12), 0, M(7, 8)),       # 14: the mapped last node
    ]
    return nodes, values, exps


def dag_properties(nodes, num_io):
    """The properties a mapped DAG holds, by name (the tests assert that none of DAG_PROPERTIES is missing)."""
    have, used = set(), {}
    for g, (x, off, _, maps) in enumerate(nodes):
        mx, mo = maps & 0xFF, (maps >> 8) & 0xFF
        if mx:
            have.add("x_map_%d" % mx)
        if mo:
            have.add("offset_map_%d" % mo)
        if PG.is_link(x) and x == off and mx != mo:
            have.add("same_node_two_maps")
        for v, m in ((x, mx), (off, mo)):
            if PG.is_link(v):
                j = v & ~OUT
                used.setdefault(j, set()).add(bool(m))
                if m and j // num_io != g // num_io:
                    have.add("mapped_link_crosses_unit")
    if nodes[-1][3]:
        have.add("mapped_last_node")
    if any(len(u) == 2 for u in used.values()):
        have.add("output_mapped_and_unmapped")
    lv, depth = levels(nodes)
    kinds = set()
    for l in range(depth):
        at = [nd for nd, ll in zip(nodes, lv) if ll == l]
        kinds.add("mapped" if any(nd[3] for nd in at) else "plain")
        if any(nd[3] and not nd[3] & 0xFF for nd in at) and not any(nd[3] & 0xFF for nd in at):
            have.add("level_offset_only")
    if kinds == {"mapped", "plain"}:
        have.add("levels_with_and_without")
    return have


DAG_PROPERTIES = ({"x_map_%d" % m for m in range(1, 12)} | {"offset_map_%d" % m for m in range(1, 12)} |
                  {"same_node_two_maps", "mapped_link_crosses_unit", "mapped_last_node", "output_mapped_and_unmapped"})
CUT = 11
CUT_PROPERTIES = {"mapped_last_node", "levels_with_and_without", "level_offset_only", "mapped_link_crosses_unit"}
