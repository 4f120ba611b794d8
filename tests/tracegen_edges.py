"""Edge-value instance lists for the five Exp tables (G1, G2, Fq, Fq12, Fq12U64) with their outputs in plain Python integers,
degenerate curve instances with their collision-free control twins, and the BN254 field operands at the edges of the
Montgomery arithmetic.  Shared by test_tracegen_edges.py (host) and test_tracegen_edges_gpu.py (device).

The reference for every output is Python integers only (oracle_lib's g1_add / g2_add / fq12_mul and pow), never the C++ oracle.
The C++ oracle asserts on a degenerate instance (oracle/airs.hpp: a zero slope denominator) and would abort the whole process,
so oracle_trace() refuses any curve list that a Python walk of its chains has not shown to be collision-free."""
import hashlib
import os

import numpy as np
import pytest

import oracle_lib as O

P = O.BN_P
R = O.BN_R
GLP = O.GL_P
U256 = (1 << 256) - 1

# exponents of the 256-bit tables: small values, single bits at the 32- and 64-bit limb seams, all-ones, alternating patterns, r and
# its neighbours (r x = O on G1 and G2)
EXPONENTS = [0, 1, 2, 3] + [1 << b for b in (31, 32, 63, 64, 127, 128, 255)] + [
    (1 << 32) - 1, U256, int("55" * 32, 16), int("AA" * 32, 16), R - 1, R, R + 1]
EXPONENTS_U64 = [0, 1, 1 << 63, GLP - 1, 2, (1 << 32) - 1, 1 << 32, GLP - 2]
DEGENERATE_STEPS = (0, 1, 31, 32, 128, 255)
# (instances per list, io words per instance, public inputs per instance, offset of the output in them, rows per instance)
SHAPE = {"g1": (128, 40, 56, 40, 512), "g2": (128, 72, 104, 72, 512), "fq": (128, 24, 32, 24, 512),
         "fq12": (16, 200, 584, 392, 512), "fq12u64": (16, 194, 577, 385, 128)}


def limbs(v, n, bits):
    return [(v >> (bits * i)) & ((1 << bits) - 1) for i in range(n)]


def from_limbs(ws, bits):
    return sum(int(w) << (bits * i) for i, w in enumerate(ws))


# ---------------------------------------------------------------- curve points
def g1_neg(p):
    return None if p is None else (p[0], (-p[1]) % P)


def g2_neg(p):
    return None if p is None else (p[0], ((-p[1][0]) % P, (-p[1][1]) % P))


def _g1_at(x0, step):
    """First G1 point with x = x0, x0 + step, x0 + 2 step, ... (p = 3 mod 4: y = rhs^((p+1)/4))."""
    x = x0 % P
    while True:
        rhs = (x * x * x + 3) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            return (x, y)
        x = (x + step) % P


def _g2_at(x0, step):
    """First twist point with x = x0, x0 + step, ... (x0 and step are Fq2 pairs)."""
    x = x0
    while True:
        rhs = O.fq2_add(O.fq2_mul(O.fq2_mul(x, x), x), O.G2_B)
        y = O.fq2_sqrt(rhs)
        if y is not None and O.fq2_mul(y, y) == rhs:
            return (x, y)
        x = O.fq2_add(x, step)


G1_GEN = (1, 2)
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
           11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930,
           4082367875863433681332203403145435568316851327593401208105741076214120093531))


def g1_bases():
    """The generator, -G, 2G, small x, x just below p, and x whose 16-bit limbs are mostly 0x0000 or 0xFFFF."""
    pts = [G1_GEN, g1_neg(G1_GEN), O.g1_add(G1_GEN, G1_GEN), _g1_at(5, 1), _g1_at(1 << 40, 1), _g1_at(P - 1, -1),
           _g1_at(P - (1 << 64) + 7, 1), _g1_at((1 << 128) - 1, -1), _g1_at(1 << 192, 1), _g1_at((1 << 253) - 1, -1),
           _g1_at((1 << 64) - 1, -1), _g1_at(0xFFFF0000FFFF0000FFFF0000FFFF << 64, 1)]
    pts.append(g1_neg(pts[5]))                                   # y -> p - y: near-p and small y both occur
    return pts


def g2_bases():
    """The twist generator, its negative, and points whose x has one zero component ((c, 0), (0, c)), small or near-p components, or
    all-ones 16-bit limbs (the table checks the group law only, so points off the prime-order subgroup are fine)."""
    return [G2_GEN, g2_neg(G2_GEN), O.g2_add(G2_GEN, G2_GEN), _g2_at((1, 0), (1, 0)), _g2_at((0, 1), (0, 1)),
            _g2_at((P - 1, 0), (P - 1, 0)), _g2_at((0, P - 1), (0, P - 1)), _g2_at((5, 7), (1, 0)),
            _g2_at(((1 << 128) - 1, (1 << 64) - 1), (P - 1, 0)), _g2_at((P - (1 << 64), (1 << 192)), (0, 1))]


def _ops(curve):
    if curve == "g1":
        return O.g1_add, g1_neg, O.g1_mul
    return O.g2_add, g2_neg, O.g2_mul


def curve_walk(curve, x, off, e):
    """The table's two chains (A[t] = 2^t x, B[0] = offset, B[t+1] = B[t] + bit_t A[t]) in Python affine integers.
    Returns (output, None) or (None, t) with t the first step whose addition meets B[t] = +-A[t], or whose doubling meets y = 0."""
    add, neg, _ = _ops(curve)
    a, b = x, off
    for t in range(256):
        if (e >> t) & 1:
            if b is None or a is None or b[0] == a[0]:
                return None, t
            b = add(b, a)
        if a is None or a[1] in (0, (0, 0)):
            return None, t
        a = add(a, a)
    return b, None


def scalar_mul(curve, x, k):
    add, neg, mul = _ops(curve)
    return mul(x, k) if k >= 0 else neg(mul(x, -k))


# ---------------------------------------------------------------- io packing
def _pack(table, inst):
    """inst = (x, offset, e) in the shape of oracle_lib's native tuples -> one io row."""
    x, off, e = inst
    if table == "g1":
        vals, ew = [x[0], x[1], off[0], off[1]], limbs(e, 8, 32)
    elif table == "g2":
        vals, ew = [x[0][0], x[0][1], x[1][0], x[1][1], off[0][0], off[0][1], off[1][0], off[1][1]], limbs(e, 8, 32)
    elif table == "fq":
        vals, ew = [x, off], limbs(e, 8, 32)
    elif table == "fq12":
        vals, ew = list(x) + list(off), limbs(e, 8, 32)
    else:
        vals, ew = list(x) + list(off), limbs(e, 2, 32)
    row = []
    for v in vals:
        row += limbs(v, 8, 32)
    return row + ew


def pack(table, insts):
    return np.array([_pack(table, i) for i in insts], dtype=np.uint32)


def expected_output(table, inst):
    """The instance's output in Python integers: offset + e x on the curves, offset * x^e in the fields."""
    x, off, e = inst
    if table in ("g1", "g2"):
        out, t = curve_walk(table, x, off, e)
        assert t is None, f"degenerate instance (step {t})"
        return out
    if table == "fq":
        return off * pow(x, e, P) % P
    return O.fq12_mul(off, O.fq12_pow(x, e))


def outputs_from_pi(table, pi):
    """The outputs the public inputs carry, as Python values (u32 limbs on the curves and Fq; 16-bit limbs on Fq12)."""
    _, _, per, at, _ = SHAPE[table]
    res = []
    for k in range(len(pi) // per):
        w = [int(v) for v in pi[per * k + at:per * (k + 1)]]
        if table == "g1":
            res.append((from_limbs(w[0:8], 32), from_limbs(w[8:16], 32)))
        elif table == "g2":
            c = [from_limbs(w[8 * j:8 * j + 8], 32) for j in range(4)]
            res.append(((c[0], c[1]), (c[2], c[3])))
        elif table == "fq":
            res.append(from_limbs(w, 32))
        else:
            res.append([from_limbs(w[16 * c:16 * c + 16], 16) for c in range(12)])
    return res


# ---------------------------------------------------------------- the edge lists
_PROVEN = set()       # digests of curve instance lists whose chains a Python walk has shown collision-free


def _digest(ios):
    return hashlib.sha256(np.ascontiguousarray(ios, dtype=np.uint32).tobytes()).hexdigest()


def _curve_edge_insts(curve, num_io, seed):
    rng = np.random.default_rng(seed)
    add, neg, _ = _ops(curve)
    bases = g1_bases() if curve == "g1" else g2_bases()
    rnd = O.g1_random if curve == "g1" else O.g2_random
    insts = []
    for k in range(num_io):
        x = bases[k % len(bases)]
        e = EXPONENTS[k % len(EXPONENTS)]
        # offsets: x itself (valid when bit 0 is clear), 2x, -x, a random point; the first one whose chains never collide
        cands = [x, add(x, x), neg(x), rnd(rng)]
        cands = cands[k % 4:] + cands[:k % 4]
        for off in cands:
            if off is not None and curve_walk(curve, x, off, e)[1] is None:
                insts.append((x, off, e))
                break
        else:
            raise AssertionError(f"no collision-free offset for instance {k}")
    return insts


def _field_edge_insts(table, num_io, seed):
    rng = np.random.default_rng(seed)
    if table == "fq":
        bases = [0, 1, P - 1, P - 2, 2, (1 << 64) - 1, 1 << 128, P - (1 << 192), (1 << 253) - 1, pow(2, -256, P), pow(2, 256, P)]
        offs = [1, P - 1, 0, int.from_bytes(rng.bytes(32), "little") % P]
        exps = EXPONENTS
    else:
        def single(j, c):
            v = [0] * 12
            v[j] = c
            return v
        rand = [int.from_bytes(rng.bytes(32), "little") % P for _ in range(12)]
        bases = [[0] * 12, single(0, 1), single(0, P - 1), single(0, P - 2), single(6, 1), single(5, P - 1), single(11, 2),
                 single(3, (1 << 253) - 1), [P - 1] * 12, [1] * 12, rand]
        offs = [single(0, 1), single(0, P - 1), [0] * 12, [int.from_bytes(rng.bytes(32), "little") % P for _ in range(12)]]
        exps = EXPONENTS if table == "fq12" else EXPONENTS_U64
    insts = []
    for k in range(num_io):
        x = bases[k % len(bases)]
        off = offs[(k // len(bases) + k) % len(offs)]
        if table == "fq":
            off = x if k % 7 == 3 else off
        insts.append((x, off, exps[k % len(exps)]))
    return insts


def edge_list(table, seed=0):
    """A full edge-case instance list of the table at its smallest device size (128 instances for G1, G2 and Fq, 16 for Fq12 and
    Fq12U64): (ios, native) as oracle_lib's *_inputs return them."""
    num_io = SHAPE[table][0]
    insts = _curve_edge_insts(table, num_io, seed) if table in ("g1", "g2") else _field_edge_insts(table, num_io, seed)
    ios = pack(table, insts)
    if table in ("g1", "g2"):
        _PROVEN.add(_digest(ios))
    return ios, insts


def identical_list(table, seed=0):
    """Every instance the same edge instance: the instance boundaries and the range-check multiplicities see one value per column."""
    num_io = SHAPE[table][0]
    _, insts = edge_list(table, seed)
    inst = insts[10]
    ios = pack(table, [inst] * num_io)
    if table in ("g1", "g2"):
        _PROVEN.add(_digest(ios))
    return ios, [inst] * num_io


def degenerate_cases(curve, seed=0):
    """Degenerate curve instances: for base x, exponent e with bit t set and s = +-1, offset = (s 2^t - (e mod 2^t)) x, so the
    addition of step t meets B[t] = s A[t] (s = -1: the sum is the point at infinity).  Each case is placed in the edge list at
    instance 0, a middle one or the last one; its control twin is the same offset with bit t cleared, which Python shows valid.
    Returns [(t, s, pos, bad_ios, control_inst)]; bad_ios is NOT registered as valid (oracle_trace refuses it)."""
    rng = np.random.default_rng(1000 + seed)
    base_ios, insts = edge_list(curve, seed)
    bases = g1_bases() if curve == "g1" else g2_bases()
    num_io = len(insts)
    cases = []
    for i, (t, s) in enumerate([(t, s) for t in DEGENERATE_STEPS for s in (1, -1)]):
        x = bases[i % len(bases)]
        while True:
            e = int.from_bytes(rng.bytes(32), "little") | (1 << t)
            m = e & ((1 << t) - 1)
            off = scalar_mul(curve, x, s * (1 << t) - m)
            if off is None:
                continue
            _, step = curve_walk(curve, x, off, e)
            twin = e & ~(1 << t)
            if step == t and curve_walk(curve, x, off, twin)[1] is None:
                break
        pos = (0, num_io // 2, num_io - 1)[i % 3]
        bad = base_ios.copy()
        bad[pos] = _pack(curve, (x, off, e))
        cases.append((t, s, pos, bad, (x, off, twin)))
    return cases


def controls_list(curve, cases, seed=0):
    """The edge list with the control twins of `cases` written over instances 0, 1, ... (each one shown valid by a walk)."""
    _, insts = edge_list(curve, seed)
    insts = list(insts)
    for j, c in enumerate(cases):
        insts[(j * 37) % len(insts)] = c[4]
    for inst in insts:
        assert curve_walk(curve, *inst)[1] is None
    ios = pack(curve, insts)
    _PROVEN.add(_digest(ios))
    return ios, insts


def assert_proven_valid(table, ios):
    """Guard in front of every oracle call: a curve list must have been built here from walked instances (or walk clean now)."""
    if table not in ("g1", "g2") or _digest(ios) in _PROVEN:
        return
    words = SHAPE[table][1]
    for k, row in enumerate(np.asarray(ios)):
        w = [from_limbs(row[8 * j:8 * j + 8], 32) for j in range(words // 8)]
        if table == "g1":
            inst = ((w[0], w[1]), (w[2], w[3]), w[4])
        else:
            inst = (((w[0], w[1]), (w[2], w[3])), ((w[4], w[5]), (w[6], w[7])), w[8])
        _, t = curve_walk(table, *inst)
        if t is not None:
            raise AssertionError(f"instance {k} is degenerate at step {t}: the oracle would abort on it")
    _PROVEN.add(_digest(ios))


TRACE = {"g1": "g1exp_trace", "g2": "g2exp_trace", "fq": "fqexp_trace", "fq12": "fq12exp_trace", "fq12u64": "fq12expu64_trace"}
AIR = {"g1": O.AIR_G1_EXP, "g2": O.AIR_G2_EXP, "fq": O.AIR_FQ_EXP, "fq12": O.AIR_FQ12_EXP, "fq12u64": O.AIR_FQ12_EXP_U64}


def oracle_trace(table, ios):
    assert_proven_valid(table, ios)
    return getattr(O, TRACE[table])(ios)


def stark_class(S, table):
    return {"g1": S.G1ExpStark, "g2": S.G2ExpStark, "fq": S.FqExpStark, "fq12": S.Fq12ExpStark, "fq12u64": S.Fq12ExpU64Stark}[table]


def degree_bits(table, num_io):
    return (SHAPE[table][4] * num_io).bit_length() - 1


def trace_domain_consumer_args(n, i):
    """On the trace domain H: z_last = w^i - w^(n-1), L_first = [i == 0], L_last = [i == n-1]."""
    lg = n.bit_length() - 1
    w = pow(1753635133440165772, 1 << (32 - lg), GLP)
    return (pow(w, i, GLP) - pow(w, n - 1, GLP)) % GLP, int(i == 0), int(i == n - 1)


# ---------------------------------------------------------------- chain placements of the device witness
def check_every_chain_placement(gpu, stark, cfg, bits, ios, pi_want, trace_want):
    """The curve chains of the device witness (src/curves/g1/exp.rs:255-318) in every placement the library can pick
    (SBN_TRACEGEN_DEVICE_CHAIN, read when a prover is created): 0 = host pool (eight instances per AVX-512 IFMA register, or the
    scalar form with SBN_NO_AVX512-less CPUs), 1 = one lane per instance (chain_kernel), 2 = one wave per instance
    (chain_coop_kernel, what a rank with a small host share gets), and the old one-pass range-check kernel: same trace words."""
    for env in PLACEMENTS:
        with placement(gpu, stark, cfg, bits, env) as pr:
            assert np.array_equal(pr.generate_trace(ios), pi_want), env
            got = pr.read_trace()
            bad = np.nonzero((got != trace_want).any(axis=1))[0]
            assert bad.size == 0, (env, bad[:8].tolist())


PLACEMENTS = ({"SBN_TRACEGEN_DEVICE_CHAIN": "0"}, {"SBN_TRACEGEN_DEVICE_CHAIN": "1"}, {"SBN_TRACEGEN_DEVICE_CHAIN": "2"},
              {"SBN_EXPERIMENTAL": "1", "SBN_RANGE_CHECK": "1"})


class placement:
    """A prover created under the switches `env` (restored afterwards), closed on exit; checks that the switches took."""
    def __init__(self, gpu, stark, cfg, bits, env):
        self.args, self.env = (gpu, stark, cfg, bits), env

    def __enter__(self):
        gpu, stark, cfg, bits = self.args
        old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        try:
            self.pr = gpu.Prover(stark, cfg, bits)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        d = self.pr.describe()
        if "SBN_TRACEGEN_DEVICE_CHAIN" in self.env:
            want = {"0": "host_pool", "1": "device_lane", "2": "device_wave"}[self.env["SBN_TRACEGEN_DEVICE_CHAIN"]]
            assert d["curve_chains"].startswith(want), d
        for k, key in (("SBN_RANGE_CHECK", "range_check"), ("SBN_FQ12_HOST_CHAIN", "fq12_host_chain"),
                       ("SBN_FQ12_ROW_KERNEL", "fq12_row_kernel"), ("SBN_EXPERIMENTAL", "experimental")):
            if k in self.env:
                assert d[key] == self.env[k], d
        return self.pr

    def __exit__(self, *exc):
        self.pr.close()
        return False


# ---------------------------------------------------------------- BN254 base-field operands
def fq_special_operands():
    """0, 1, 2, p-1, p-2, (p+-1)/2, the 32/64/128/192-bit seams, 2^253, p - 2^192, 2^k - 1 (all-ones 32-bit limbs), R = 2^256,
    R^-1 and R^2 mod p, and the values whose Montgomery form is 1 or p-1 (R^-1 and -R^-1)."""
    rinv = pow(2, -256, P)
    vals = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 64, (1 << 128) - 1,
            1 << 192, 1 << 253, P - (1 << 192)]
    vals += [(1 << k) - 1 for k in range(32, 254, 32)]
    vals += [pow(2, 256, P), rinv, pow(2, 512, P), (P - rinv) % P, pow(2, 256 * 3, P)]
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    return out


def fq_random(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    return [int(a) % P for a in (from_limbs(r, 64) for r in w)]


def fq_field_parity(S, on_device):
    """Every op of sbn_bn254_fq_batch on all pairs of the special operands plus a 2^16-element random sweep, against Python."""
    sp = fq_special_operands()
    a = [x for x in sp for _ in sp]
    b = [y for _ in sp for y in sp]
    ra, rb = fq_random(1 << 16, 1), fq_random(1 << 16, 2)
    nz = [x for x in sp if x]
    inv_pairs = [(x, pow(x, -1, P)) for x in nz] + [(x, P - pow(x, -1, P)) for x in nz]   # products land on 1 and p - 1
    A, B = a + ra + [p[0] for p in inv_pairs], b + rb + [p[1] for p in inv_pairs]
    run = lambda op, x, y=None: S.bn254_fq_batch(op, x, y, on_device=on_device)   # noqa: E731
    assert run("mul", A, B) == [x * y % P for x, y in zip(A, B)]
    assert run("add", A, B) == [(x + y) % P for x, y in zip(A, B)]
    assert run("sub", A, B) == [(x - y) % P for x, y in zip(A, B)]
    xs = nz + [x for x in ra if x]
    assert run("inv", xs) == [pow(x, -1, P) for x in xs]
    xs8 = nz * 8 + [x for x in ra if x][:4096]                        # the special values in several slots of a group
    assert run("batch_inv", xs8) == [pow(x, -1, P) for x in xs8]
    c0 = [x for x in sp for _ in sp] + ra[:4096]
    c1 = [y for _ in sp for y in sp] + rb[:4096]
    keep = [i for i in range(len(c0)) if c0[i] or c1[i]]
    c0, c1 = [c0[i] for i in keep], [c1[i] for i in keep]
    assert run("fq2_inv", c0, c1) == [O.fq2_inv((x, y)) for x, y in zip(c0, c1)]
    # refusals: an input >= p, a zero to invert
    for op, args in (("mul", ([P], [1])), ("add", ([1], [P])), ("inv", ([(1 << 256) - 1],)), ("fq2_inv", ([0], [P + 1]))):
        with pytest.raises(S.SbnError) as e:
            run(op, *args)
        assert e.value.code == -2, op
    for op, args in (("inv", ([1, 0],)), ("batch_inv", ([1] * 7 + [0],)), ("fq2_inv", ([1, 0], [0, 0]))):
        with pytest.raises(S.SbnError) as e:
            run(op, *args)
        assert e.value.code == -1, op
    with pytest.raises(S.SbnError):
        run("batch_inv", [1] * 7)                                      # not a multiple of 8
