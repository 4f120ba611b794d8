"""Host tests of the field powers and power towers (sbn_power_instances, sbn_power_check, sbn_bn_x; run with `-m "not gpu"`): the
explicit, padded list and the powers equal Python's word for word -- Fq against pow(), the Fq12 tables against the schoolbook
product of tests/power_lists.py --, the unchanged host generators put the same outputs among the public inputs, the check accepts
those public inputs and rejects every single edit naming the instance and the field, and every refusal returns its code in the
order the header states."""
import ctypes
import re

import numpy as np
import pytest

import power_lists as PL
import tracegen_edges as T

BAD_ARG, NON_CANONICAL, VERIFY_FAILED, UNSUPPORTED = -1, -2, -6, -7
P = PL.P


def refused(S, code, names, fn, *args, **kw):
    with pytest.raises(S.SbnError) as e:
        fn(*args, **kw)
    assert e.value.code == code and re.search(names, str(e.value)), str(e.value)


def test_constants_and_exports(S):
    assert S.BN_X == PL.BN_X == 0x44E992B44A6909F1 == S.bn_x() and S.BN_P == P
    assert (S.FQ_INVERSE_EXP, S.FQ_LEGENDRE_EXP, S.FQ_SQRT_EXP) == (P - 2, (P - 1) // 2, (P + 1) // 4) and P % 4 == 3
    out = np.zeros(2, dtype=np.uint32)
    assert S.lib().sbn_bn_x(out.ctypes.data) == 0 and out.tolist() == [0x4A6909F1, 0x44E992B4]
    assert S.lib().sbn_bn_x(None) == BAD_ARG
    for name in ("sbn_power_instances", "sbn_prover_generate_trace_powers", "sbn_batch_prover_prove_powers", "sbn_power_check", "sbn_bn_x"):
        assert name in S.EXPORTS and hasattr(S.lib(), name), name


# ---------------------------------------------------------------- Fq against pow()
FQ_RNG = PL.rng(11)
FQ_BASES = [0, 1, P - 1, FQ_RNG.randrange(P), FQ_RNG.randrange(P)]
FQ_EXPS = [0, 1, P - 2, (1 << 256) - 1, FQ_RNG.randrange(1 << 256)]


def _check_rows(table, ios, powers, bases, exps, depth):
    """The shape every list must have, stated on the words: offset one, the level links, pads = the last row."""
    w, ew = PL.WORDS[table]
    count = len(bases)
    rows = ios.reshape(-1, 2 * w + ew)
    one = np.array([1] + [0] * (w - 1), dtype=np.uint32)
    for g, row in enumerate(rows):
        if g >= count * depth:
            assert np.array_equal(row, rows[count * depth - 1]), g
            continue
        k, l = divmod(g, depth)
        assert np.array_equal(row[w:2 * w], one), g
        assert row[2 * w:].tolist() == PL.limbs(exps[0] if len(exps) == 1 else exps[k], ew), g
        want_x = np.array(PL.elem_words(table, bases[k]), dtype=np.uint32) if l == 0 else powers[k][l - 1]
        assert np.array_equal(row[:w], want_x), g


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("shared", [False, True], ids=["per_tower", "shared"])
def test_fq_powers_equal_pow(S, depth, shared):
    stark = S.FqExpStark(4)                                                  # num_io only shapes the list: 5 / 15 rows in units of 4
    for exps in ([[e] for e in FQ_EXPS] if shared else [FQ_EXPS]):
        ios, powers = S.power_instances(stark, PL.base_words("fq", FQ_BASES), PL.exp_words("fq", exps), depth)
        units, want = PL.explicit_units("fq", FQ_BASES, exps, depth, 4)
        assert ios.shape == units.shape == (-(-5 * depth // 4), 4, 24)
        assert np.array_equal(powers, want) and np.array_equal(ios, units)
        for k, b in enumerate(FQ_BASES):
            x = b
            for l in range(depth):
                x = pow(x, exps[0] if shared else exps[k], P)
                assert PL.from_limbs(powers[k][l]) == x, (k, l)
        _check_rows("fq", ios, powers, FQ_BASES, exps, depth)
    # the Python conveniences: ints as bases, one int as the shared exponent
    ios2, powers2 = S.power_instances(stark, FQ_BASES, FQ_EXPS[4], depth)
    assert np.array_equal(powers2, PL.explicit_units("fq", FQ_BASES, [FQ_EXPS[4]], depth, 4)[1])


def test_fq_inverse_and_square_roots(S):
    stark = S.FqExpStark(128)
    xs = [x for x in FQ_BASES if x] + [FQ_RNG.randrange(1, P) for _ in range(3)]
    _, inv = S.power_instances(stark, xs, S.FQ_INVERSE_EXP)
    for x, w in zip(xs, inv[:, 0]):
        assert x * PL.from_limbs(w) % P == 1
    _, zero = S.power_instances(stark, [0], S.FQ_INVERSE_EXP)
    assert not zero.any()                                                    # 0^(p-2) = 0: legal, the table defines it
    # known squares (a^2, and 0) and known non-residues (-a^2: -1 is a non-residue because p = 3 mod 4)
    roots_of = [FQ_RNG.randrange(1, P) for _ in range(4)]
    squares = [a * a % P for a in roots_of] + [0, 1]
    non_res = [(P - a * a) % P for a in roots_of] + [P - 1]
    xs = squares + non_res
    _, leg = S.power_instances(stark, xs, S.FQ_LEGENDRE_EXP)
    assert [PL.from_limbs(w) for w in leg[:, 0]] == [1, 1, 1, 1, 0, 1] + [P - 1] * 5
    _, roots = S.power_instances(stark, xs, S.FQ_SQRT_EXP)
    flags = S.fq_sqrt_flags(xs, roots[:, 0])
    assert flags.tolist() == [True] * len(squares) + [False] * len(non_res)
    assert S.fq_sqrt_flags(PL.base_words("fq", xs), [PL.from_limbs(w) for w in roots[:, 0]]).tolist() == flags.tolist()


# ---------------------------------------------------------------- the Fq12 tables against the schoolbook product
def test_the_schoolbook_product_is_a_field_product():
    r = PL.rng(5)
    x, y, z = (PL.random_elem("fq12", r) for _ in range(3))
    assert PL.fq12_mul(x, PL.FQ12_ONE) == x and PL.fq12_mul(x, y) == PL.fq12_mul(y, x)
    assert PL.fq12_mul(PL.fq12_mul(x, y), z) == PL.fq12_mul(x, PL.fq12_mul(y, z))
    w = [0, 1] + [0] * 10
    assert PL.fq12_pow(w, 6) == [9, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]            # w^6 = 9 + i


FQ12_CASES = {"fq12u64": (3, 3, [PL.BN_X], 21), "fq12": (2, 2, [PL.rng(22).randrange(1 << 255, 1 << 256)], 23)}


@pytest.fixture(scope="module")
def fq12_case(S):
    """(bases, exps, depth, ios, powers, public inputs of the unit from the unchanged host generator), once per table."""
    cache = {}

    def get(table):
        if table not in cache:
            count, depth, exps, seed = FQ12_CASES[table]
            r = PL.rng(seed)
            bases = [PL.random_elem("fq12", r) for _ in range(count)]
            stark = T.stark_class(S, table)(16)
            ios, powers = S.power_instances(stark, PL.base_words(table, bases), PL.exp_words(table, exps), depth)
            cache[table] = (bases, exps, depth, ios, powers, stark.generate_public_inputs(ios[0]))
        return cache[table]
    return get


@pytest.mark.parametrize("table", ["fq12u64", "fq12"])
def test_fq12_towers_equal_the_schoolbook_product(S, fq12_case, table):
    bases, exps, depth, ios, powers, pi = fq12_case(table)
    count = len(bases)
    units, want = PL.explicit_units(table, bases, exps, depth, 16)
    assert ios.shape == units.shape and units.shape[0] == 1
    for k in range(count):                                                   # square-and-multiply over Python integers
        x = bases[k]
        for l in range(depth):
            x = PL.fq12_pow(x, exps[0])
            assert PL.elem_from_words(table, powers[k][l].tolist()) == x, (k, l)
    assert np.array_equal(powers, want) and np.array_equal(ios, units)
    _check_rows(table, ios, powers, bases, exps, depth)
    # the unchanged host generator, run on ios_out, puts the same outputs among its public inputs
    outs = PL.pi_outputs(table, 16, pi)
    assert np.array_equal(outs[:count * depth], powers.reshape(count * depth, 96))
    assert np.array_equal(outs[count * depth:], np.repeat(outs[count * depth - 1:count * depth], 16 - count * depth, axis=0))
    stark = T.stark_class(S, table)(16)
    assert np.array_equal(S.power_check(stark, [pi], PL.base_words(table, bases), PL.exp_words(table, exps), depth), powers)


# ---------------------------------------------------------------- power_check
@pytest.fixture(scope="module")
def straddling(S):
    """3 towers of depth 3 with BN_X in units of 4: towers 1 and 2 straddle a unit boundary, the last unit has 3 pads."""
    r = PL.rng(31)
    bases = PL.base_words("fq12u64", [PL.random_elem("fq12", r) for _ in range(3)])
    stark = S.Fq12ExpU64Stark(4)
    ios, powers = S.power_instances(stark, bases, S.BN_X, 3)
    assert ios.shape == (3, 4, 194)
    return stark, bases, powers, [stark.generate_public_inputs(u) for u in ios]


U64_PER, U64_X, U64_OFF, U64_EXP, U64_OUT = 577, 0, 192, 384, 385


def test_power_check_accepts_the_honest_public_inputs(S, straddling):
    stark, bases, powers, pis = straddling
    assert np.array_equal(S.power_check(stark, pis, bases, S.BN_X, 3), powers)
    refused(S, VERIFY_FAILED, r"instance 0\b.*exponent", S.power_check, stark, pis, bases, S.BN_X + 1, 3)
    refused(S, VERIFY_FAILED, r"instance 0\b.*x differs", S.power_check, stark, pis, bases[::-1], S.BN_X, 3)


@pytest.mark.parametrize("g,at,value,names", [
    (5, U64_OFF + 3, 1, r"instance 5\b.*offset"),
    (2, U64_EXP, None, r"instance 2\b.*exponent"),
    (4, U64_X, None, r"instance 4\b.*x differs from the output of instance 3\b"),      # a level-1 x, across the unit boundary
    (6, U64_X + 17, None, r"instance 6\b.*x differs from the caller's base"),
    (10, U64_EXP, None, r"instance 10 \(pad\): exponent"),
    (9, U64_OUT + 1, None, r"instance 9 \(pad\): output"),
    (7, U64_OUT + 5, 1 << 16, r"instance 7\b.*output limb 5\b"),
], ids=["offset", "exponent", "level1_x", "base", "pad_exponent", "pad_output", "output_limb"])
def test_power_check_names_the_tampered_instance_and_field(S, straddling, g, at, value, names):
    stark, bases, _, pis = straddling
    bad = [p.copy() for p in pis]
    w = bad[g // 4]
    i = U64_PER * (g % 4) + at
    w[i] = value if value is not None else int(w[i]) ^ 1
    refused(S, VERIFY_FAILED, names, S.power_check, stark, bad, bases, S.BN_X, 3)


def test_power_check_counts_the_units_and_bounds_the_coefficients(S, straddling):
    stark, bases, _, pis = straddling
    refused(S, VERIFY_FAILED, r"2 units given", S.power_check, stark, pis[:2], bases, S.BN_X, 3)
    refused(S, VERIFY_FAILED, r"4 units given", S.power_check, stark, pis + pis[:1], bases, S.BN_X, 3)
    bad = [p.copy() for p in pis]
    bad[2][U64_PER * 0 + U64_OUT:U64_PER * 0 + U64_OUT + 16] = 0xFFFF          # instance 8: output coefficient 0 = 2^256 - 1 >= p
    refused(S, VERIFY_FAILED, r"instance 8\b.*output has a coefficient >= p", S.power_check, stark, bad, bases, S.BN_X, 3)


def test_power_check_on_fq_public_inputs(S):
    """FqExpStark(128), the table's minimum: 42 towers of depth 3 and 2 pads in one unit; an output limb of 2^32 is out of range."""
    stark = S.FqExpStark(128)
    r = PL.rng(41)
    bases = [r.randrange(P) for _ in range(42)]
    ios, powers = S.power_instances(stark, bases, S.FQ_SQRT_EXP, 3)
    pi = stark.generate_public_inputs(ios[0])
    assert np.array_equal(PL.pi_outputs("fq", 128, pi)[:126], powers.reshape(126, 8))
    assert np.array_equal(S.power_check(stark, [pi], bases, S.FQ_SQRT_EXP, 3), powers)
    bad = pi.copy()
    bad[32 * 100 + 24 + 7] = 1 << 32
    refused(S, VERIFY_FAILED, r"instance 100\b.*output limb 7\b", S.power_check, stark, [bad], bases, S.FQ_SQRT_EXP, 3)
    bad = pi.copy()
    bad[32 * 127 + 8] = 2                                                    # the offset of the last pad
    refused(S, VERIFY_FAILED, r"instance 127 \(pad\): offset", S.power_check, stark, [bad], bases, S.FQ_SQRT_EXP, 3)


# ---------------------------------------------------------------- refusals, in the order of the header
def test_refusals_in_header_order(S):
    L = S.lib()
    bases = PL.base_words("fq", [3, 5])
    exps = PL.exp_words("fq", [7, 9])

    def call(kind, b, e, exp_count, count, depth, num_io):
        rc = L.sbn_power_instances(kind, b.ctypes.data if b is not None else None, e.ctypes.data if e is not None else None,
                                   exp_count, count, depth, num_io, None, None)
        return rc, L.sbn_last_error().decode()

    # 1. the kind, before anything else (null arguments included)
    for kind in (S.AIR_G1_EXP, S.AIR_G2_EXP, S.AIR_G1_OP, S.AIR_FQ12_MUL, 99):
        assert call(kind, None, None, 0, 0, 0, 0)[0] == UNSUPPORTED, kind
    refused(S, UNSUPPORTED, "field tables", S.power_instances, S.G1ExpStark(128), np.zeros((1, 16), dtype=np.uint32), 1)
    # 2. the arguments, before any value is read (the bases below hold a value >= p)
    big = PL.base_words("fq", [3, P])
    for args in ((None, exps, 2, 2, 1, 4), (big, None, 2, 2, 1, 4), (big, exps, 2, 0, 1, 4), (big, exps, 2, 2, 0, 4), (big, exps, 2, 2, 1, 0)):
        rc, msg = call(S.AIR_FQ_EXP, *args)
        assert rc == BAD_ARG and "null argument" in msg, (args[2:], msg)
    three = PL.base_words("fq", [3, P, 5])
    for exp_count in (0, 2, 4):
        rc, msg = call(S.AIR_FQ_EXP, three, exps, exp_count, 3, 1, 4)
        assert rc == BAD_ARG and "exp_count" in msg, msg
    # 3. the values, tower by tower, as the table's generator refuses an instance
    rc, msg = call(S.AIR_FQ_EXP, three, exps, 1, 3, 2, 4)
    assert rc == BAD_ARG and re.search(r">= p \(tower 1\)", msg), msg
    f12 = np.zeros((3, 96), dtype=np.uint32)
    f12[2, 88:96] = PL.limbs(P, 8)                                           # the last coefficient of tower 2
    for kind in (S.AIR_FQ12_EXP, S.AIR_FQ12_EXP_U64):
        rc, msg = call(kind, f12, exps, 1, 3, 1, 16)
        assert rc == BAD_ARG and re.search(r"coefficient >= p \(tower 2\)", msg), msg
    e64 = PL.exp_words("fq12u64", [PL.BN_X, PL.GLP, PL.GLP - 1])
    rc, msg = call(S.AIR_FQ12_EXP_U64, f12, e64, 3, 3, 1, 16)                 # tower 1's exponent comes before tower 2's base
    assert rc == NON_CANONICAL and re.search(r"exponent of tower 1\b", msg), msg
    f12[2, 88:96] = 0
    e64[1] = PL.limbs(PL.GLP - 1, 2)
    assert call(S.AIR_FQ12_EXP_U64, f12, e64, 3, 3, 2, 16)[0] == 0           # p - 1 of Goldilocks, zero bases: legal
    rc, msg = call(S.AIR_FQ12_EXP_U64, f12, PL.exp_words("fq12u64", [PL.GLP]), 1, 3, 2, 16)
    assert rc == NON_CANONICAL and re.search(r"exponent of tower 0\b", msg), msg
    # the check refuses the same way, before it reads a public input
    ptrs = (ctypes.c_void_p * 1)()
    assert L.sbn_power_check(S.AIR_G1_EXP, 4, ptrs, 1, 1, 1, bases.ctypes.data, exps.ctypes.data, 1, None) == UNSUPPORTED
    assert L.sbn_power_check(S.AIR_FQ_EXP, 4, ptrs, 1, 0, 1, bases.ctypes.data, exps.ctypes.data, 1, None) == BAD_ARG
    assert L.sbn_power_check(S.AIR_FQ_EXP, 4, None, 1, 1, 1, bases.ctypes.data, exps.ctypes.data, 1, None) == BAD_ARG


def test_zero_bases_and_zero_exponents_are_legal(S):
    stark = S.Fq12ExpU64Stark(16)
    zero = np.zeros((1, 96), dtype=np.uint32)
    _, p0 = S.power_instances(stark, zero, 0, 2)                             # 0^0 = 1, then 1^0 = 1
    assert PL.elem_from_words("fq12", p0[0][0].tolist()) == PL.FQ12_ONE == PL.elem_from_words("fq12", p0[0][1].tolist())
    _, p1 = S.power_instances(stark, zero, 5, 2)                             # 0^5 = 0
    assert not p1.any()
