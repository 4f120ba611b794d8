"""Host tests of the independent scalar multiplications (sbn_scalar_mul_instances, sbn_scalar_mul_check and the cofactor forms;
run with `-m "not gpu"`): the explicit, padded list, the products and the infinity flags equal Python's word for word on both
curves; every refusal returns its code and names its instance; the check accepts the public inputs of the host generators and
rejects every single-word edit naming the instance and the field.  The lists are tests/scalar_mul_lists.py."""
import re

import numpy as np
import pytest

import chained_lists as CL
import scalar_mul_lists as SL
import tracegen_edges as T

BAD_ARG, VERIFY_FAILED, UNSUPPORTED, WITNESS = -1, -6, -7, -8
CURVES = ["g1", "g2"]


def stark_of(S, curve, num_io=SL.NUM_IO):
    return T.stark_class(S, curve)(num_io)


def refused(S, code, names, fn, *args, **kw):
    with pytest.raises(S.SbnError) as e:
        fn(*args, **kw)
    assert e.value.code == code and re.search(names, str(e.value)), str(e.value)


@pytest.fixture(scope="module")
def pis(S):
    """The public inputs of the two units of each curve's seeded list, from the host generators, once."""
    cache = {}

    def get(curve):
        if curve not in cache:
            cache[curve] = SL.public_inputs(S, curve, SL.case(curve)[3])
        return cache[curve]
    return get


def test_generator_and_cofactor_are_the_reference_values(S):
    assert np.array_equal(S.generator(S.G1ExpStark(128)), CL.value_words("g1", T.G1_GEN))
    assert np.array_equal(S.generator(S.G2ExpStark(128)), CL.value_words("g2", T.G2_GEN))
    assert S.G2_COFACTOR == 2 * T.P - T.R == SL.G2_COFACTOR
    out = np.zeros(8, dtype=np.uint32)
    assert S.lib().sbn_g2_cofactor(out.ctypes.data) == 0 and T.from_limbs(out, 32) == 2 * T.P - T.R
    refused(S, UNSUPPORTED, "curve", S.generator, S.FqExpStark(128))


@pytest.mark.parametrize("curve", CURVES)
def test_instances_equal_python_word_for_word(S, curve):
    points, scalars, off, units, products, inf, _ = SL.case(curve)
    stark = stark_of(S, curve)
    ios, got, flags = S.scalar_mul_instances(stark, points, scalars, off)
    assert ios.shape == (2, SL.NUM_IO, units.shape[2]) and np.array_equal(ios, units)
    assert np.array_equal(flags, inf) and flags[[3, 11, 132]].tolist() == [1, 1, 1] and flags.sum() == 3
    assert np.array_equal(got, products)
    assert not got[[3, 11, 132]].any()                                       # an infinite product has zero words
    # offset=None is the generator
    ios2, got2, flags2 = S.scalar_mul_instances(stark, points, scalars)
    assert np.array_equal(ios2, ios) and np.array_equal(got2, got) and np.array_equal(flags2, flags)
    # a single padded unit and a table the list does not fill evenly
    ios3, got3, _ = S.scalar_mul_instances(stark, points[:5], scalars[:5], off)
    assert ios3.shape[0] == 1 and np.array_equal(ios3[0, :5], units[0, :5]) and np.array_equal(ios3[0, 5:], np.repeat(units[0, 4:5], 123, axis=0))
    assert np.array_equal(got3, products[:5])


@pytest.mark.parametrize("curve", CURVES)
def test_shared_scalar_equals_the_scalar_repeated(S, curve):
    points, _, off, _, _, _, _ = SL.case(curve)
    points = points[:129]                                                    # (instance 130 is x = offset: no odd scalar walks it)
    stark = stark_of(S, curve)
    e = SL.G2_COFACTOR if curve == "g2" else (1 << 255) + 12345
    one = SL.scalar_words([e])
    want = S.scalar_mul_instances(stark, points, np.repeat(one, 129, axis=0), off)
    for shared in (one, one[0], e):                                          # (1, 8), (8,), a Python int
        got = S.scalar_mul_instances(stark, points, shared, off)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_cofactor_clearing_equals_python(S):
    points, units, cleared = SL.cofactor_case()
    ios, got, flags = S.scalar_mul_instances(S.G2ExpStark(SL.NUM_IO), points, S.G2_COFACTOR)
    assert np.array_equal(ios, units) and np.array_equal(got, cleared) and not flags.any()


@pytest.mark.parametrize("curve", CURVES)
def test_refusals_name_their_instance(S, curve):
    points, scalars, off, _, _, _, _ = SL.case(curve)
    xs, es, offp, _, _ = SL.seeded_list(curve)
    add, neg, mul = T._ops(curve)
    stark = stark_of(S, curve)
    run = lambda p, s, o=off: S.scalar_mul_instances(stark, p, s, o)   # noqa: E731
    W = points.shape[1]
    bad = points.copy()
    bad[17, 8:16] = T.limbs(T.P, 8, 32)                                      # a coordinate >= p
    refused(S, BAD_ARG, r">= p.*instance 17\b", run, bad, scalars)
    bad = points.copy()
    bad[21, 0] ^= 1                                                          # a point off the curve
    refused(S, BAD_ARG, r"instance 21\b.*not a point of the curve", run, bad, scalars)
    bad_off = off.copy()
    bad_off[0] ^= 1
    refused(S, BAD_ARG, r"offset is not a point of the curve", run, points, scalars, bad_off)
    bad_off[W - 8:] = T.limbs(T.P, 8, 32)
    refused(S, BAD_ARG, r">= p \(offset\)", run, points, scalars, bad_off)
    refused(S, BAD_ARG, r"scalar_count", run, points, scalars[:2])           # scalar_count = 2
    # the table's own walk: x = offset with e = 1 (B[0] = A[0]) at 40, x = -offset with e = 3 (B[1] = -A[1]... B[0] = -A[0]) at 30
    cx, ce = list(xs), list(es)
    cx[40], ce[40] = offp, 1
    refused(S, WITNESS, r"instance 40\b", run, SL.point_words(curve, cx), SL.scalar_words(ce))
    cx[30], ce[30] = neg(offp), 3
    refused(S, WITNESS, r"instance 30\b", run, SL.point_words(curve, cx), SL.scalar_words(ce))   # the FIRST of the two
    # e x = -offset: the output itself is the point at infinity
    cx, ce = list(xs), list(es)
    cx[131], ce[131] = neg(mul(offp, pow(5, -1, T.R))), 5                    # offset is in the prime-order subgroup on both curves
    assert add(offp, mul(cx[131], 5)) is None
    refused(S, WITNESS, r"instance 131\b", run, SL.point_words(curve, cx), SL.scalar_words(ce))


def test_field_tables_and_cofactor_forms_on_g1_are_refused(S):
    pts, sc = np.zeros((4, 16), dtype=np.uint32), np.ones((4, 8), dtype=np.uint32)
    L = S.lib()
    for kind in (S.AIR_FQ_EXP, S.AIR_FQ12_EXP, S.AIR_FQ12_EXP_U64, S.AIR_G1_OP):
        assert L.sbn_scalar_mul_instances(kind, pts.ctypes.data, sc.ctypes.data, 4, 4, 128, None, None, None, None) == UNSUPPORTED
        assert L.sbn_scalar_mul_check(kind, 128, None, 1, 4, pts.ctypes.data, sc.ctypes.data, 4, None, None, None) == UNSUPPORTED
    assert L.sbn_scalar_mul_instances(S.AIR_G1_EXP, None, sc.ctypes.data, 4, 4, 128, None, None, None, None) == BAD_ARG
    assert L.sbn_scalar_mul_instances(S.AIR_G1_EXP, pts.ctypes.data, sc.ctypes.data, 4, 0, 128, None, None, None, None) == BAD_ARG
    refused(S, UNSUPPORTED, "curve", S.scalar_mul_instances, S.FqExpStark(128), pts, sc)
    refused(S, BAD_ARG, "G2ExpStark", S.mul_by_cofactor_check, S.G1ExpStark(128), [], pts)


@pytest.mark.parametrize("curve", CURVES)
def test_check_accepts_the_host_generators_and_returns_pythons_products(S, curve, pis):
    points, scalars, off, _, products, inf, outputs = SL.case(curve)
    stark = stark_of(S, curve)
    pi = pis(curve)
    assert T.outputs_from_pi(curve, pi[0]) == outputs[:SL.NUM_IO] and T.outputs_from_pi(curve, pi[1])[:5] == outputs[SL.NUM_IO:]
    got, flags = S.scalar_mul_check(stark, pi, points, scalars, off)
    assert np.array_equal(got, products) and np.array_equal(flags, inf)
    got, flags = S.scalar_mul_check(stark, pi, points, scalars)              # offset=None: the generator
    assert np.array_equal(got, products) and np.array_equal(flags, inf)


@pytest.mark.parametrize("curve", CURVES)
def test_check_rejects_every_single_word_edit(S, curve, pis):
    points, scalars, off, _, _, _, _ = SL.case(curve)
    stark = stark_of(S, curve)
    W = points.shape[1]
    per, oOff, oExp, oOut = 3 * W + 8, W, 2 * W, 2 * W + 8
    good = pis(curve)

    def edited(g, at, fn):
        pi = [p.copy() for p in good]
        u, k = divmod(g, SL.NUM_IO)
        pi[u][per * k + at] = fn(int(pi[u][per * k + at]))
        return pi
    flip = lambda v: v ^ 1   # noqa: E731
    check = lambda pi: S.scalar_mul_check(stark, pi, points, scalars, off)   # noqa: E731
    refused(S, VERIFY_FAILED, r"instance 19: x ", check, edited(19, 3, flip))
    refused(S, VERIFY_FAILED, r"instance 129: exponent", check, edited(129, oExp + 7, flip))
    refused(S, VERIFY_FAILED, r"instance 64: offset", check, edited(64, oOff + 1, flip))
    refused(S, VERIFY_FAILED, r"instance 2: output limb 5 is out of range", check, edited(2, oOut + 5, lambda v: v | (1 << 32)))
    refused(S, VERIFY_FAILED, r"instance 131: output is not a point of the curve", check, edited(131, oOut, flip))
    for f, (name, at) in enumerate((("x", 0), ("offset", oOff + 2), ("exponent", oExp), ("output", oOut + W - 1))):
        g = 133 + 30 * f                                                     # pad rows 133, 163, 193, 223
        refused(S, VERIFY_FAILED, rf"instance {g} \(pad\): {name} differs from instance 132", check, edited(g, at, flip))
    refused(S, VERIFY_FAILED, r"1 units given", check, good[:1])             # one unit too few
    # the caller's own list differs: a point, a scalar, another offset
    other = points.copy()
    other[4] = points[8]
    refused(S, VERIFY_FAILED, r"instance 4: x ", lambda: S.scalar_mul_check(stark, good, other, scalars, off))
    refused(S, VERIFY_FAILED, r"instance 0: offset", lambda: S.scalar_mul_check(stark, good, points, scalars, points[0]))


def test_cofactor_check_agrees(S):
    points, units, cleared = SL.cofactor_case()
    stark = S.G2ExpStark(SL.NUM_IO)
    pi = SL.public_inputs(S, "g2", units)
    got, flags = S.mul_by_cofactor_check(stark, pi, points)
    assert np.array_equal(got, cleared) and not flags.any()
    assert all(np.array_equal(a, b) for a, b in zip(S.scalar_mul_check(stark, pi, points, S.G2_COFACTOR), (got, flags)))
    pi[1][104 + 32] ^= 1                                                        # instance 129 of the list: its offset
    refused(S, VERIFY_FAILED, r"instance 129: offset", S.mul_by_cofactor_check, stark, pi, points)
