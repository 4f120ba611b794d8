"""sbn_chain_instances on the host: the explicit instance list of a chained one (offset[0] = start, offset[k+1] = output[k]; the
reference's *_msm call shape) for all five Exp tables against Python integers (tests/chained_lists.py), exactly: every offset word,
the last output, any count, and the refusals -- a point off the curve, a coordinate >= p, an offset at infinity, a list the
table's own walk cannot take, and the accepted twin of that list."""
import numpy as np
import pytest

import chained_lists as CL
import tracegen_edges as T

TABLES = ["g1", "g2", "fq", "fq12", "fq12u64"]
BAD_ARG, NON_CANONICAL, WITNESS = -1, -2, -8


def _stark(S, table, count):
    return T.stark_class(S, table)(count)


def _chain(S, table, terms, start):
    return S.chain_instances(_stark(S, table, len(terms)), terms, start)


@pytest.mark.parametrize("table", TABLES)
def test_list_and_final_output_equal_python(S, table):
    """128 instances on the curves (the seeded list: identity terms, x = start, a repeated and an opposite instance, e = r,
    e = 2^256 - 1), 16 on the fields (0, one, p - 1 in one coefficient, random; exponents 0, 1 and the table's edge exponents)."""
    terms, start, insts, final = CL.chained_list(table)
    ios, fin = _chain(S, table, terms, start)
    want = T.pack(table, insts)
    bad = np.nonzero((ios != want).any(axis=1))[0]
    assert bad.size == 0, bad[:8].tolist()
    assert np.array_equal(fin, CL.value_words(table, final))
    # the list is the table's own: instance k's output in Python is instance k + 1's offset
    for k in (0, len(insts) // 2, len(insts) - 1):
        out = T.expected_output(table, insts[k])
        assert out == (insts[k + 1][1] if k + 1 < len(insts) else final)


@pytest.mark.parametrize("count", [1, 3, 128])
@pytest.mark.parametrize("table", TABLES)
def test_any_count(S, table, count):
    """Counts that are no power of two, one instance, and 128 of every table (a prefix of a chained list is a chained list)."""
    terms, start, insts, final = CL.chained_list(table, 128)
    ios, fin = _chain(S, table, terms[:count], start)
    assert np.array_equal(ios, T.pack(table, insts[:count]))
    last = final if count == len(insts) else insts[count][1]
    assert np.array_equal(fin, CL.value_words(table, last))


def test_final_output_is_optional(S):
    terms, start, insts, _ = CL.chained_list("fq")
    ios = np.zeros((len(terms), 24), dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)   # noqa: E731
    assert S.lib().sbn_chain_instances(S.FqExpStark.kind, ptr(terms), len(terms), ptr(start), ptr(ios), None) == 0
    assert np.array_equal(ios, T.pack("fq", insts))


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_point_off_the_curve_is_refused(S, curve):
    terms, start, _, _ = CL.chained_list(curve)
    for k in (0, 77, 127):
        bad = terms.copy()
        bad[k, 0] ^= 1                          # x.x (c0) changes, y stays: off the curve, still canonical
        with pytest.raises(S.SbnError) as e:
            _chain(S, curve, bad, start)
        assert e.value.code == BAD_ARG and f"instance {k}" in str(e.value), str(e.value)
    bad_start = start.copy()
    bad_start[0] ^= 1
    with pytest.raises(S.SbnError) as e:
        _chain(S, curve, terms, bad_start)
    assert e.value.code == BAD_ARG and "start" in str(e.value)


@pytest.mark.parametrize("table", TABLES)
def test_value_not_below_p_is_refused_as_the_generators_refuse_it(S, table):
    """A coordinate / coefficient = p: SBN_ERR_BAD_ARG, what sbn_generate_trace_* returns for it; Fq12U64: an exponent that is no
    canonical field element: SBN_ERR_NON_CANONICAL."""
    terms, start, insts, _ = CL.chained_list(table)
    p_words = np.array(T.limbs(T.P, 8, 32), dtype=np.uint32)
    bad = terms.copy()
    bad[3, 8 * (len(CL._flat(table, insts[0][0])) - 1):][:8] = p_words        # the last component of x[3]
    with pytest.raises(S.SbnError) as e:
        _chain(S, table, bad, start)
    assert e.value.code == BAD_ARG and "instance 3" in str(e.value), str(e.value)
    bad_start = start.copy()
    bad_start[:8] = p_words
    with pytest.raises(S.SbnError) as e:
        _chain(S, table, terms, bad_start)
    assert e.value.code == BAD_ARG
    if table in ("fq12", "fq12u64"):   # the explicit-list generator on the same value: the same code (it checks before it works)
        ios = T.pack(table, insts)
        ios[3, :8] = p_words
        with pytest.raises(S.SbnError) as e:
            _stark(S, table, len(insts)).generate_trace_and_public_inputs(ios)
        assert e.value.code == BAD_ARG
    if table == "fq12u64":
        bad = terms.copy()
        bad[5, 96:98] = (0xFFFFFFFF, 0xFFFFFFFF)
        with pytest.raises(S.SbnError) as e:
            _chain(S, table, bad, start)
        assert e.value.code == NON_CANONICAL


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_witness_refusals_and_the_accepted_twin(S, curve):
    """x[0] = -start with e[0] = 1 (offset[1] is the point at infinity) and an instance whose x is its own offset with an odd
    exponent (the table's first addition meets B = A) are refused with SBN_ERR_WITNESS; the twin of the second with bit 0 cleared
    walks clean in Python and is accepted, with Python's words."""
    cases = CL.witness_refusals(curve)
    for name in ("opposite", "collide"):
        xs, es, start = cases[name]
        with pytest.raises(S.SbnError) as e:
            _chain(S, curve, CL.terms_words(curve, xs, es), CL.value_words(curve, start))
        assert e.value.code == WITNESS, (name, str(e.value))
    xs, es, start = cases["twin"]
    insts, final = CL.derive(curve, xs, es, start)
    ios, fin = _chain(S, curve, CL.terms_words(curve, xs, es), CL.value_words(curve, start))
    assert np.array_equal(ios, T.pack(curve, insts))
    assert np.array_equal(fin, CL.value_words(curve, final))


def test_bad_arguments(S):
    terms, start, _, _ = CL.chained_list("fq")
    with pytest.raises(S.SbnError) as e:
        S.chain_instances(S.G1Stark(), terms, start)
    assert e.value.code == BAD_ARG
    with pytest.raises(S.SbnError) as e:
        S.chain_instances(S.FqExpStark(16), terms[:, :15], start)
    assert e.value.code == BAD_ARG
    ios = np.zeros((1, 24), dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)   # noqa: E731
    assert S.lib().sbn_chain_instances(S.FqExpStark.kind, ptr(terms), 0, ptr(start), ptr(ios), None) == BAD_ARG
    assert S.lib().sbn_chain_instances(S.G1Stark.kind, ptr(terms), 1, ptr(start), ptr(ios), None) == BAD_ARG
    assert S.lib().sbn_chain_instances(S.FqExpStark.kind, None, 1, ptr(start), ptr(ios), None) == BAD_ARG
