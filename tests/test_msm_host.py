"""Host tests of the long chained lists (include/sbn.h, "Long chained lists"; no device): sbn_msm_instances against the list
Python derives (tests/msm_lists.py) with the pad rule of the reference's g1_exp_circuit, its refusals by GLOBAL instance index,
and sbn_msm_check_links on the public inputs of the host generators: the good list, and every way the units can fail to be one
chained list."""
import numpy as np
import pytest

import chained_lists as CL
import msm_lists as ML
import tracegen_edges as T

BAD_ARG, VERIFY_FAILED, WITNESS = -1, -6, -8
TABLES = ("g1", "g2", "fq", "fq12", "fq12u64")


def _final_words(table, final):
    return CL.value_words(table, final)


@pytest.mark.parametrize("table", TABLES)
def test_msm_instances_equals_python(S, table):
    num_io, count = ML.SIZES[table]
    terms, start, insts, final, want = ML.msm_list(table)
    assert len(insts) == count and want.shape[0] == 3
    ios, fin = S.msm_instances(T.stark_class(S, table)(num_io), terms, start)
    assert ios.shape == want.shape
    flat, wflat = ios.reshape(-1, ios.shape[2]), want.reshape(-1, ios.shape[2])
    bad = np.nonzero((flat[:count] != T.pack(table, insts)).any(axis=1))[0]
    assert bad.size == 0, ("real rows", bad[:8].tolist())
    assert (flat[count:] == flat[count - 1]).all(), "pad rows are copies of row count - 1"
    assert np.array_equal(flat, wflat)
    assert np.array_equal(fin, _final_words(table, final))
    # rows [0, count) are exactly what sbn_chain_instances writes
    cios, cfin = S.chain_instances(T.stark_class(S, table)(num_io), terms, start)
    assert np.array_equal(cios, flat[:count]) and np.array_equal(cfin, fin)


@pytest.mark.parametrize("count", [256, 5])
def test_g1_no_pad_and_single_padded_unit(S, count):
    terms, start, insts, _, _ = ML.msm_list("g1")
    ios, fin = S.msm_instances(S.G1ExpStark(128), terms[:count], start)
    assert ios.shape == (ML.num_units(count, 128), 128, 40)
    want = ML.padded_units("g1", insts[:count], 128)
    assert np.array_equal(ios, want)
    assert np.array_equal(fin, CL.value_words("g1", insts[count][1]))     # the output of instance count - 1 = offset[count]


def test_num_units_and_empty_calls(S):
    L = S.lib()
    for count, num_io, want in ((0, 128, 0), (5, 0, 0), (0, 0, 0), (1, 128, 1), (127, 128, 1), (128, 128, 1), (129, 128, 2), (256, 128, 2),
                                (261, 128, 3), (35, 16, 3), (5000, 128, 40), (7, 1, 7)):
        assert L.sbn_msm_num_units(count, num_io) == want, (count, num_io)
    terms, start, _, _, _ = ML.msm_list("g1")
    ios = np.zeros((128, 40), dtype=np.uint32)
    p = lambda a: a.ctypes.data   # noqa: E731
    assert L.sbn_msm_instances(S.AIR_G1_EXP, p(terms), 0, 128, p(start), p(ios), None) == BAD_ARG
    assert L.sbn_msm_instances(S.AIR_G1_EXP, p(terms), 5, 0, p(start), p(ios), None) == BAD_ARG
    assert L.sbn_msm_instances(S.AIR_G1_OP, p(terms), 5, 128, p(start), p(ios), None) == BAD_ARG
    assert not ios.any()


def test_refusals_name_the_global_instance(S):
    stark = S.G1ExpStark(128)
    terms, start = ML.boundary_infinity("g1")
    with pytest.raises(S.SbnError) as e:
        S.msm_instances(stark, terms, start)
    assert e.value.code == WITNESS and "instance 128 " in str(e.value) and "infinity" in str(e.value), str(e.value)
    good, start, _, _, _ = ML.msm_list("g1")
    off_curve = good.copy()
    off_curve[258, 0] ^= 1
    with pytest.raises(S.SbnError) as e:
        S.msm_instances(stark, off_curve, start)
    assert e.value.code == BAD_ARG and "instance 258 " in str(e.value), str(e.value)
    not_below_p = good.copy()
    not_below_p[257, 8:16] = T.limbs(T.P, 8, 32)
    with pytest.raises(S.SbnError) as e:
        S.msm_instances(stark, not_below_p, start)
    assert e.value.code == BAD_ARG and "instance 257)" in str(e.value), str(e.value)


# ---------------------------------------------------------------- the link check
@pytest.fixture(scope="module", params=["g1", "fq12u64"])
def linked(S, request):
    """(table, stark, pis, terms, start, final): the public inputs of the host generator for every unit of the Python list."""
    table = request.param
    num_io, count = ML.SIZES[table]
    terms, start, _, final, units = ML.msm_list(table)
    stark = T.stark_class(S, table)(num_io)
    pis = [stark.generate_public_inputs(u) for u in units]
    return table, stark, pis, terms, start, final


def _rejects(S, stark, pis, count, start, terms, *names):
    with pytest.raises(S.SbnError) as e:
        S.msm_check_links(stark, pis, count, start, terms)
    assert e.value.code == VERIFY_FAILED, str(e.value)
    for n in names:
        assert n in str(e.value), str(e.value)


def test_check_links_accepts_the_good_list(S, linked):
    table, stark, pis, terms, start, final = linked
    count = ML.SIZES[table][1]
    want = _final_words(table, final)
    assert np.array_equal(S.msm_check_links(stark, pis, count, start), want)
    assert np.array_equal(S.msm_check_links(stark, pis, count, start, terms), want)
    assert T.outputs_from_pi(table, pis[2])[count - 1 - 2 * stark.num_io] == final


def test_check_links_rejections(S, linked):
    table, stark, pis, terms, start, _ = linked
    num_io, count = ML.SIZES[table]
    per, out_at = T.SHAPE[table][2], T.SHAPE[table][3]
    b = num_io - 1                                     # the boundary instance: its output is the carry into unit 1
    # units 0 and 1 swapped: the list no longer begins at start
    _rejects(S, stark, [pis[1], pis[0], pis[2]], count, start, None, "instance 0:", "start")
    changed = start.copy()
    changed[0] ^= 1
    _rejects(S, stark, pis, count, changed, None, "instance 0:", "start")
    # one output limb of the boundary instance flipped: the offset of instance b + 1 no longer continues it
    flipped = [p.copy() for p in pis]
    flipped[0][per * b + out_at + 3] ^= 1
    _rejects(S, stark, flipped, count, start, terms, f"instance {b + 1}:", f"output of instance {b}")
    # ... and the same inside a unit
    inner = [p.copy() for p in pis]
    inner[1][per * 4 + out_at] ^= 1
    _rejects(S, stark, inner, count, start, None, f"instance {num_io + 5}:", f"output of instance {num_io + 4}")
    # a pad row that differs from row count - 1, in each field
    r = count - 2 * num_io                             # first pad row of unit 2
    x_w = per - out_at                                 # public inputs of x = of the offset = of the output
    for field, at in (("x", 1), ("offset", x_w + 1), ("exponent", 2 * x_w), ("output", out_at + 2)):
        pad = [p.copy() for p in pis]
        pad[2][per * (r + 1) + at] ^= 1
        _rejects(S, stark, pad, count, start, None, f"instance {count + 1} (pad)", field, f"instance {count - 1}")
    # a wrong number of units
    _rejects(S, stark, pis[:2], count, start, None, "units")
    _rejects(S, stark, pis + [pis[2]], count, start, None, "units")
    _rejects(S, stark, pis, 2 * num_io, start, None, "units")
    # terms with one exponent limb, or one x limb, changed
    x_words = terms.shape[1] - (2 if table == "fq12u64" else 8)
    wrong = terms.copy()
    wrong[num_io + 7, x_words] ^= 1
    _rejects(S, stark, pis, count, start, wrong, f"instance {num_io + 7}:", "exponent")
    wrong = terms.copy()
    wrong[count - 1, 2] ^= 1 << 16
    _rejects(S, stark, pis, count, start, wrong, f"instance {count - 1}:", "x differs")
    # a shorter count turns real rows into pad rows that are no copies
    _rejects(S, stark, pis, count - 1, start, None, f"instance {count - 1} (pad)")
