"""Host tests of the batches of short MSMs (include/sbn.h, "Batches of short MSMs"; no device): sbn_msm_batch_instances against
the segmented lists Python derives (tests/msm_batches.py) on all five tables, its two ends (one segment = sbn_msm_instances,
lengths all 1 with a shared start = sbn_scalar_mul_instances), its refusals by GLOBAL instance and segment, and
sbn_msm_batch_check on the public inputs of the host generators: the good list, and every way the units can fail to be it."""
import re

import numpy as np
import pytest

import chained_lists as CL
import msm_batches as MB
import msm_lists as ML
import scalar_mul_lists as SM
import tracegen_edges as T

BAD_ARG, NON_CANONICAL, VERIFY_FAILED, UNSUPPORTED, WITNESS = -1, -2, -6, -7, -8
UNITS = [("g1", 128), ("g2", 128), ("fq", 128), ("fq12", 16), ("fq12u64", 16), ("fq12u64", 64)]


def test_symbols_are_exported(S):
    for name in ("sbn_msm_batch_instances", "sbn_prover_generate_trace_msm_batch", "sbn_batch_prover_prove_msm_batch", "sbn_msm_batch_check"):
        assert name in S.EXPORTS and hasattr(S.lib(), name), name


def _unit_case(table, num_io, shared):
    """(terms, lengths, starts_words or None, insts, finals, sums) of the table's one-unit recipe."""
    if table in ("g1", "g2"):
        xs, es, starts, insts, finals, sums = MB.curve_unit(table, shared)
        lengths = MB.CURVE_LENGTHS
    else:
        xs, es, starts, insts, finals = MB.field_unit(table, num_io, shared)
        lengths, sums = MB.field_lengths(num_io), None
    return CL.terms_words(table, xs, es), MB.lengths_words(lengths), (None if shared else MB.starts_words(table, starts)), insts, finals, sums


def _assert_outputs(table, got, finals, sums):
    fin, sm, inf = got
    assert np.array_equal(fin, MB.starts_words(table, finals))
    if table in ("g1", "g2"):
        assert np.array_equal(sm, MB.point_words(table, sums)) and np.array_equal(inf, MB.flags(sums))
    else:
        assert sm is None and inf is None


@pytest.mark.parametrize("shared", [False, True], ids=["starts", "default"])
@pytest.mark.parametrize("table,num_io", UNITS, ids=lambda v: str(v))
def test_instances_equal_python(S, table, num_io, shared):
    terms, lengths, starts, insts, finals, sums = _unit_case(table, num_io, shared)
    M = len(insts)
    ios, *outs = S.msm_batch_instances(T.stark_class(S, table)(num_io), terms, lengths, starts)
    assert ios.shape == (1, num_io, T.SHAPE[table][1]) and M < num_io
    bad = np.nonzero((ios[0, :M] != T.pack(table, insts)).any(axis=1))[0]
    assert bad.size == 0, ("real rows", bad[:8].tolist())
    assert (ios[0, M:] == ios[0, M - 1]).all(), "pad rows are copies of row M - 1"
    _assert_outputs(table, outs, finals, sums)


@pytest.mark.parametrize("table", ["g1", "fq12"])
def test_segments_straddle_unit_boundaries(S, table):
    num_io, lengths, xs, es, starts, insts, finals, sums = MB.batch_list(table)
    ios, *outs = S.msm_batch_instances(T.stark_class(S, table)(num_io), CL.terms_words(table, xs, es), MB.lengths_words(lengths), MB.starts_words(table, starts))
    assert np.array_equal(ios, MB.padded(table, insts, num_io)) and ios.shape[0] == 3
    _assert_outputs(table, outs, finals, sums)


@pytest.mark.parametrize("table", ["g1", "g2", "fq", "fq12", "fq12u64"])
def test_one_segment_is_msm_instances(S, table):
    num_io, count = ML.SIZES[table]
    terms, start, _, _, _ = ML.msm_list(table)
    stark = T.stark_class(S, table)(num_io)
    want_ios, want_final = S.msm_instances(stark, terms, start)
    ios, fin, _, _ = S.msm_batch_instances(stark, terms, [count], start)
    assert np.array_equal(ios, want_ios) and np.array_equal(fin[0], want_final)


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_unit_segments_with_a_shared_start_are_scalar_muls(S, curve):
    points, scalars, offset, _, _, _, _ = SM.case(curve)
    stark = T.stark_class(S, curve)(SM.NUM_IO)
    want_ios, want_products, want_inf = S.scalar_mul_instances(stark, points, scalars, offset)
    terms = np.concatenate([points, scalars], axis=1)
    for starts in (offset, None):                       # the offset of that list is the generator: the default start
        ios, _, sums, inf = S.msm_batch_instances(stark, terms, [1] * SM.COUNT, starts)
        assert np.array_equal(ios, want_ios) and np.array_equal(sums, want_products) and np.array_equal(inf, want_inf)


# ---------------------------------------------------------------- refusals
def _refused(S, stark, terms, lengths, starts, code, pattern):
    with pytest.raises(S.SbnError) as e:
        S.msm_batch_instances(stark, terms, lengths, starts)
    assert e.value.code == code and re.search(pattern, str(e.value)), str(e.value)


def test_argument_refusals(S):
    terms, lengths, starts, _, _, _ = _unit_case("g1", 128, False)
    stark = S.G1ExpStark(128)
    L = S.lib()
    p = lambda a: a.ctypes.data   # noqa: E731
    ios = np.zeros((128, 40), dtype=np.uint32)
    zero = lengths.copy()
    zero[3], zero[4] = 60, 0                             # the same sum: the C call sees a zero length in segment 4 (instance 64)
    assert L.sbn_msm_batch_instances(S.AIR_G1_EXP, p(terms), p(zero), 8, p(starts), 8, 128, p(ios), None, None, None) == BAD_ARG
    msg = L.sbn_last_error().decode()
    assert re.search(r"segment 4\b", msg) and re.search(r"instance 64\b", msg), msg
    with pytest.raises(S.SbnError) as e:                 # the wrapper adds the lengths up
        S.msm_batch_instances(stark, terms, list(lengths[:-1]) + [int(lengths[-1]) + 1], starts)
    assert e.value.code == BAD_ARG and "122" in str(e.value) and "121" in str(e.value), str(e.value)
    three = np.array([1, 1, 119], dtype=np.uint64)
    assert L.sbn_msm_batch_instances(S.AIR_G1_EXP, p(terms), p(three), 3, p(starts), 2, 128, p(ios), None, None, None) == BAD_ARG
    assert "start_count" in L.sbn_last_error().decode()
    assert L.sbn_msm_batch_instances(S.AIR_G1_EXP, p(terms), p(lengths), 0, p(starts), 8, 128, p(ios), None, None, None) == BAD_ARG
    assert L.sbn_msm_batch_instances(S.AIR_G1_EXP, p(terms), p(lengths), 8, p(starts), 8, 0, p(ios), None, None, None) == BAD_ARG
    assert L.sbn_msm_batch_instances(S.AIR_G1_EXP, None, p(lengths), 8, p(starts), 8, 128, p(ios), None, None, None) == BAD_ARG
    assert L.sbn_msm_batch_instances(S.AIR_G1_OP, p(terms), p(lengths), 8, p(starts), 8, 128, p(ios), None, None, None) == UNSUPPORTED
    fterms, flengths, fstarts, _, _, _ = _unit_case("fq", 128, False)
    sums = np.zeros((len(flengths), 8), dtype=np.uint32)
    assert L.sbn_msm_batch_instances(S.AIR_FQ_EXP, p(fterms), p(flengths), len(flengths), p(fstarts), len(flengths), 128, None, None, p(sums), None) == BAD_ARG
    assert "sums_out" in L.sbn_last_error().decode()
    assert not ios.any()


def test_value_refusals_name_the_instance_and_its_segment(S):
    terms, lengths, starts, _, _, _ = _unit_case("g1", 128, False)
    stark = S.G1ExpStark(128)
    off_curve = terms.copy()
    off_curve[70, 0] ^= 1
    _refused(S, stark, off_curve, lengths, starts, BAD_ARG, r"instance 70 \(segment 5\).*curve")
    not_below_p = terms.copy()
    not_below_p[99, 8:16] = T.limbs(T.P, 8, 32)
    _refused(S, stark, not_below_p, lengths, starts, BAD_ARG, r">= p \(instance 99, segment 6\)")
    bad_start = starts.copy()
    bad_start[3, 0] ^= 1
    _refused(S, stark, terms, lengths, bad_start, BAD_ARG, r"start 3\b")
    fterms, flengths, fstarts, _, _, _ = _unit_case("fq12", 16, False)
    big = fterms.copy()
    big[9, 88:96] = T.limbs(T.P, 8, 32)
    _refused(S, S.Fq12ExpStark(16), big, flengths, fstarts, BAD_ARG, r"coefficient >= p \(instance 9, segment 3\)")
    uterms, ulengths, ustarts, _, _, _ = _unit_case("fq12u64", 16, False)
    nc = uterms.copy()
    nc[5, 96:98] = T.limbs(T.GLP, 2, 32)
    _refused(S, S.Fq12ExpU64Stark(16), nc, ulengths, ustarts, NON_CANONICAL, r"instance 5 \(segment 2\)")


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_witness_refusals_and_the_accepted_twin(S, curve):
    cases, starts = MB.refusal_lists(curve)
    stark = T.stark_class(S, curve)(128)
    sw, lengths = MB.starts_words(curve, starts), MB.lengths_words(MB.CURVE_LENGTHS)
    words = lambda name: CL.terms_words(curve, *cases[name])   # noqa: E731
    _refused(S, stark, words("infinity"), lengths, sw, WITNESS, r"offset of instance 65 \(segment 5\).*infinity")
    _refused(S, stark, words("collide"), lengths, sw, WITNESS, r"instance 97 \(segment 6\).*degenerate")
    insts, finals = MB.derive(curve, *cases["twin"], MB.CURVE_LENGTHS, starts)
    ios, fin, sums, inf = S.msm_batch_instances(stark, words("twin"), lengths, sw)
    assert np.array_equal(ios, MB.padded(curve, insts, 128))
    _assert_outputs(curve, (fin, sums, inf), finals, MB.sums_of(curve, finals, starts))


# ---------------------------------------------------------------- the check on the public inputs
@pytest.fixture(scope="module", params=["g1", "fq12"])
def batch(S, request):
    """(table, stark, pis, terms, lengths, starts, finals, sums): the public inputs of the host generator for every unit of the
    batch-prover recipe (three units, a segment across each boundary)."""
    table = request.param
    num_io, lengths, xs, es, starts, insts, finals, sums = MB.batch_list(table)
    stark = T.stark_class(S, table)(num_io)
    pis = [stark.generate_public_inputs(u) for u in MB.padded(table, insts, num_io)]
    return table, stark, pis, CL.terms_words(table, xs, es), MB.lengths_words(lengths), MB.starts_words(table, starts), finals, sums


def _rejects(S, stark, pis, lengths, starts, terms, *patterns):
    with pytest.raises(S.SbnError) as e:
        S.msm_batch_check(stark, pis, lengths, starts, terms)
    assert e.value.code == VERIFY_FAILED, str(e.value)
    for pat in patterns:
        assert re.search(pat, str(e.value)), (pat, str(e.value))


def test_check_accepts_the_good_list(S, batch):
    table, stark, pis, terms, lengths, starts, finals, sums = batch
    _assert_outputs(table, S.msm_batch_check(stark, pis, lengths, starts), finals, sums)
    _assert_outputs(table, S.msm_batch_check(stark, pis, lengths, starts, terms), finals, sums)


def test_check_rejections(S, batch):
    table, stark, pis, terms, lengths, starts, _, _ = batch
    num_io = stark.num_io
    per, out_at = T.SHAPE[table][2], T.SHAPE[table][3]
    x_w = per - out_at
    hs = MB.heads([int(n) for n in lengths])
    M = int(lengths.sum())
    seg_of = lambda g: max(s for s, h in enumerate(hs) if h <= g)   # noqa: E731
    # a head offset changed: segment 3 no longer begins at its start
    h = hs[3]
    head = [p.copy() for p in pis]
    head[h // num_io][per * (h % num_io) + x_w] ^= 1
    _rejects(S, stark, head, lengths, starts, terms, rf"instance {h} \(segment 3\)", "start")
    changed = starts.copy()
    changed[5, 0] ^= 1
    _rejects(S, stark, pis, lengths, changed, None, rf"instance {hs[5]} \(segment 5\)", "start")
    # a link broken across the unit boundary: one output limb of instance num_io - 1 flipped
    b = num_io - 1
    assert seg_of(b) == seg_of(b + 1)
    link = [p.copy() for p in pis]
    link[0][per * b + out_at + 3] ^= 1
    _rejects(S, stark, link, lengths, starts, terms, rf"instance {b + 1} \(segment {seg_of(b)}\)", rf"output of instance {b}\b")
    # ... while the output of a TAIL is no link: flipping it changes the final only (on the curves it is no curve point any more)
    tail = hs[4] - 1
    loose = [p.copy() for p in pis]
    loose[tail // num_io][per * (tail % num_io) + out_at] ^= 1
    if table == "g1":
        _rejects(S, stark, loose, lengths, starts, None, rf"instance {tail} \(segment 3\)", "curve")
    else:
        fin, _, _ = S.msm_batch_check(stark, loose, lengths, starts)
        assert int(fin[3, 0]) & 0xFFFF == int(pis[tail // num_io][per * (tail % num_io) + out_at]) ^ 1
    # a pad changed, in each field
    r = M - 2 * num_io
    for field, at in (("x", 1), ("offset", x_w + 1), ("exponent", 2 * x_w), ("output", out_at + 2)):
        pad = [p.copy() for p in pis]
        pad[2][per * (r + 1) + at] ^= 1
        _rejects(S, stark, pad, lengths, starts, None, rf"instance {M + 1} \(pad\)", field, rf"instance {M - 1}\b")
    # a caller term changed
    wrong = terms.copy()
    wrong[num_io + 7, x_w if table == "g1" else 96] ^= 1
    _rejects(S, stark, pis, lengths, starts, wrong, rf"instance {num_io + 7} \(segment {seg_of(num_io + 7)}\)", "exponent")
    wrong = terms.copy()
    wrong[M - 1, 2] ^= 1 << 16
    _rejects(S, stark, pis, lengths, starts, wrong, rf"instance {M - 1} \(segment {len(hs) - 1}\)", "x differs")
    # units swapped, and a wrong number of units
    _rejects(S, stark, [pis[1], pis[0], pis[2]], lengths, starts, None, r"instance 0 \(segment 0\)", "start")
    _rejects(S, stark, pis[:2], lengths, starts, None, "units")
