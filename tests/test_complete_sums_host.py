"""Host tests of the complete sums (include/sbn.h, "Complete sums"; no device): the start candidates against their rule in Python
integers, sbn_msm_batch_instances_complete against the model of tests/complete_sums.py on both curve tables with num_io = 4 (so
that segments straddle unit boundaries) -- the traps the default start refuses, head and middle kills, masks -- its defining
property against sbn_msm_batch_instances and sbn_msm_batch_check, the exhausted list and the argument refusals in header order."""
import re

import numpy as np
import pytest

import chained_lists as CL
import complete_sums as CS
import msm_batches as MB
import tracegen_edges as T

BAD_ARG, VERIFY_FAILED, UNSUPPORTED, WITNESS = -1, -6, -7, -8
NUM_IO = 4
CURVES = ["g1", "g2"]
CASES = ["random", "traps", "head", "middle", "masks"]


def test_symbols_are_exported(S):
    for name in ("sbn_start_candidate", "sbn_msm_batch_instances_complete", "sbn_prover_generate_trace_msm_batch_complete",
                 "sbn_batch_prover_prove_msm_batch_complete"):
        assert name in S.EXPORTS and hasattr(S.lib(), name), name
    assert S.START_CANDIDATES == CS.CANDIDATES == 8


@pytest.mark.parametrize("curve", CURVES)
def test_candidates_follow_their_rule(S, curve):
    stark = T.stark_class(S, curve)(NUM_IO)
    want = CS.candidates(curve)
    got = np.array([S.start_candidate(stark, j) for j in range(S.START_CANDIDATES)])
    assert np.array_equal(got, MB.starts_words(curve, want))
    assert all(CS.on_curve(curve, c) for c in want)
    assert CS.GEN[curve] not in want and len(set(want)) == 8
    assert not np.array_equal(got[0], S.generator(stark))
    if curve == "g1":
        assert [c[0] for c in want] == [2, 3, 5, 6, 7, 8, 9, 11]
    else:
        assert [c[0] for c in want] == [(k, 1) for k in (0, 2, 3, 4, 5, 6, 8, 11)]
    with pytest.raises(S.SbnError) as e:
        S.start_candidate(stark, 8)
    assert e.value.code == BAD_ARG
    L = S.lib()
    out = np.zeros(32, dtype=np.uint32)
    assert L.sbn_start_candidate(S.AIR_FQ_EXP, 0, out.ctypes.data) == UNSUPPORTED      # as sbn_curve_generator
    assert L.sbn_start_candidate(S.AIR_G1_OP, 0, out.ctypes.data) == UNSUPPORTED
    assert L.sbn_start_candidate(stark.kind, 0, None) == BAD_ARG and not out.any()


@pytest.fixture(scope="module")
def derived(S):
    """(stark, caller's terms, lengths, masks, outputs of the complete call, Python's model) per (curve, case), computed once."""
    cache = {}

    def get(curve, name):
        if (curve, name) not in cache:
            xs, es, lengths, masks, want = CS.host_cases(curve)[name]
            stark = T.stark_class(S, curve)(NUM_IO)
            terms = CS.words(curve, xs, es, masks)
            got = S.msm_batch_instances_complete(stark, terms, lengths, masks)
            cache[curve, name] = (stark, terms, MB.lengths_words(lengths), masks, got, CS.model(curve, xs, es, lengths, masks), want)
        return cache[curve, name]
    return get


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("curve", CURVES)
def test_complete_call_equals_python(S, derived, curve, name):
    """The choice, the starts, the effective terms, the list, the finals and the sums are Python's; the sums are also the plain
    sums of e_k x_k, which no start enters."""
    stark, terms, lengths, masks, got, model, want = derived(curve, name)
    ios, eff, starts, choice, finals, sums, inf = got
    ex, ee, m_choice, m_starts, insts, m_finals, m_sums = model
    assert choice.tolist() == want == m_choice
    assert np.array_equal(starts, MB.starts_words(curve, m_starts))
    assert np.array_equal(eff, CL.terms_words(curve, ex, ee))
    assert np.array_equal(ios, MB.padded(curve, insts, NUM_IO)) and ios.shape[0] == -(-len(insts) // NUM_IO)
    assert np.array_equal(finals, MB.starts_words(curve, m_finals))
    assert np.array_equal(sums, MB.point_words(curve, m_sums)) and np.array_equal(inf, MB.flags(m_sums))
    hs = MB.heads([int(n) for n in lengths])
    plain = [CS.sum_of(curve, ex[h:h + int(n)], ee[h:h + int(n)]) for h, n in zip(hs, lengths)]
    assert plain == m_sums
    for s, (h, n) in enumerate(zip(hs, lengths)):                      # a masked term is (generator, 0); a sum at infinity keeps its start
        for g in range(h, h + int(n)):
            if masks and masks[g]:
                assert np.array_equal(eff[g, :-8], S.generator(stark)) and not eff[g, -8:].any()
        if m_sums[s] is None:
            assert np.array_equal(finals[s], starts[s]) and not sums[s].any() and inf[s] == 1


def _public_inputs(curve, ios, lengths, finals):
    """The public inputs of the units as the tables lay them out (x, offset, exponent, output, one u32 limb per word), built here:
    the output of an instance is the offset of the next one of its segment, or the final; a pad repeats instance M - 1."""
    num_io, M = ios.shape[1], int(np.sum(lengths))
    rows = ios.reshape(-1, ios.shape[2])
    tails = {h + int(n) - 1: s for s, (h, n) in enumerate(zip(MB.heads([int(v) for v in lengths]), lengths))}
    w = rows.shape[1] // 2 - 4
    outs = [finals[tails[g]] if g in tails else rows[g + 1, w:2 * w] for g in range(M)]
    outs += [outs[M - 1]] * (len(rows) - M)
    pi = np.concatenate([rows, np.array(outs, dtype=np.uint32)], axis=1).astype(np.uint64)
    return [np.ascontiguousarray(pi[u * num_io:(u + 1) * num_io].reshape(-1)) for u in range(ios.shape[0])]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("curve", CURVES)
def test_defining_property(S, derived, curve, name):
    """Word for word what sbn_msm_batch_instances returns on (terms_eff, starts), which succeeds; sbn_msm_batch_check accepts the
    public inputs the host generator builds from the list, with the effective terms and the returned starts."""
    stark, terms, lengths, masks, got, _, _ = derived(curve, name)
    ios, eff, starts, choice, finals, sums, inf = got
    e_ios, e_finals, e_sums, e_inf = S.msm_batch_instances(stark, eff, lengths, starts)
    assert np.array_equal(ios, e_ios) and np.array_equal(finals, e_finals) and np.array_equal(sums, e_sums) and np.array_equal(inf, e_inf)
    assert (ios.reshape(-1, ios.shape[2])[len(eff):] == ios.reshape(-1, ios.shape[2])[len(eff) - 1]).all(), "pads copy row M - 1, offset included"
    pis = _public_inputs(curve, ios, lengths, finals)
    c_finals, c_sums, c_inf = S.msm_batch_check(stark, pis, lengths, starts, eff)
    assert np.array_equal(c_finals, finals) and np.array_equal(c_sums, sums) and np.array_equal(c_inf, inf)
    wrong = starts.copy()                                              # ... and it is a check: the generator is not the start
    wrong[0] = S.generator(stark)
    with pytest.raises(S.SbnError) as e:
        S.msm_batch_check(stark, pis, lengths, wrong, eff)
    assert e.value.code == VERIFY_FAILED and "instance 0 (segment 0)" in str(e.value), str(e.value)


@pytest.mark.parametrize("curve", CURVES)
def test_check_accepts_the_host_generators_public_inputs(S, curve):
    """The head case in a table of 128 (the smallest the host generator writes): sbn_msm_batch_check accepts the public inputs
    of the host generator on the list of the complete call, and returns its finals, sums and flags."""
    xs, es, lengths, masks, want = CS.host_cases(curve)["head"]
    stark = T.stark_class(S, curve)(128)
    ios, eff, starts, choice, finals, sums, inf = S.msm_batch_instances_complete(stark, CS.words(curve, xs, es, masks), lengths)
    assert choice.tolist() == want and ios.shape[0] == 1
    got = S.msm_batch_check(stark, [stark.generate_public_inputs(ios[0])], lengths, starts, eff)
    assert np.array_equal(got[0], finals) and np.array_equal(got[1], sums) and np.array_equal(got[2], inf)


@pytest.mark.parametrize("curve", CURVES)
def test_the_default_start_refuses_the_traps(S, curve):
    """What the feature is for: the same lists through sbn_msm_batch_instances with its default start are refused."""
    xs, es, lengths, _, _ = CS.host_cases(curve)["traps"]
    with pytest.raises(S.SbnError) as e:
        S.msm_batch_instances(T.stark_class(S, curve)(NUM_IO), CL.terms_words(curve, xs, es), lengths)
    assert e.value.code == WITNESS and "instance 0 (segment 0)" in str(e.value), str(e.value)


@pytest.mark.parametrize("curve", CURVES)
def test_choice_is_a_function_of_the_segment_alone(S, derived, curve):
    """Every segment of the head case on its own gets the choice it got among its neighbours."""
    stark, terms, lengths, _, got, _, want = derived(curve, "head")
    for s, (h, n) in enumerate(zip(MB.heads([int(v) for v in lengths]), lengths)):
        alone = S.msm_batch_instances_complete(stark, terms[h:h + int(n)], [int(n)])
        assert alone[3].tolist() == [want[s]] and np.array_equal(alone[4][0], got[4][s]) and np.array_equal(alone[5][0], got[5][s])


@pytest.mark.parametrize("curve", CURVES)
def test_exhausted_candidates(S, curve):
    xs, es, lengths, seg, inst, own = CS.exhausted(curve)
    stark = T.stark_class(S, curve)(NUM_IO)
    terms = CL.terms_words(curve, xs, es)
    with pytest.raises(S.SbnError) as e:
        S.msm_batch_instances_complete(stark, terms, lengths)
    msg = str(e.value)
    assert e.value.code == WITNESS and re.search(rf"segment {seg}\b", msg) and re.search(r"\b1 segment\b", msg), msg
    assert re.search(rf"candidate 7 fails at instance {inst}\b", msg) and "sbn_msm_batch_instances" in msg, msg
    two = np.concatenate([terms, terms[2:10]])                        # the same segment again: two segments in this state
    with pytest.raises(S.SbnError) as e:
        S.msm_batch_instances_complete(stark, two, lengths + [8])
    assert e.value.code == WITNESS and re.search(rf"segment {seg}\b", str(e.value)) and "2 segments" in str(e.value), str(e.value)
    starts = MB.starts_words(curve, [own] * 3)                        # starts of the caller's own take the same terms
    ios, finals, sums, inf = S.msm_batch_instances(stark, terms, lengths, starts)
    assert np.array_equal(sums[1], MB.point_words(curve, [CS.sum_of(curve, xs[2:10], es[2:10])])[0]) and not inf.any()


def test_argument_refusals_in_header_order(S):
    xs, es, lengths, _, _ = CS.host_cases("g1")["random"]
    terms, lw = CL.terms_words("g1", xs, es), MB.lengths_words(lengths)
    L = S.lib()
    p = lambda a: a.ctypes.data   # noqa: E731
    ios = np.zeros((12, 40), dtype=np.uint32)
    choice = np.full(4, 9, dtype=np.uint8)

    def call(kind, t, ln, segs, num_io, mask=None):
        rc = L.sbn_msm_batch_instances_complete(kind, t, mask, ln, segs, num_io, p(ios), None, None, p(choice), None, None, None)
        return rc, L.sbn_last_error().decode()
    # the kind before anything else: no Exp table, then the three field tables
    assert call(S.AIR_G1_OP, None, None, 0, 0)[0] == UNSUPPORTED
    for kind in (S.AIR_FQ_EXP, S.AIR_FQ12_EXP, S.AIR_FQ12_EXP_U64):
        rc, msg = call(kind, None, None, 0, 0)
        assert rc == UNSUPPORTED and "G1_EXP and G2_EXP" in msg, msg
    # the arguments, in the order of sbn_msm_batch_instances: null, no segment, a zero length, num_io = 0
    assert call(S.AIR_G1_EXP, None, p(lw), 0, 0)[0] == BAD_ARG and "null" in L.sbn_last_error().decode()
    assert call(S.AIR_G1_EXP, p(terms), None, 4, NUM_IO)[0] == BAD_ARG
    rc, msg = call(S.AIR_G1_EXP, p(terms), p(lw), 0, 0)
    assert rc == BAD_ARG and "no segment" in msg, msg
    zero = np.array([1, 2, 0, 8], dtype=np.uint64)
    rc, msg = call(S.AIR_G1_EXP, p(terms), p(zero), 4, 0)
    assert rc == BAD_ARG and re.search(r"segment 2\b", msg) and re.search(r"instance 3\b", msg), msg
    rc, msg = call(S.AIR_G1_EXP, p(terms), p(lw), 4, 0)
    assert rc == BAD_ARG and "num_io" in msg, msg
    # the values of the terms that are not masked, naming the instance and its segment: >= p before off the curve
    both = terms.copy()
    both[2, 0] ^= 1
    both[9, 8:16] = T.limbs(T.P, 8, 32)
    rc, msg = call(S.AIR_G1_EXP, p(both), p(lw), 4, NUM_IO)
    assert rc == BAD_ARG and re.search(r">= p \(instance 9, segment 3\)", msg), msg
    mask = np.zeros(11, dtype=np.uint8)
    mask[9] = 1
    rc, msg = call(S.AIR_G1_EXP, p(both), p(lw), 4, NUM_IO, p(mask))
    assert rc == BAD_ARG and re.search(r"instance 2 \(segment 1\).*curve", msg), msg
    assert not ios.any() and (choice == 9).all()
    mask[2] = 1                                                       # both masked: accepted
    assert call(S.AIR_G1_EXP, p(both), p(lw), 4, NUM_IO, p(mask))[0] == 0 and not choice.any()
    # the wrapper's own checks
    stark = S.G1ExpStark(NUM_IO)
    with pytest.raises(S.SbnError) as e:
        S.msm_batch_instances_complete(stark, terms, lengths, np.zeros(3, dtype=np.uint8))
    assert e.value.code == BAD_ARG and "term_infinity" in str(e.value)
    with pytest.raises(S.SbnError) as e:
        S.msm_batch_instances_complete(S.FqExpStark(NUM_IO), terms, lengths)
    assert e.value.code == UNSUPPORTED


@pytest.mark.parametrize("curve", CURVES)
def test_every_output_pointer_is_optional(S, curve):
    xs, es, lengths, masks, want = CS.host_cases(curve)["head"]
    terms, lw = CS.words(curve, xs, es, masks), MB.lengths_words(lengths)
    choice = np.full(len(lengths), 9, dtype=np.uint8)
    L = S.lib()
    kind = T.stark_class(S, curve)(NUM_IO).kind
    assert L.sbn_msm_batch_instances_complete(kind, terms.ctypes.data, None, lw.ctypes.data, len(lengths), NUM_IO, None, None, None, None, None, None, None) == 0
    assert L.sbn_msm_batch_instances_complete(kind, terms.ctypes.data, None, lw.ctypes.data, len(lengths), NUM_IO, None, None, None, choice.ctypes.data, None, None, None) == 0
    assert choice.tolist() == want
