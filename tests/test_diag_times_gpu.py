"""The five *_times getters of a prover (sbn_prover_stage_times, sbn_prover_check_times, sbn_prover_explain_times,
sbn_prover_explain_permutation_times, sbn_prover_diff_witness_times) share one copy routine, and the four diagnostics one table of
times in the context (csrc/prover_ctx.hpp copy_times, sbn_prover.diag_ms).  What that sharing could break silently: the count a
getter returns for a given cap, how many floats it writes, and one feature's call overwriting another feature's times.

Fq12ExpStark(1) at 2^9 rows, the smallest height the prover accepts, goes through prove() and all four diagnostics;
G1ExpStark(128) at 2^16 rows through the witness diff of a u16-range-check table (its device witness starts at that height)."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

# getter -> the number of times it holds (include/sbn.h; the stage getter: ST_COUNT + EX_COUNT of csrc/prover_ctx.hpp)
GETTERS = {"sbn_prover_stage_times": 16, "sbn_prover_check_times": 4, "sbn_prover_explain_times": 3,
           "sbn_prover_explain_permutation_times": 3, "sbn_prover_diff_witness_times": 3}
SENTINEL = -12345.0   # no time is negative
PAD = 8


def _get(S, prover, getter, cap):
    """(returned count, the whole buffer) of one call with a buffer of count + PAD sentinels."""
    buf = (C.c_float * (GETTERS[getter] + PAD))(*([SENTINEL] * (GETTERS[getter] + PAD)))
    k = getattr(S.lib(), getter)(prover._h, buf, cap)
    return k, list(buf)


def _all(S, prover):
    out = {}
    for getter, count in GETTERS.items():
        k, buf = _get(S, prover, getter, count)
        assert k == count and SENTINEL not in buf[:count] and buf[count:] == [SENTINEL] * PAD, (getter, k, buf)
        out[getter] = buf[:count]
    return out


def _exercise(S, prover, steps):
    """steps: [(getter, call)].  Zeros before the first call; each call moves its own times only; every cap copies min(cap, count)."""
    before = _all(S, prover)
    assert all(v == [0.0] * GETTERS[g] for g, v in before.items()), before
    for getter, call in steps:
        call()
        after = _all(S, prover)
        for other in GETTERS:
            if other != getter:
                assert after[other] == before[other], (getter, other, before[other], after[other])
        count, own = GETTERS[getter], after[getter]
        assert all(t >= 0 for t in own) and sum(own) > 0, (getter, own)
        for cap in (0, 1, count, count + 3):
            k, buf = _get(S, prover, getter, cap)
            want = min(cap, count)
            assert k == want and buf[:want] == own[:want] and buf[want:] == [SENTINEL] * (count + PAD - want), (getter, cap, k, buf)
        before = after


@pytest.fixture()
def device(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device")
    S.lib().sbn_set_device(0)


def test_every_getter_on_the_smallest_table(S, O, device):
    stark = S.Fq12ExpStark(1)
    ios, _ = O.fq12exp_inputs(1, 7)
    trace, pi = stark.generate_trace_and_public_inputs(ios)
    prover = S.Prover(stark, stark.config(), 9)
    assert all(v == [0.0] * GETTERS[g] for g, v in _all(S, prover).items())   # also before a trace is loaded
    prover.load_trace(trace, pi)
    _exercise(S, prover, [("sbn_prover_stage_times", prover.prove), ("sbn_prover_check_times", prover.check_trace),
                          ("sbn_prover_explain_times", prover.explain_trace), ("sbn_prover_explain_permutation_times", prover.explain_permutations),
                          ("sbn_prover_diff_witness_times", prover.diff_witness)])
    assert prover.check_trace().ok and prover.diff_witness().ok
    prover.close()


def test_witness_diff_getter_on_a_u16_range_check_table(S, device, g1exp_case):
    stark = S.G1ExpStark(128)
    prover = S.Prover(stark, stark.config(), 16)
    prover.load_trace(g1exp_case["trace"], g1exp_case["pi"])
    _exercise(S, prover, [("sbn_prover_diff_witness_times", prover.diff_witness)])
    prover.close()
