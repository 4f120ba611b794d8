"""GPU test of the stage lines device witness generation prints under SBN_TRACE_TIMING (run with `-m gpu` on the MI355X box): for
every list source of the curve tables (explicit, chained, scalar multiplications, segmented), of the Fq12 tables (explicit, chained,
segmented, power towers) and for FqExpStark, one call prints exactly the expected stage names, in order, then `total`, each line in
the format "[device tracegen] %-14s %8.3f ms" with a finite time >= 0.  Smallest device sizes, one prover per case; the lists are
those of the other GPU tests (chained_lists, scalar_mul_lists, msm_batches, power_lists, tracegen_edges)."""
import math
import re

import pytest

import chained_lists as CL
import msm_batches as MB
import power_lists as PL
import scalar_mul_lists as SL
import tracegen_edges as T

pytestmark = pytest.mark.gpu
TIMING = {"SBN_TRACE_TIMING": "1"}
CHAIN2 = dict(TIMING, SBN_TRACEGEN_DEVICE_CHAIN="2")
CHAIN0 = dict(TIMING, SBN_TRACEGEN_DEVICE_CHAIN="0")
LINE = re.compile(r"\[device tracegen\] (\S+) +(\S+) ms")

CURVE_EXPLICIT = ["flags+pulses", "chains", "affine+lambda", "row_witness", "range_check"]
FIELD_EXPLICIT = ["flags+pulses", "chains", "row_witness", "range_check"]
FQ12_OFFSETS = ["flags+pulses", "chains", "chain_offsets", "row_witness", "range_check"]


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


def _explicit(table):
    return lambda gpu, pr: pr.generate_trace(T.edge_list(table)[0])


def _chained(table):
    def call(gpu, pr):
        terms, start, _, _ = CL.chained_list(table, T.SHAPE[table][0])
        pr.generate_trace_chained(terms, start)
    return call


def _scalar_muls(gpu, pr):
    points, scalars, off, _, _, _, _ = SL.case("g1")
    pr.generate_trace_scalar_muls(points[:SL.NUM_IO], scalars[:SL.NUM_IO], off)


def _curve_msms(gpu, pr):
    xs, es, starts, _, _, _ = MB.curve_unit("g1", False)
    pr.generate_trace_msms(CL.terms_words("g1", xs, es), MB.lengths_words(MB.CURVE_LENGTHS), MB.starts_words("g1", starts))


def _field_msms(gpu, pr):
    xs, es, starts, _, _ = MB.field_unit("fq12u64", 16, False)
    pr.generate_trace_msms(CL.terms_words("fq12u64", xs, es), MB.lengths_words(MB.field_lengths(16)), MB.starts_words("fq12u64", starts))


def _towers(gpu, pr):
    """5 towers of depth 3 with the shared BN parameter: 15 instances and one pad."""
    r = PL.rng(1)
    pr.generate_trace_powers(PL.base_words("fq12", [PL.random_elem("fq12", r) for _ in range(5)]), gpu.BN_X, 3)


# (id, table, instances, switches, call, stage names)
CASES = [
    ("g1-explicit", "g1", 128, CHAIN2, _explicit("g1"), CURVE_EXPLICIT),
    ("g1-chained", "g1", 128, CHAIN2, _chained("g1"), ["chain_offsets"] + CURVE_EXPLICIT),
    ("g1-scalar_muls", "g1", 128, CHAIN2, _scalar_muls,
     ["scalar_list", "flags+pulses", "chains", "affine+lambda", "un_offset", "row_witness", "range_check"]),
    ("g1-msms", "g1", 128, CHAIN2, _curve_msms,
     ["chain_offsets", "flags+pulses", "chains", "affine+lambda", "un_offset", "row_witness", "range_check"]),
    ("g1-chained-host_pool", "g1", 128, CHAIN0, _chained("g1"), CURVE_EXPLICIT),        # the explicit-list fallback
    ("fq12u64-explicit", "fq12u64", 16, TIMING, _explicit("fq12u64"), FIELD_EXPLICIT),
    ("fq12u64-chained", "fq12u64", 16, TIMING, _chained("fq12u64"), FQ12_OFFSETS),
    ("fq12u64-msms", "fq12u64", 16, TIMING, _field_msms, FQ12_OFFSETS),
    ("fq12u64-powers", "fq12u64", 16, TIMING, _towers, ["flags+pulses", "tower_links", "tower_pads", "row_witness", "range_check"]),
    ("fq-explicit", "fq", 128, TIMING, _explicit("fq"), FIELD_EXPLICIT),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_one_call_prints_its_stages_in_order(gpu, capfd, case):
    _, table, num_io, env, call, stages = case
    stark = T.stark_class(gpu, table)(num_io)
    with T.placement(gpu, stark, stark.config(), T.degree_bits(table, num_io), env) as pr:
        capfd.readouterr()
        call(gpu, pr)
        err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if ln.startswith("[device tracegen]")]
    print("\n".join(lines))
    parsed = [LINE.fullmatch(ln) for ln in lines]
    assert all(parsed), lines
    assert [m.group(1) for m in parsed] == stages + ["total"]
    for ln, m in zip(lines, parsed):
        ms = float(m.group(2))
        assert math.isfinite(ms) and ms >= 0, ln
        assert ln == "[device tracegen] %-14s %8.3f ms" % (m.group(1), ms), ln
