"""GPU test of the chain walks (run with `-m gpu` on the MI355X box).  The kernels of the explicit list, of the tower and chained
calls and of the programs walk a chain by the same step, spelled out in each kernel, and share one verdict and one un-offset; a
copy that drifts, or a shared piece that breaks, shows here.  The three routes are held against each other on one prover: the trace of one list generated as the explicit
list, as the tower or segmented chained call that spells it and as the program that spells it must agree word for word in
read_trace() and in the public inputs.  Fq12ExpU64Stark(16) and G1ExpStark(128) in the placements 1 (one lane per instance) and 2
(one wave per instance) of the curve chains.  Every list has count = num_io - 1 instances, so one pad row exists, an exponent with
bit 0 clear and its top bit (63 / 255) set, and an exponent of zero.  The curves have no tower call: there the chained call and the
program are compared with the explicit list.  The placements are those of the CURVE chains; the Fq12 chains have one device form,
so the Fq12 prover is created without a switch."""
import numpy as np
import pytest

import chained_lists as CL
import curve_programs as CP
import oracle_lib as O
import power_lists as PL
import program_lists as G
import tracegen_edges as T

pytestmark = pytest.mark.gpu
TOP_U64, TOP_256 = (1 << 63) | 2, (1 << 255) | 2                           # bit 0 clear, the top bit set


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


def _segments_as_program(lengths):
    """The nodes of a segmented chained list: x = literal S + g, exponent g; the head of segment s starts from literal s (its
    start), every other instance from the output before it."""
    nodes, g = [], 0
    for s, n in enumerate(lengths):
        for j in range(n):
            nodes.append((len(lengths) + g, s if j == 0 else G.out(g - 1), g))
            g += 1
    return nodes


def _agree(pr, want, got_pi, what):
    """The loaded trace and the public inputs against those of the explicit list."""
    pi_want, trace_want = want
    assert np.array_equal(got_pi, pi_want), what
    bad = np.nonzero((pr.read_trace() != trace_want).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:8].tolist())


def _explicit(pr, ios):
    return pr.generate_trace(ios), pr.read_trace()


def test_fq12_u64_towers_chains_and_programs_walk_alike(gpu):
    """Fq12ExpU64Stark(16), 2^11 rows.  Five towers of depth 3 and two chained segments of 8 and 7, fifteen instances each."""
    stark = gpu.Fq12ExpU64Stark(16)
    r = PL.rng(21)
    bases = [PL.random_elem("fq12", r) for _ in range(5)]
    tower_exps = [TOP_U64, 0] + [r.randrange(PL.GLP) for _ in range(2)] + [TOP_U64 + 4]   # the last tower ends in the row the pad copies
    tower_prog = G.arrays("fq12u64", G.towers_as_program(5, 3, False), bases, tower_exps)
    lengths = [8, 7]
    starts = [PL.random_elem("fq12", r) for _ in lengths]
    xs = [PL.random_elem("fq12", r) for _ in range(15)]
    chain_exps = [r.randrange(PL.GLP) for _ in range(15)]
    chain_exps[0], chain_exps[3], chain_exps[14] = 0, TOP_U64, TOP_U64        # a head, the middle of a segment, the row the pad copies
    chain_prog = G.arrays("fq12u64", _segments_as_program(lengths), starts + xs, chain_exps)
    tower_ios = gpu.program_instances(stark, *tower_prog)[0]
    chain_ios = gpu.program_instances(stark, *chain_prog)[0]
    assert tower_ios.shape == chain_ios.shape == (1, 16, 194)
    assert np.array_equal(tower_ios[0, 15], tower_ios[0, 14]) and np.array_equal(chain_ios[0, 15], chain_ios[0, 14])   # the pad row
    with T.placement(gpu, stark, stark.config(), 11, {}) as pr:
        want = _explicit(pr, tower_ios[0])
        pi, _, ios = pr.generate_trace_powers(PL.base_words("fq12u64", bases), PL.exp_words("fq12u64", tower_exps), 3)
        assert np.array_equal(ios, tower_ios[0])
        _agree(pr, want, pi, "towers")
        _agree(pr, want, pr.generate_trace_program(*tower_prog)[0], "towers as a program")
        want = _explicit(pr, chain_ios[0])
        pi, _, _, _, ios = pr.generate_trace_msms(CL.terms_words("fq12u64", xs, chain_exps), lengths, np.array([CL.value_words("fq12u64", s) for s in starts]))
        assert np.array_equal(ios, chain_ios[0])
        _agree(pr, want, pi, "chained segments")
        _agree(pr, want, pr.generate_trace_program(*chain_prog)[0], "chained segments as a program")


@pytest.mark.parametrize("mode", ["1", "2"])
def test_g1_chains_and_programs_walk_alike(gpu, mode):
    """G1ExpStark(128), 2^16 rows: sixteen chained segments, 127 instances, eight levels as a program."""
    stark = gpu.G1ExpStark(128)
    rng = np.random.default_rng(22)
    lengths = [8] * 15 + [7]
    starts = [O.g1_random(rng) for _ in lengths]
    xs = [O.g1_random(rng) for _ in range(127)]
    exps = [int.from_bytes(rng.bytes(32), "little") % T.R for _ in range(127)]
    exps[0], exps[8], exps[13], exps[125], exps[126] = TOP_256, 0, TOP_256, 0, TOP_256   # heads, inside a segment, the row the pad copies
    prog = CP.arrays("g1", _segments_as_program(lengths), starts + xs, exps)
    ios_want, _, _, infinity, choice = gpu.curve_program_instances(stark, *prog)
    assert ios_want.shape == (1, 128, 40) and choice == 0 and not infinity.any()
    assert np.array_equal(ios_want[0, 127], ios_want[0, 126])                  # the pad row
    with T.placement(gpu, stark, stark.config(), 16, {"SBN_TRACEGEN_DEVICE_CHAIN": mode}) as pr:
        want = _explicit(pr, ios_want[0])
        got = pr.generate_trace_msms(CL.terms_words("g1", xs, exps), lengths, np.array([CL.value_words("g1", s) for s in starts]))
        assert np.array_equal(got[4], ios_want[0])
        _agree(pr, want, got[0], "chained segments")
        got = pr.generate_trace_curve_program(*prog)
        assert got[4] == 0 and np.array_equal(got[5], ios_want[0])
        _agree(pr, want, got[0], "chained segments as a program")
