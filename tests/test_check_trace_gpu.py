"""The trace check on the device (sbn_prover_check_trace: the quotient stage's constraint kernels on the trace domain, then one
reduction) against the host form on the same matrix and seed -- the report field by field, the flags byte for byte -- and
against what the verifier says about the proof of the same trace."""
import numpy as np
import pytest

import check_trace_cases as K

pytestmark = pytest.mark.gpu
SEED = 0x9E3779B97F4A7C15


def _device(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device")
    S.lib().sbn_set_device(0)


def _same(S, prover, c, trace):
    """check_trace of the loaded trace == check_trace_host of `trace`; returns the report."""
    dev = prover.check_trace(SEED, flags=True)
    host = S.check_trace_host(c["stark"], trace, c["pi"], seed=SEED, flags=True)
    K.consistent(dev)
    assert dev.row_flags.dtype == np.uint8 and np.array_equal(dev.row_flags, host.row_flags)
    assert (dev.rows, dev.failing_rows, dev.first_failing_row, dev.num_zs, dev.z_split) == \
        (host.rows, host.failing_rows, host.first_failing_row, host.num_zs, host.z_split)
    assert dev.segments == host.segments and dev == host
    noflags = prover.check_trace(SEED)
    assert noflags.row_flags is None and noflags.segments == dev.segments and noflags.failing_rows == dev.failing_rows
    return dev


def _accepts(S, stark, proof, cfg):
    try:
        S.verify_stark_proof(stark, proof, cfg)
        return True
    except S.SbnError as e:
        assert e.code == -6, e
        return False


@pytest.mark.parametrize("name", K.SMALL_TABLES)
def test_device_equals_host_and_verifier(S, name):
    """Every 512-row table, the valid trace and every changed cell of the host tests: device report == host report, the trace
    and the proof are untouched by a check, and report.ok exactly when the verifier accepts the proof of that trace."""
    _device(S)
    c = K.case(name)
    stark, cfg = c["stark"], c["stark"].config()
    prover = S.Prover(stark, cfg, 9)
    prover.load_trace(c["trace"], c["pi"])
    before = prover.prove()
    rep = _same(S, prover, c, c["trace"])
    assert rep.ok and not rep.row_flags.any()
    assert np.array_equal(prover.read_trace(), c["trace"])
    after = prover.prove()
    assert np.array_equal(before.words, after.words)
    assert _accepts(S, stark, after, cfg)
    times = prover.check_times()
    assert list(times) == ["perm_z", "constraints", "reduction", "download"] and all(t >= 0 for t in times.values())
    for cell in K.corruptions(name):
        bad = K.corrupt(c["trace"], [cell])
        prover.load_trace(bad, c["pi"])
        rep = _same(S, prover, c, bad)
        assert np.array_equal(prover.read_trace(), bad)
        assert rep.ok == _accepts(S, stark, prover.prove(), cfg), (name, cell, str(rep))
        assert not rep.ok, (name, cell)
    prover.close()


def test_permutation_only_and_two_blocks(S):
    _device(S)
    c = K.case("lookup")
    prover = S.Prover(c["stark"], c["stark"].config(), 9)
    for col, mine, other in ((2, 2, 3), (3, 3, 2)):
        bad = K.corrupt(c["trace"], [(100, col)])
        prover.load_trace(bad, c["pi"])
        rep = _same(S, prover, c, bad)
        assert [int(i) for i in np.nonzero(rep.row_flags & (1 << mine))[0]] == [c["n"] - 1]
        assert not (rep.row_flags & (1 << other)).any()
    prover.close()
    c = K.case("modular")
    prover = S.Prover(c["stark"], c["stark"].config(), 9)
    bad = K.corrupt(c["trace"], [(300, c["cols"][0]), (40, c["cols"][0])])
    prover.load_trace(bad, c["pi"])
    assert _same(S, prover, c, bad).first_failing_row == 40
    prover.close()


def test_chunked_z_path_at_8192_rows(S):
    """ModularStark at 2^13 rows: Z comes from the chunked kernels (permz_chunk_*, n >= 8192), which the 512-row cases do not
    reach, and their chunk products share d_part with the accumulator planes."""
    _device(S)
    c = K.case("modular_8192")
    prover = S.Prover(c["stark"], c["stark"].config(), 13)
    prover.load_trace(c["trace"], c["pi"])
    rep = _same(S, prover, c, c["trace"])
    assert rep.ok
    bad = K.corrupt(c["trace"], [(4097, c["cols"][1])])
    prover.load_trace(bad, c["pi"])
    rep = _same(S, prover, c, bad)
    assert not rep.ok and rep.segments[2]["first_row"] == c["n"] - 1
    prover.close()


def test_g1exp_device_witness(S, O):
    """G1ExpStark(128): the witness generated on the device is clean; read back, one cell changed, loaded again: the device
    names what the host form names."""
    _device(S)
    c = K.case("g1exp")
    stark = c["stark"]
    prover = S.Prover(stark, stark.config(), 16)
    pi = prover.generate_trace(O.g1exp_inputs(128, 1)[0])
    assert np.array_equal(pi, c["pi"])
    rep = prover.check_trace(SEED, flags=True)
    K.consistent(rep)
    assert rep.ok and rep.failing_instances() == []
    trace = prover.read_trace()
    r, col = 512 * 77 + 5, c["cols"][0]
    trace[col, r] = (int(trace[col, r]) + 1) % K.P
    prover.load_trace(trace, pi)
    rep = _same(S, prover, c, trace)
    # the gadget is active on that row; the range check of the changed limb closes on row n - 1, in instance 127
    assert not rep.ok and rep.failing_instances() == [77, 127] and rep.row_flags[r] & 1
    assert str(rep) == "row 39429 (instance 77, row 5 of 512): air_head; 2 rows fail"
    prover.close()


def test_no_trace_loaded(S, O):
    _device(S)
    stark = S.Fq12ExpStark(1)
    prover = S.Prover(stark, stark.config(), 9)
    with pytest.raises(S.SbnError) as e:
        prover.check_trace()
    assert e.value.code == -1 and "no trace loaded" in str(e.value)
    ios = O.fq12exp_inputs(1, 3)[0].copy()
    prover.generate_trace(ios)
    assert prover.check_trace().ok
    ios[0, 0:8] = 0xFFFFFFFF                     # coefficient 0 of x >= p: generate_trace fails and leaves no trace loaded
    with pytest.raises(S.SbnError):
        prover.generate_trace(ios)
    with pytest.raises(S.SbnError) as e:
        prover.check_trace()
    assert e.value.code == -1 and "no trace loaded" in str(e.value)
    prover.close()


def test_split_prover(S, O):
    """World 1: the check runs on the split context (pairs in local order); local world 2: SBN_ERR_UNSUPPORTED on every rank."""
    from starky_bn254_amd import split
    _device(S)
    ios = O.fq12exp_inputs(16, 3)[0]
    stark = S.Fq12ExpStark(16)
    cfg = stark.config()
    for world in (1, 2):
        sb, rb = split.exchange_bytes(stark, cfg, 13, world)
        grp = split.LocalGroup(world, sb, rb)
        provers = [split.SplitProver(stark, cfg, 13, transport=grp.comms[r]) for r in range(world)]
        for p in provers:
            p.generate_trace(ios)
            if world == 1:
                assert p.check_trace(SEED).ok
            else:
                with pytest.raises(S.SbnError) as e:
                    p.check_trace(SEED)
                assert e.value.code == -7
        for p in provers:
            p.close()
        grp.close()
