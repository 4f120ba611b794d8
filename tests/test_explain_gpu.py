"""Explain on the device (sbn_prover_explain_rows / sbn_prover_explain_trace: one thread per row through the recording consumer,
wave ballots and one atomic per failing block) against the host forms on the same matrix and seed, bit for bit."""
import numpy as np
import pytest

import check_trace_cases as K
import explain_cases as E

pytestmark = pytest.mark.gpu
SEED = E.SEED


def _device(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device")
    S.lib().sbn_set_device(0)


def _same(S, prover, c, trace, rows):
    """explain_rows and explain_trace of the loaded trace == the host forms of `trace`; returns the device results."""
    dev_rows = prover.explain_rows(rows, SEED)
    host_rows = S.explain_rows_host(c["stark"], trace, c["pi"], rows, seed=SEED)
    assert dev_rows.block_flags.dtype == np.uint8 and np.array_equal(dev_rows.block_flags, host_rows.block_flags)
    assert np.array_equal(dev_rows.z_flags, host_rows.z_flags) and dev_rows == host_rows and str(dev_rows) == str(host_rows)
    dev, host = prover.explain_trace(SEED), S.explain_trace_host(c["stark"], trace, c["pi"], seed=SEED)
    for f in ("block_failing_rows", "block_first_row", "z_failing_rows", "z_first_row"):
        assert np.array_equal(getattr(dev, f), getattr(host, f)), f
    assert dev == host and str(dev) == str(host)
    return dev_rows, dev


@pytest.mark.parametrize("name", K.SMALL_TABLES)
def test_device_equals_host(S, name):
    """Every 512-row table, rows 0, 1, 255 | 256 (the workgroup boundary), n - 1, the instance boundary and their predecessors:
    the valid trace and every corrupted one of the host tests."""
    _device(S)
    c = K.case(name)
    rows = E.gpu_rows(name)
    prover = S.Prover(c["stark"], c["stark"].config(), 9)
    prover.load_trace(c["trace"], c["pi"])
    dev_rows, dev = _same(S, prover, c, c["trace"], rows)
    assert dev.ok and all(r.ok for r in dev_rows)
    times = prover.explain_times()
    assert list(times) == ["perm_z", "explain", "download"] and all(t >= 0 for t in times.values())
    for cells, bad, _ in E.corrupted(name):
        prover.load_trace(bad, c["pi"])
        dev_rows, dev = _same(S, prover, c, bad, rows)
        assert not dev.ok, (name, cells)
        assert np.array_equal(prover.read_trace(), bad)
    # a list longer than a workgroup, unordered and with repeats; an empty list
    many = np.array([(7 * k) % c["n"] for k in range(300)] + [5, 5], dtype=np.uint64)
    got = prover.explain_rows(many, SEED)
    assert got == S.explain_rows_host(c["stark"], bad, c["pi"], many, seed=SEED)
    assert len(prover.explain_rows([], SEED)) == 0
    with pytest.raises(S.SbnError) as e:
        prover.explain_rows([c["n"]], SEED)
    assert e.value.code == -1
    prover.close()


def _every_row_fails(S, name, bits, columns):
    c = K.case(name)
    bad = np.array(c["trace"])
    for col in columns:
        bad[col] = (bad[col] + np.uint64(1)) % np.uint64(K.P)     # (v + 1 < 2^64: the words are canonical)
    prover = S.Prover(c["stark"], c["stark"].config(), bits)
    prover.load_trace(bad, c["pi"])
    dev, host = prover.explain_trace(SEED), S.explain_trace_host(c["stark"], bad, c["pi"], seed=SEED)
    prover.close()
    assert dev == host
    assert int(dev.block_failing_rows.max()) == c["n"]            # some block fails on every row: every wave adds into its counter
    assert int(dev.block_first_row[int(dev.block_failing_rows.argmax())]) == 0
    return dev


def test_atomics_every_row_fails(S):
    """ModularStark, 512 rows, one whole column incremented: every row fails, and the device counts equal the host's exactly;
    then two columns of different sections (a gadget output limb and a range-check lookup column)."""
    _device(S)
    gadget_col, rc_col, _ = K.case("modular")["cols"]
    one = _every_row_fails(S, "modular", 9, [gadget_col])
    assert {b.name for b, _, _ in one.failing_blocks()} >= {"gadget_mul", "range_check_recomposition"}
    two = _every_row_fails(S, "modular", 9, [gadget_col, rc_col])
    assert {b.name for b, _, _ in two.failing_blocks()} >= {"gadget_mul", "range_check_lookup"}
    assert two.failing_zs() and all(first == 511 for _, _, first in two.failing_zs())


def test_atomics_many_workgroups_8192_rows(S):
    """ModularStark at 2^13 rows: 32 workgroups add into one counter, and Z comes from the chunked kernels."""
    _device(S)
    gadget_col, rc_col, _ = K.case("modular_8192")["cols"]
    dev = _every_row_fails(S, "modular_8192", 13, [gadget_col, rc_col])
    assert "fails on 8,192 rows, first on row 0" in str(dev)


def test_g1exp_headline(S):
    """G1ExpStark(128), 65,536 rows, three changed cells -- a gadget limb, the sorted copy of range-check target 0, the last column
    -- on rows of different instances: explain_trace names no row the check does not name, and the blocks it flags on the
    check's rows are those explain_rows_host flags there."""
    _device(S)
    c = K.case("g1exp")
    stark, n = c["stark"], c["n"]
    cells = [(512 * 77 + 5, c["cols"][0]), (512 * 3 + 100, c["cols"][1]), (512 * 120 + 17, c["cols"][2])]
    bad = K.corrupt(c["trace"], cells)
    prover = S.Prover(stark, stark.config(), 16)
    prover.load_trace(bad, c["pi"])
    rep = prover.check_trace(SEED, flags=True)
    failing = [int(i) for i in np.nonzero(rep.row_flags)[0]]
    assert 1 <= len(failing) <= 16
    dev = prover.explain_trace(SEED)
    assert not dev.ok
    named = {r for _, k, r in dev.failing_blocks()} | {r for _, k, r in dev.failing_zs()}
    assert named <= set(failing)
    assert int(dev.block_failing_rows.max()) <= len(failing) and int(dev.z_failing_rows.max(initial=0)) <= len(failing)
    dev_rows = prover.explain_rows(failing, SEED)
    host_rows = S.explain_rows_host(stark, bad, c["pi"], failing, seed=SEED)
    assert dev_rows == host_rows
    bits = np.unpackbits(dev_rows.block_flags, axis=1, bitorder="little")[:, :len(stark.constraint_blocks())]
    zbits = np.unpackbits(dev_rows.z_flags, axis=1, bitorder="little")[:, :stark.num_permutation_zs()]
    # every failing row of a block is one of the check's rows, so the whole-trace statistics are the sums over those rows
    assert np.array_equal(bits.sum(axis=0).astype(np.uint64), dev.block_failing_rows)
    assert np.array_equal(zbits.sum(axis=0).astype(np.uint64), dev.z_failing_rows)
    first = np.where(bits.any(axis=0), np.array(failing, dtype=np.uint64)[bits.argmax(axis=0)], np.uint64((1 << 64) - 1))
    assert np.array_equal(first, dev.block_first_row)
    text = str(dev_rows[failing.index(512 * 77 + 5)])
    assert text.startswith("row 39429 (instance 77, row 5 of 512): ") and "gadget_" in text and "cols 64..384" in text
    prover.close()


def test_no_side_effects(S, O):
    """prove() gives the same words before and after an explain; no trace loaded, and after a failed generate_trace: BAD_ARG."""
    _device(S)
    stark = S.Fq12ExpStark(1)
    prover = S.Prover(stark, stark.config(), 9)
    for call in (lambda: prover.explain_trace(SEED), lambda: prover.explain_rows([0], SEED)):
        with pytest.raises(S.SbnError) as e:
            call()
        assert e.value.code == -1 and "no trace loaded" in str(e.value)
    ios = O.fq12exp_inputs(1, 3)[0].copy()
    prover.generate_trace(ios)
    before = prover.prove()
    assert prover.explain_trace(SEED).ok and all(r.ok for r in prover.explain_rows([0, 255, 511], SEED))
    after = prover.prove()
    assert np.array_equal(before.words, after.words)
    assert prover.check_trace(SEED).ok
    ios[0, 0:8] = 0xFFFFFFFF                     # coefficient 0 of x >= p: generate_trace fails and leaves no trace loaded
    with pytest.raises(S.SbnError):
        prover.generate_trace(ios)
    for call in (lambda: prover.explain_trace(SEED), lambda: prover.explain_rows([0], SEED)):
        with pytest.raises(S.SbnError) as e:
            call()
        assert e.value.code == -1 and "no trace loaded" in str(e.value)
    prover.close()


def test_split_prover(S, O):
    """A split prover of one rank answers as the single-GPU prover does (pairs in local order); two local ranks:
    SBN_ERR_UNSUPPORTED on each."""
    from starky_bn254_amd import split
    _device(S)
    c = K.case("fq12exp")
    stark, cfg = c["stark"], c["stark"].config()
    cells, bad, rows = E.corrupted("fq12exp")[0]
    single = S.Prover(stark, cfg, 9)
    single.load_trace(bad, c["pi"])
    want_rows, want = single.explain_rows(rows, SEED), single.explain_trace(SEED)
    single.close()
    assert not want.ok
    sb, rb = split.exchange_bytes(stark, cfg, 9, 1)
    grp = split.LocalGroup(1, sb, rb)
    p = split.SplitProver(stark, cfg, 9, transport=grp.comms[0])
    p.load_trace(bad, c["pi"])
    assert p.explain_rows(rows, SEED) == want_rows and p.explain_trace(SEED) == want
    p.close()
    grp.close()
    stark = S.Fq12ExpStark(16)
    cfg, ios = stark.config(), O.fq12exp_inputs(16, 3)[0]
    sb, rb = split.exchange_bytes(stark, cfg, 13, 2)
    grp = split.LocalGroup(2, sb, rb)
    provers = [split.SplitProver(stark, cfg, 13, transport=grp.comms[r]) for r in range(2)]
    for p in provers:
        p.generate_trace(ios)
        for call in (lambda: p.explain_trace(SEED), lambda: p.explain_rows([0], SEED)):
            with pytest.raises(S.SbnError) as e:
                call()
            assert e.value.code == -7
    for p in provers:
        p.close()
    grp.close()
