"""The trace check on the host (sbn_check_trace_host, no device): every row of a trace against the table's constraints on the
trace domain, compared with the oracle's constraint-by-constraint evaluator row by row (tests/check_trace_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import check_trace_cases as K


def _check(S, c, trace, seed=7):
    rep = S.check_trace_host(c["stark"], trace, c["pi"], seed=seed, flags=True)
    K.consistent(rep)
    return rep


@pytest.mark.parametrize("name", K.SMALL_TABLES)
def test_valid_trace_is_clean(S, O, name):
    """The host generator's trace: no row fails, row 0 and the wrap-around row n - 1 (transitions masked, the permutation product
    closes) included; the oracle agrees on every row."""
    c = K.case(name)
    rep = _check(S, c, c["trace"])
    assert rep.ok and rep.failing_rows == 0 and rep.first_failing_row is None and not rep.row_flags.any()
    assert rep.rows == c["n"] and rep.num_zs == c["stark"].num_permutation_zs() and rep.z_split == rep.num_zs // 2
    assert str(rep).startswith("ok")
    assert not any(K.oracle_nonzero(c, c["trace"]).values())


@pytest.mark.parametrize("name", K.SMALL_TABLES)
def test_one_changed_cell_matches_the_oracle_on_every_row(S, O, name):
    """One cell set to (v + 1) mod p at rows 0, 1, 255, 256, n - 1 (and the instance boundary of the Exp tables) x a gadget
    column, a range-check / lookup column and the last column: the AIR segments flag exactly the rows on which the oracle's
    accumulators are non-zero."""
    c = K.case(name)
    for cell in K.corruptions(name):
        bad = K.corrupt(c["trace"], [cell])
        rep = _check(S, c, bad)
        want = K.oracle_nonzero(c, bad)
        got = (rep.row_flags & 3) != 0
        assert [i for i in range(c["n"]) if want[i]] == [int(i) for i in np.nonzero(got)[0]], (name, cell)
        assert not rep.ok, (name, cell)
        if rep.first_failing_row is not None and c["stark"].kind in (S.AIR_FQ12_EXP, S.AIR_FQ12_EXP_U64):
            r = rep.first_failing_row
            assert f"row {r} (instance {r // rep.rows_per_instance}, row {r % rep.rows_per_instance} of {rep.rows_per_instance})" in str(rep)
            assert rep.failing_instances() == sorted({int(i) // rep.rows_per_instance for i in np.nonzero(rep.row_flags)[0]})


def test_g1exp_at_65536_rows(S, O):
    """G1ExpStark(128), 2^16 rows: the valid trace is clean; one changed cell is flagged where the oracle says (rows r - 1, r,
    r + 1, 0, n - 1 and every 97th row)."""
    c = K.case("g1exp")
    n = c["n"]
    rep = _check(S, c, c["trace"])
    assert rep.ok and not rep.row_flags.any()
    for r, col in ((512, c["cols"][0]), (511, c["cols"][1]), (n - 1, c["cols"][2]), (512 * 77 + 5, c["cols"][0])):
        bad = K.corrupt(c["trace"], [(r, col)])
        rep = _check(S, c, bad)
        rows = sorted({(r - 1) % n, r, (r + 1) % n, 0, n - 1} | set(range(0, n, 97)))
        want = K.oracle_nonzero(c, bad, rows)
        got = (rep.row_flags & 3) != 0
        assert [i for i in rows if want[i]] == [i for i in rows if got[i]], (r, col)
        assert not rep.ok            # (a changed table cell may pass every AIR constraint: the permutation check has it then)
        if r == 512 * 77 + 5:        # a row on which the gadget is active; the range check of the changed limb closes on row n - 1
            assert rep.failing_instances() == [77, 127] and "row 39429 (instance 77, row 5 of 512): air_head; 2 rows fail" == str(rep)
        del bad


@pytest.mark.parametrize("col", [2, 3])
def test_permutation_only(S, col):
    """MyStark, one cell of a permuted column changed: Z is the running product, so only the closing row n - 1 of that column's
    permutation check can break; the other half of the Z columns stays clean."""
    c = K.case("lookup")
    n = c["n"]
    bad = K.corrupt(c["trace"], [(100, col)])
    rep = _check(S, c, bad)
    mine, other = (2, 3) if col == 2 else (3, 2)
    assert [int(i) for i in np.nonzero(rep.row_flags & (1 << mine))[0]] == [n - 1]
    assert not (rep.row_flags & (1 << other)).any()
    assert rep.segments[mine]["failing_rows"] == 1 and rep.segments[mine]["first_row"] == n - 1
    assert rep.segments[other]["failing_rows"] == 0 and rep.segments[other]["first_row"] is None
    assert (rep.num_zs, rep.z_split) == (2, 1)


def test_two_rows_in_different_blocks(S):
    c = K.case("modular")
    rep = _check(S, c, K.corrupt(c["trace"], [(300, c["cols"][0]), (40, c["cols"][0])]))
    assert rep.first_failing_row == 40 and rep.failing_rows >= 2
    assert rep.row_flags[40] & 1 and rep.row_flags[300] & 1
    assert "row 40: air_head" in str(rep)


def test_seeds(S):
    """Two seeds give the same flags on these inputs (the challenges only weigh the constraints); one seed twice: the same report."""
    for name in ("g1op", "fq12exp_u64"):
        c = K.case(name)
        bad = K.corrupt(c["trace"], [(1, c["cols"][0]), (256, c["cols"][1])])
        a, b, a2 = _check(S, c, bad, seed=1), _check(S, c, bad, seed=(1 << 64) - 1), _check(S, c, bad, seed=1)
        assert np.array_equal(a.row_flags, b.row_flags)
        assert a == a2 and a == b
        assert S.check_trace_host(c["stark"], bad, c["pi"], seed=1).row_flags is None


def test_argument_errors(S):
    L = S.lib()
    c = K.case("lookup")
    tr, raw = np.array(c["trace"]), S.api._TraceReport(struct_size=C.sizeof(S.api._TraceReport))
    air = c["stark"]._d
    call = lambda air, tr, bits, rep: L.sbn_check_trace_host(C.byref(air) if air else None, S.api._ptr(tr), bits, None, 0, 0, C.byref(rep) if rep else None, None)  # noqa: E731
    assert call(air, tr, 9, raw) == 0
    assert call(air, tr, 9, None) == -1                       # null report
    assert call(None, tr, 9, raw) == -1 and call(air, None, 9, raw) == -1
    short = S.api._TraceReport(struct_size=C.sizeof(S.api._TraceReport) - 8)
    assert call(air, tr, 9, short) == -1 and b"struct_size" in L.sbn_last_error()
    assert call(S.api._AirDesc(99, 0), tr, 9, raw) == -1      # unknown kind
    assert call(air, tr, 8, raw) == -7                        # as sbn_prover_create: degree_bits out of range
    assert call(S.api._AirDesc(S.AIR_FLAGS, 2), tr, 9, raw) == -1   # FlagStark(2) has 1024 rows
    pi1 = np.zeros(1, dtype=np.uint64)
    assert L.sbn_check_trace_host(C.byref(air), S.api._ptr(tr), 9, S.api._ptr(pi1), 1, 0, C.byref(raw), None) == -1
    tr[1, 17] = K.P                                           # word 1 * 512 + 17
    tr[3, 5] = K.P + 1
    assert call(air, tr, 9, raw) == -2 and b"trace word 529 " in L.sbn_last_error()
    with pytest.raises(S.SbnError) as e:
        S.check_trace_host(c["stark"], tr, c["pi"])
    assert e.value.code == -2
    with pytest.raises(S.SbnError):
        S.check_trace_host(c["stark"], tr[:3], c["pi"])
    # the device form refuses a null prover before it looks for a device
    assert L.sbn_prover_check_trace(None, 0, C.byref(raw), None) == -1
    assert L.sbn_split_prover_check_trace(None, 0, C.byref(raw), None) == -1
    assert L.sbn_prover_check_times(None, None, 0) == 0


def test_segment_names(S):
    L = S.lib()
    names = [L.sbn_trace_segment_name(s).decode() for s in range(4)]
    assert all(names) and len(set(names)) == 4
    assert L.sbn_trace_segment_name(4) == b"" and L.sbn_trace_segment_name(-1) == b""
