"""Explain on the host (sbn_air_constraint_blocks, sbn_explain_rows_host, sbn_explain_trace_host; no device): the block table of
every table, the flagged blocks against the oracle's per-constraint values (tests/explain_cases.py: exact, by an inverse NTT
over the oracle's accumulators), against the trace check, and the names against the column layout."""
import ctypes as C

import numpy as np
import pytest

import check_trace_cases as K
import explain_cases as E

NO_ROW = (1 << 64) - 1


def _smallest(S):
    return [S.G1Stark(), S.G1ExpStark(128), S.G2ExpStark(128), S.Fq12ExpStark(1), S.FqExpStark(128), S.Fq12ExpU64Stark(4),
            S.ModularStark(), S.Fq12Stark(), S.MyStark(), S.FlagStark(1), S.FlagU64Stark(4)]


def test_block_table_of_every_kind(S):
    """All eleven kinds at their smallest size: the blocks are contiguous from 0 and sum to sbn_air_num_constraints; the segment
    never decreases and segment 1 holds the tail count the check's segments use; names and column spans are sane."""
    L = S.lib()
    kinds = set()
    for stark in _smallest(S):
        kinds.add(stark.kind)
        blocks = stark.constraint_blocks()
        assert blocks and [b.index for b in blocks] == list(range(len(blocks)))
        first = 0
        for b in blocks:
            assert b.first == first and b.count >= 1, (stark.kind, b)
            first += b.count
            assert b.name and b.name == L.sbn_constraint_section_name(b.section).decode()
            assert b.col_first + b.col_count <= stark.num_columns and b.segment in (0, 1)
        assert first == stark.num_constraints
        segs = [b.segment for b in blocks]
        assert segs == sorted(segs)
        tail = sum(b.count for b in blocks if b.segment == 1)
        if stark.kind in (S.AIR_G1_EXP, S.AIR_G2_EXP, S.AIR_FQ12_EXP, S.AIR_FQ_EXP, S.AIR_FQ12_EXP_U64):
            rc = {S.AIR_G1_EXP: 2 * 381, S.AIR_G2_EXP: 2 * 762, S.AIR_FQ_EXP: 2 * 143}.get(stark.kind, 5 * 1332)
            assert tail == 2 + 4 * stark.num_io + rc + 3     # io pulses + range check (csrc/air.cuh num_tail_constraints)
        else:
            assert tail == 0
        # a short buffer gets the first entries, and the count all the same
        raw = (S.api._ConstraintBlock * 1)()
        assert L.sbn_air_constraint_blocks(C.byref(stark._d), raw, 1) == len(blocks) and (raw[0].first, raw[0].count) == (0, blocks[0].count)
    assert len(kinds) == 11
    assert S.G1ExpStark(128).num_constraints == 9027
    assert L.sbn_air_constraint_blocks(C.byref(S.api._AirDesc(99, 0)), None, 0) == 0
    assert L.sbn_constraint_section_name(-1) == b"" and L.sbn_constraint_section_name(1000) == b""
    names = {L.sbn_constraint_section_name(s).decode() for s in range(17)}
    assert len(names) == 17 and {"transition_double", "transition_add", "transition_hold", "gadget_add", "gadget_double", "gadget_sq", "gadget_mul",
                                 "flags", "flags_repeat", "rotation_pulse", "io_pulse", "range_check_recomposition", "range_check_lookup",
                                 "range_table"} <= names


def test_exp_sections_in_emission_order(S):
    """G1ExpStark(128) and Fq12ExpStark(1): sections [1] to [10] of exp_eval, the head / tail boundary a block boundary."""
    for stark, gadgets in ((S.G1ExpStark(128), ["gadget_add", "gadget_double"]), (S.Fq12ExpStark(1), ["gadget_sq", "gadget_mul"])):
        blocks = stark.constraint_blocks()
        head = [b.name for b in blocks if b.segment == 0]
        assert head == ["output_pulse_sum", "public_inputs", "transition_double", "transition_add", "transition_hold", "flags"] + gadgets + \
            ["flags_repeat"] + ["rotation_pulse"] * 5
        assert blocks[1].count == stark.num_public_inputs
        tail = [b for b in blocks if b.segment == 1]
        assert [b.name for b in tail[:2 + 4 * stark.num_io]] == ["io_pulse"] * (2 + 4 * stark.num_io)
        assert [b.instance for b in tail[:6]] == [None, None, 0, 0, 1, 1]
        assert [b.name for b in tail[-3:]] == ["range_table"] * 3 and all(b.count == 1 for b in tail)
    assert "gadget_add [7387, 7552) cols 64..384" == str(S.G1ExpStark(128).constraint_blocks()[6])


@pytest.mark.parametrize("name", K.SMALL_TABLES)
def test_valid_trace_flags_nothing(S, name):
    c = K.case(name)
    e = S.explain_trace_host(c["stark"], c["trace"], c["pi"], seed=E.SEED)
    assert e.ok and not e.block_failing_rows.any() and not e.z_failing_rows.any()
    assert (e.block_first_row == NO_ROW).all() and (e.z_first_row == NO_ROW).all()
    assert len(e.block_first_row) == len(c["stark"].constraint_blocks()) and len(e.z_first_row) == c["stark"].num_permutation_zs()
    assert str(e).startswith("ok")
    r = S.explain_rows_host(c["stark"], c["trace"], c["pi"], c["rows"], seed=E.SEED)
    assert not r.block_flags.any() and not r.z_flags.any() and all(x.ok for x in r)


@pytest.mark.parametrize("name", K.SMALL_TABLES)
def test_flagged_blocks_equal_the_oracle_per_constraint(S, O, name):
    """Every changed cell of check_trace_cases, rows r - 1 and r: the set of blocks explain_rows_host flags == the set of blocks
    that contain a constraint the oracle finds non-zero.  The issue's G1Stark figures: cell (column 80, row 5) breaks 34
    constraints."""
    c = K.case(name)
    for cells, bad, rows in E.corrupted(name):
        got = S.explain_rows_host(c["stark"], bad, c["pi"], rows, seed=E.SEED)
        seen = set()
        for k, i in enumerate(rows):
            want = E.oracle_blocks(c, bad, i)
            assert E.flagged(got[k]) == want, (name, cells, i, sorted(E.flagged(got[k]) ^ want))
            seen |= want
        # every changed cell shows on one of its two rows, except where only a permutation closes over it (row n - 1)
        assert seen or got.z_flags.any() or S.explain_trace_host(c["stark"], bad, c["pi"], seed=E.SEED).z_failing_rows.any(), (name, cells)
    if name == "g1op":
        assert not any(E.oracle_constraints(c, c["trace"], 5))
        ct = E.oracle_constraints(c, K.corrupt(c["trace"], [(5, 80)]), 5)
        n = c["stark"].num_constraints
        exps = list(range(181, 197)) + [262, 279] + list(range(281, 285)) + list(range(286, 297)) + [1896]
        assert n == 1913 and sorted(n - 1 - t for t, v in enumerate(ct) if v) == exps


@pytest.mark.parametrize("name", K.SMALL_TABLES)
def test_agreement_with_the_check(S, name):
    """Same seed, same traces, every row: a block of segment s is flagged <=> bit s of the check's row flag; a Z column below /
    from z_split <=> bit 2 / 3.  explain_trace_host == the column sums of explain_rows_host over all rows."""
    c = K.case(name)
    stark, n = c["stark"], c["n"]
    blocks = stark.constraint_blocks()
    seg = np.array([b.segment for b in blocks])
    B, Z = len(blocks), stark.num_permutation_zs()
    for cells, bad, _ in E.corrupted(name):
        rep = S.check_trace_host(stark, bad, c["pi"], seed=E.SEED, flags=True)
        rows = S.explain_rows_host(stark, bad, c["pi"], np.arange(n), seed=E.SEED)
        bits = np.unpackbits(rows.block_flags, axis=1, bitorder="little")[:, :B].astype(bool)
        zbits = np.unpackbits(rows.z_flags, axis=1, bitorder="little")[:, :Z].astype(bool)
        for s in (0, 1):
            assert np.array_equal(bits[:, seg == s].any(axis=1), (rep.row_flags >> s) & 1 != 0), (name, cells, s)
        assert np.array_equal(zbits[:, :rep.z_split].any(axis=1), (rep.row_flags >> 2) & 1 != 0), (name, cells)
        assert np.array_equal(zbits[:, rep.z_split:].any(axis=1), (rep.row_flags >> 3) & 1 != 0), (name, cells)
        e = S.explain_trace_host(stark, bad, c["pi"], seed=E.SEED)
        assert not e.ok
        for flags, cnt, first in ((bits, e.block_failing_rows, e.block_first_row), (zbits, e.z_failing_rows, e.z_first_row)):
            assert np.array_equal(flags.sum(axis=0).astype(np.uint64), cnt), (name, cells)
            want_first = np.where(flags.any(axis=0), flags.argmax(axis=0), NO_ROW).astype(np.uint64)
            assert np.array_equal(want_first, first), (name, cells)


RC_SECTIONS = ("range_check_recomposition", "range_check_lookup", "range_table")


@pytest.mark.parametrize("name", ["g1op", "modular", "fq12exp", "fq12exp_u64"])
def test_names_from_the_column_layout(S, name):
    """The sorted / permuted copy of range-check target 0 changed: every flagged block is a range-check block of instance 0, and
    the Z column flagged on row n - 1 has that column in its permutation pair.  The first gadget column changed: the flagged
    blocks of the head segment are gadget or transition blocks whose column span contains it (or the public-input block)."""
    c = K.case(name)
    stark, n = c["stark"], c["n"]
    gadget_col, rc_col, _ = c["cols"]
    exp = stark.kind in (S.AIR_FQ12_EXP, S.AIR_FQ12_EXP_U64)
    # a row on which the sorted copy steps to a new value: there the lookup constraint (next - local) * (next - next table) has a
    # non-zero first factor, and the changed table cell makes the second one -1
    sorted_col = c["trace"][rc_col - 1]
    r = next(i for i in range(2, n - 1) if sorted_col[i] != sorted_col[i - 1])
    bad = K.corrupt(c["trace"], [(r, rc_col)])
    got = S.explain_rows_host(stark, bad, c["pi"], [r - 1, r, n - 1], seed=E.SEED)
    hit = [b for x in got for b in x.blocks]
    assert got[0].blocks and all(b.name in RC_SECTIONS and b.instance == 0 for b in hit), [str(b) for b in hit]
    assert all(b.segment == (1 if exp else 0) for b in hit)
    assert all(b.col_first <= rc_col < b.col_first + b.col_count for b in hit)
    assert got[0].zs == [] and got[1].zs == [] and len(got[2].zs) >= 1
    assert all(rc_col in stark.permutation_pair(z) for z in got[2].zs)
    assert f"Z {got[2].zs[0]} (cols " in str(got[2]) and str(got[2]).startswith(f"row {n - 1}")
    assert str(got[0]).startswith(f"row {r - 1}") and "range_check_lookup[0] cols" in str(got[0])

    # the first gadget column changed on each of the rows 1 .. 64 (one trace copy: the rows do not share a gadget)
    rows = list(range(1, 65))
    bad = K.corrupt(c["trace"], [(i, gadget_col) for i in rows])
    got = S.explain_rows_host(stark, bad, c["pi"], rows, seed=E.SEED)
    head = [b for x in got for b in x.blocks if b.segment == 0 and b.name not in RC_SECTIONS]
    assert any(b.name.startswith("gadget_") for b in head), str(got)
    for b in head:
        assert b.name == "public_inputs" or (b.name.startswith(("gadget_", "transition_")) and b.col_first <= gadget_col < b.col_first + b.col_count), str(b)
    # the tables without a tail segment keep the range check of the changed limb in the head: it names that limb's target
    rc = [b for x in got for b in x.blocks if b.name in RC_SECTIONS]
    assert all(b.name == "range_check_recomposition" for b in rc) and len({b.instance for b in rc}) <= 1
    assert "gadget_" in str(got)


def test_argument_errors(S):
    L = S.lib()
    c = K.case("lookup")
    tr, air = np.array(c["trace"]), c["stark"]._d
    rows = np.array([0, 511], dtype=np.uint64)
    bf, zf = np.zeros((2, 1), dtype=np.uint8), np.zeros((2, 1), dtype=np.uint8)
    stats, zstats = np.zeros((2, 2), dtype=np.uint64), np.zeros((2, 2), dtype=np.uint64)
    p = S.api._ptr
    rows_call = lambda air, tr, bits, rows, k, bf: L.sbn_explain_rows_host(C.byref(air) if air else None, p(tr), bits, None, 0, 0, p(rows), k, p(bf), p(zf))  # noqa: E731
    trace_call = lambda air, tr, bits, st: L.sbn_explain_trace_host(C.byref(air) if air else None, p(tr), bits, None, 0, 0, p(st), p(zstats))  # noqa: E731
    assert rows_call(air, tr, 9, rows, 2, bf) == 0 and trace_call(air, tr, 9, stats) == 0
    assert rows_call(air, tr, 9, rows, 0, bf) == 0 and rows_call(air, tr, 9, None, 0, None) == 0      # an empty list is fine
    assert L.sbn_explain_rows_host(C.byref(air), p(tr), 9, None, 0, 0, p(rows), 2, p(bf), None) == 0    # the Z flags are optional
    assert L.sbn_explain_trace_host(C.byref(air), p(tr), 9, None, 0, 0, p(stats), None) == 0
    assert rows_call(None, tr, 9, rows, 2, bf) == -1 and rows_call(air, None, 9, rows, 2, bf) == -1
    assert rows_call(air, tr, 9, None, 2, bf) == -1 and rows_call(air, tr, 9, rows, 2, None) == -1
    assert trace_call(None, tr, 9, stats) == -1 and trace_call(air, None, 9, stats) == -1 and trace_call(air, tr, 9, None) == -1
    assert rows_call(air, tr, 9, np.array([0, 512], dtype=np.uint64), 2, bf) == -1 and b"row 512" in L.sbn_last_error()
    assert rows_call(S.api._AirDesc(99, 0), tr, 9, rows, 2, bf) == -1 and trace_call(S.api._AirDesc(99, 0), tr, 9, stats) == -1
    assert rows_call(air, tr, 8, rows, 2, bf) == -7 and trace_call(air, tr, 8, stats) == -7     # as sbn_check_trace_host
    assert rows_call(S.api._AirDesc(S.AIR_FLAGS, 2), tr, 9, rows, 2, bf) == -1
    pi1 = np.zeros(1, dtype=np.uint64)
    assert L.sbn_explain_rows_host(C.byref(air), p(tr), 9, p(pi1), 1, 0, p(rows), 2, p(bf), p(zf)) == -1
    tr[1, 17] = K.P
    assert rows_call(air, tr, 9, rows, 2, bf) == -2 and b"trace word 529 " in L.sbn_last_error()
    assert trace_call(air, tr, 9, stats) == -2
    with pytest.raises(S.SbnError) as e:
        S.explain_rows_host(c["stark"], tr, c["pi"], [0])
    assert e.value.code == -2
    with pytest.raises(S.SbnError):
        S.explain_trace_host(c["stark"], tr[:3], c["pi"])
    # the device forms refuse a null prover before they look for a device
    assert L.sbn_prover_explain_rows(None, 0, p(rows), 2, p(bf), None) == -1 and L.sbn_prover_explain_trace(None, 0, p(stats), None) == -1
    assert L.sbn_split_prover_explain_rows(None, 0, p(rows), 2, p(bf), None) == -1 and L.sbn_split_prover_explain_trace(None, 0, p(stats), None) == -1
    assert L.sbn_prover_explain_times(None, None, 0) == 0
    lhs, rhs = C.c_uint32(), C.c_uint32()
    assert L.sbn_air_permutation_pair(C.byref(air), 1, C.byref(lhs), C.byref(rhs)) == 0 and (lhs.value, rhs.value) == (1, 3)
    assert L.sbn_air_permutation_pair(C.byref(air), 2, C.byref(lhs), C.byref(rhs)) == -1
    assert L.sbn_air_permutation_pair(C.byref(air), 0, None, C.byref(rhs)) == -1
