"""Every column of every table through the host trace check and explain (no device): tests/column_sweep.py changes one cell per
column per pass, and what the check flags must be what the oracle's evaluator (AIR segments) and a numpy multiset comparison
(permutation segments) say -- row by row, Z column by Z column, both ways.  A column that a constraint template never reads,
reads at the wrong offset or puts into the wrong segment shows here as a named (table, column, row); a column that the
references themselves leave unbound must be one of column_sweep.FREE_COLUMNS."""
import time

import numpy as np
import pytest

import check_trace_cases as K
import column_sweep as W

NO_ROW = (1 << 64) - 1


def test_recipe():
    """The packing at both heights: rows distinct and 4 apart inside a copy (asserted by plan), every column once per pass, and
    over the four passes a column meets four rows of different residues mod 4."""
    for n, ncols in ((512, 4), (512, 126), (512, 127), (512, 9722), (1 << 16, 2822)):
        per = (n - 8) // 4
        seen = {}
        for p in range(W.PASSES):
            copies = W.plan(n, ncols, p)
            assert len(copies) == -(-ncols // per)
            for cells in copies:
                for r, col in cells:
                    seen.setdefault(col, []).append(r)
        assert sorted(seen) == list(range(ncols))
        assert all(sorted(r % 4 for r in rows) == [0, 1, 2, 3] for rows in seen.values())
    assert W.cell_row(512, 0, 0) == 4 and W.cell_row(512, 1, 0) == 4 + 4 * 37 and W.cell_row(512, 125, 3) == 4 + 4 * ((37 * 125 + 51) % 126) + 3
    spread = {W.cell_row(1 << 16, k, 0) // 512 for k in range(2822)}
    assert len(spread) == 128                      # at 2^16 rows one pass reaches every instance


def _agreement_with_explain(S, c, bad, rep, who):
    """test_explain_host.test_agreement_with_the_check on one copy: a block of segment s is flagged <=> bit s of the row flag, a
    Z column below / from z_split <=> bit 2 / 3, on every row; explain_trace_host == the column sums."""
    stark, n = c["stark"], c["n"]
    blocks = stark.constraint_blocks()
    seg = np.array([b.segment for b in blocks])
    B, Z = len(blocks), stark.num_permutation_zs()
    rows = S.explain_rows_host(stark, bad, c["pi"], np.arange(n), seed=W.SEED)
    e = S.explain_trace_host(stark, bad, c["pi"], seed=W.SEED)
    failing = np.zeros(n, dtype=bool)
    for lo in range(0, n, 4096):                   # (a G2 table has 3,000 blocks: unpack a slab of rows at a time)
        hi = min(n, lo + 4096)
        bits = np.unpackbits(rows.block_flags[lo:hi], axis=1, bitorder="little")[:, :B].astype(bool)
        zbits = np.unpackbits(rows.z_flags[lo:hi], axis=1, bitorder="little")[:, :Z].astype(bool)
        f = rep.row_flags[lo:hi]
        for s in (0, 1):
            assert np.array_equal(bits[:, seg == s].any(axis=1), (f >> s) & 1 != 0), (who, s, lo)
        assert np.array_equal(zbits[:, :rep.z_split].any(axis=1), (f >> 2) & 1 != 0), (who, lo)
        assert np.array_equal(zbits[:, rep.z_split:].any(axis=1), (f >> 3) & 1 != 0), (who, lo)
        failing[lo:hi] = bits.any(axis=1) | zbits.any(axis=1)
    # the statistics over the failing rows alone (every other row adds nothing)
    idx = np.nonzero(failing)[0]
    bits = np.unpackbits(rows.block_flags[idx], axis=1, bitorder="little")[:, :B].astype(bool)
    zbits = np.unpackbits(rows.z_flags[idx], axis=1, bitorder="little")[:, :Z].astype(bool)
    for flags, cnt, first in ((bits, e.block_failing_rows, e.block_first_row), (zbits, e.z_failing_rows, e.z_first_row)):
        assert np.array_equal(flags.sum(axis=0).astype(np.uint64), cnt), who
        want_first = np.where(flags.any(axis=0), idx[flags.argmax(axis=0)] if len(idx) else 0, NO_ROW).astype(np.uint64)
        assert np.array_equal(want_first, first), who


@pytest.mark.parametrize("name", W.TABLES)
def test_every_column_against_the_references(S, O, name):
    """Four passes.  Every copy: AIR flags == the oracle on rows r - 1, r, r + 1 of every cell, 0 and n - 1 (the controls r + 1
    clean in both, no AIR bit anywhere else); failing Z columns == the numpy multiset comparison, bits 2 / 3 on row n - 1
    alone.  Then the coverage: the references bind every column but those of FREE_COLUMNS."""
    c = K.case(name)
    stark, n, pi, valid = c["stark"], c["n"], c["pi"], c["trace"]
    ncols = valid.shape[0]
    assert W.broken_zs(name, valid) == set()
    air_bound = set()
    t0 = time.perf_counter()
    for p in range(W.PASSES):
        for k, (cells, bad) in enumerate(W.copies(valid, p)):
            who = f"{name} pass {p} copy {k}"
            rep = S.check_trace_host(stark, bad, pi, seed=W.SEED, flags=True)
            K.consistent(rep)
            air = (rep.row_flags & 3) != 0
            rows = W.air_rows(n, cells)
            want = W.oracle_nonzero(c, bad, rows)
            owner = W.cell_of_row(cells)
            for i in rows:
                assert bool(air[i]) == want[i], f"{who}: row {i} (cell (row, column) = {owner.get(i)}): check {int(rep.row_flags[i]) & 3:#x}, oracle {want[i]}"
            for r, col in cells:
                assert not want[r + 1] and not air[r + 1] and not air[r + 2], f"{who}: control rows of column {col}, row {r}"
                if want[r - 1] or want[r]:
                    air_bound.add(col)
            elsewhere = [int(i) for i in np.nonzero(air)[0] if int(i) not in want]
            if elsewhere:                           # only rows the oracle names as well may carry an AIR bit
                also = K.oracle_nonzero(c, bad, elsewhere)
                assert all(also.values()), f"{who}: the check flags rows {[i for i in elsewhere if not also[i]]} that read no changed cell; the oracle does not"
            # permutation segments
            e = S.explain_trace_host(stark, bad, pi, seed=W.SEED)
            got_z = {int(z) for z in np.nonzero(e.z_failing_rows)[0]}
            want_z = W.broken_zs(name, bad)
            assert got_z == want_z, f"{who}: Z columns {sorted(got_z ^ want_z)[:8]} (pairs {[W.pairs(name)[z] for z in sorted(got_z ^ want_z)[:8]]}): explain {sorted(got_z)[:8]}, numpy {sorted(want_z)[:8]}"
            assert all(int(e.z_failing_rows[z]) == 1 and int(e.z_first_row[z]) == n - 1 for z in got_z), who
            assert bool(rep.row_flags[n - 1] & 4) == any(z < rep.z_split for z in want_z), who
            assert bool(rep.row_flags[n - 1] & 8) == any(z >= rep.z_split for z in want_z), who
            assert not (rep.row_flags[:n - 1] & 12).any(), who
            assert rep.num_zs == len(W.pairs(name)) and not rep.ok
            if p == 0 and k == 0:
                _agreement_with_explain(S, c, bad, rep, who)
            del bad
    # coverage, from the references alone
    unbound = []
    for col in sorted(set(range(ncols)) - air_bound):
        cells = [(W.cell_row(n, col % ((n - 8) // 4), p), col) for p in range(W.PASSES)]
        if not any(W.bump_breaks_a_pair(name, valid, cell) for cell in cells):
            unbound.append(col)
    print(f"{name}: {ncols} columns, {len(air_bound)} bound by the AIR, {time.perf_counter() - t0:.1f} s")
    assert unbound == W.FREE_COLUMNS.get(name, []), f"{name}: columns {unbound} are bound by no constraint and no permutation pair of the oracle"


@pytest.mark.parametrize("name", sorted(W.FREE_COLUMNS))
def test_listed_free_columns_pass_the_check(S, O, name):
    """The other direction for the filter columns: the oracle is zero on every row of the one-cell trace, the column is in no
    permutation pair, and check_trace_host passes it."""
    c = K.case(name)
    n = c["n"]
    for col in W.FREE_COLUMNS[name]:
        assert not any(col in pair for pair in W.pairs(name))
        for p in range(W.PASSES):
            cell = (W.cell_row(n, col % ((n - 8) // 4), p), col)
            bad = W.one_cell(c["trace"], cell)
            assert not np.array_equal(bad, c["trace"])
            assert not any(K.oracle_nonzero(c, bad).values()), (name, cell)
            rep = S.check_trace_host(c["stark"], bad, c["pi"], seed=W.SEED, flags=True)
            assert rep.ok and not rep.row_flags.any(), (name, cell, str(rep))
            assert S.explain_trace_host(c["stark"], bad, c["pi"], seed=W.SEED).ok
