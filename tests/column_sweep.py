"""Shared by tests/test_column_sweep_host.py and tests/test_column_sweep_gpu.py: every column of every table changed once per
pass, packed many cells to a trace copy, and the two independent references that say what such a copy must break.

A pass changes one cell of every column to (v + 1) mod p.  Cell k of a copy sits on row 4 + 4 ((37 k + 17 pass) mod per) +
(pass mod 4), per = (n - 8) // 4, and the columns are taken `per` at a time: the rows of one copy are distinct and at least 4
apart, so the rows {r - 1, r} whose constraints read a cell never meet another cell's, and r + 1, r + 2 stay untouched as
controls.  A 512-row table needs ceil(columns / 126) copies per pass, a 2^16-row table one.

References (never the code under test):
 - the AIR segments: the oracle's constraint-by-constraint evaluator (check_trace_cases.oracle_nonzero) on rows r - 1, r, r + 1
   of every cell and on rows 0 and n - 1;
 - the permutation segments: Z column z with pair (lhs, rhs) fails exactly when sort(lhs column) != sort(rhs column), in numpy;
   no challenge enters it."""
import functools
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import check_trace_cases as K
import oracle_lib as O

P = K.P
SEED = 0x9E3779B97F4A7C15
PASSES = 4
TABLES = list(K.SMALL_TABLES) + ["fq12mul", "g1exp", "g2exp", "fqexp"]
DEVICE_WITNESS = ("g1exp", "g2exp", "fqexp")       # the device tests sweep what the device generator wrote

# The columns no constraint and no permutation pair of the REFERENCE binds: the filter of its three single-operation test
# tables.  A filter multiplies every constraint of the gadget behind it and has no constraint of its own (no f (f - 1), no
# public input), and on a valid row the gadget's constraints vanish, so any value passes:
#   g1op    384   is_add     src/curves/g1/muladd.rs:574-581  (eval_g1_add(yield_constr, is_add, ..); is_double, column 385, is
#                            bound only because the rows are additions: eval_g1_double does not vanish on them)
#   modular 144   filter     src/modular/modular.rs:468-481   (eval_modular_op(yield_constr, filter, ..), :123 and :228)
#   fq12mul 1728  filter     src/fields/fq12/mul.rs:443-447   (eval_fq12_mul(yield_constr, filter, x, y, &output), :256-267)
# The Exp tables drive these gadgets with their flag columns, which are boolean-constrained: they have no such column.  A
# column that shows up unbound and is not such a filter is a finding about the AIR, not an entry for this dict.
FREE_COLUMNS = {"g1op": [384], "modular": [144], "fq12mul": [1728]}
assert all(len(v) <= 1 for v in FREE_COLUMNS.values()) and set(FREE_COLUMNS) <= {"g1op", "modular", "fq12mul"}


def cell_row(n, k, p):
    per = (n - 8) // 4
    return 4 + 4 * ((37 * k + 17 * p) % per) + (p % 4)


@functools.lru_cache(maxsize=None)
def plan(n, ncols, p):
    """The copies of pass p: a tuple of tuples of (row, column)."""
    per = (n - 8) // 4
    out = []
    for first in range(0, ncols, per):
        cells = tuple((cell_row(n, k, p), first + k) for k in range(min(per, ncols - first)))
        rows = sorted(r for r, _ in cells)
        assert len(set(rows)) == len(cells), "two cells of a copy share a row"
        assert all(b - a >= 4 for a, b in zip(rows, rows[1:])) and rows[0] >= 4 and rows[-1] + 3 <= n - 1, "cells closer than 4 rows"
        assert all(r % 4 == p % 4 for r in rows)
        out.append(cells)
    assert sorted(col for cells in out for _, col in cells) == list(range(ncols))
    return tuple(out)


def copies(trace, p):
    """(cells, copy of `trace` with those cells changed) for every copy of pass p, built one at a time."""
    for cells in plan(trace.shape[1], trace.shape[0], p):
        yield cells, K.corrupt(trace, cells)


def air_rows(n, cells):
    """The rows the oracle is evaluated on: r - 1, r, r + 1 of every cell, 0 and n - 1."""
    return sorted({0, n - 1} | {r + d for r, _ in cells for d in (-1, 0, 1)})


def touched_rows(cells):
    """The rows whose constraints read a changed cell: r - 1 (as the next row) and r."""
    return sorted({r + d for r, _ in cells for d in (-1, 0)})


def cell_of_row(cells):
    """row -> the cell that row r - 1, r or r + 1 belongs to (for messages)."""
    return {r + d: (r, col) for r, col in cells for d in (-1, 0, 1)}


WORKERS = max(1, min(O._effective_cpus(), 16))
_pool = None


def _threads():
    global _pool
    if _pool is None:
        _pool = ThreadPoolExecutor(WORKERS)
    return _pool


def oracle_nonzero(c, trace, rows):
    """check_trace_cases.oracle_nonzero on `rows`, the rows shared out among host threads: the evaluator is re-entrant and
    ctypes drops the interpreter lock around it.  With the default 5 ms switch interval a thread coming back from a 0.5 ms
    call queues behind whichever thread holds the lock, and eight threads run no faster than one; 0.1 ms for the length of
    the call gives 4-5 x on eight CPUs."""
    rows = list(rows)
    if WORKERS == 1 or len(rows) < 4 * WORKERS:
        return K.oracle_nonzero(c, trace, rows)
    interval = sys.getswitchinterval()
    sys.setswitchinterval(1e-4)
    try:
        out = {}
        for part in _threads().map(lambda k: K.oracle_nonzero(c, trace, rows[k::WORKERS]), range(WORKERS)):
            out.update(part)
    finally:
        sys.setswitchinterval(interval)
    return out


@functools.lru_cache(maxsize=None)
def pairs(name):
    """[(lhs, rhs)] by Z column."""
    stark = K.case(name)["stark"]
    return [stark.permutation_pair(z) for z in range(stark.num_permutation_zs())]


def broken_zs(name, trace):
    """The Z columns whose two columns differ as multisets: plain numpy."""
    pr = np.array(pairs(name), dtype=np.int64).reshape(-1, 2)
    if not len(pr):
        return set()
    cols = np.unique(pr)                           # every column of a pair sorted once, a slab of columns per host thread
    slabs = np.array_split(cols, max(1, min(len(cols), trace.shape[1] * len(cols) >> 18)))
    srt = np.concatenate(list(_threads().map(lambda s: np.sort(trace[s], axis=1), slabs)))
    lhs, rhs = np.searchsorted(cols, pr[:, 0]), np.searchsorted(cols, pr[:, 1])
    step = max(1, (1 << 24) // trace.shape[1])      # pairs compared at a time
    return {z0 + int(z) for z0 in range(0, len(pr), step) for z in np.nonzero((srt[lhs[z0:z0 + step]] != srt[rhs[z0:z0 + step]]).any(axis=1))[0]}


def bump_breaks_a_pair(name, trace, cell):
    """Does changing `cell` alone break the multiset equality of a pair its column is in?  (The valid columns are equal as
    multisets: broken_zs(valid trace) is empty, which the tests assert.)"""
    r, col = cell
    mine = [(lhs, rhs) for lhs, rhs in pairs(name) if col in (lhs, rhs)]
    if not mine:
        return False
    bad = np.array(trace[col])
    bad[r] = (int(bad[r]) + 1) % P
    bad.sort()
    return any(not np.array_equal(bad, np.sort(trace[rhs if col == lhs else lhs])) for lhs, rhs in mine)


def one_cell(trace, cell):
    return K.corrupt(trace, [cell])
