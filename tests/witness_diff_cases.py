"""Shared by tests/test_witness_diff_host.py and tests/test_witness_diff_gpu.py: the independent reference of the witness diff (numpy
alone: np.argwhere over `trace != canonical`, sorted main columns first), the planted corruptions, and the comparison of a
WitnessDiff with the reference.  Every planted word stays canonical -- (v + 1) mod p -- so that a loader takes the trace; for a range-checked limb
of a main-row load the caller picks another value inside the range itself (plant_values)."""
import numpy as np

P = 0xFFFFFFFF00000001
NO_ROW = (1 << 64) - 1


def reference(trace, canonical, num_main, cap):
    """The diff of two [C][n] matrices in the order of include/sbn.h: ascending (row, column) over the main columns [0, num_main),
    the derived columns only behind them.  Returns a dict of the report's counts, the two per-column arrays and the first `cap`
    cells as (row, column, got, want)."""
    differs = trace != canonical
    column_cells = np.count_nonzero(differs, axis=1).astype(np.uint64)
    columns = np.nonzero(column_cells)[0]                        # only these are looked at cell by cell
    at = np.argwhere(differs[columns])                           # (index into columns, row)
    cells = np.stack([at[:, 1], columns[at[:, 0]]], axis=1) if len(at) else np.zeros((0, 2), dtype=np.int64)   # (row, column)
    column_first_row = np.full(len(column_cells), NO_ROW, dtype=np.uint64)
    column_first_row[columns] = differs[columns].argmax(axis=1).astype(np.uint64)     # of a row of booleans: the first True
    derived = cells[:, 1] >= num_main
    order = cells[np.lexsort((cells[:, 1], cells[:, 0], derived))]   # main before derived, then by row, then by column
    main = order[order[:, 1] < num_main]
    first = order[0] if len(order) else (None, None)
    rows = len(np.unique(cells[:, 0]))
    cells = [(int(r), int(c), int(trace[c, r]), int(canonical[c, r])) for r, c in order[:cap]]
    return {"cells": len(order), "main_cells": len(main), "rows": rows, "columns": int((column_cells > 0).sum()),
            "first_row": None if first[0] is None else int(first[0]), "first_column": None if first[1] is None else int(first[1]),
            "column_cells": column_cells, "column_first_row": column_first_row, "listed": cells}


def assert_equals_reference(got, ref):
    """A WitnessDiff against reference(): the counts, both per-column arrays and the list."""
    for f in ("cells", "main_cells", "rows", "columns", "first_row", "first_column"):
        assert getattr(got, f) == ref[f], (f, getattr(got, f), ref[f])
    assert np.array_equal(got.column_cells, ref["column_cells"])
    assert np.array_equal(got.column_first_row, ref["column_first_row"])
    assert [(c["row"], c["column"], c["got"], c["want"]) for c in got.listed] == ref["listed"]
    assert [tuple(int(x) for x in c) for c in got.raw_cells] == ref["listed"]


def plant(trace, cells):
    """A writable copy with (v + 1) mod p in every (row, column) of `cells`."""
    bad = np.array(trace, dtype=np.uint64)
    for r, c in cells:
        bad[c, r] = (int(bad[c, r]) + 1) % P
    return bad


def plant_values(trace, cells):
    """A writable copy with trace[column, row] = value for every (row, column, value)."""
    bad = np.array(trace, dtype=np.uint64)
    for r, c, v in cells:
        bad[c, r] = v
    return bad


def single_cells(n, num_main, C):
    """The single cells of the issue: the first cell, the last main cell, both sides of the 64 x 64 tile corner, the last cell."""
    return [(0, 0), (n - 1, num_main - 1), (63, 63), (64, 64), (n - 1, C - 1)]


def whole_column(n, column):
    return [(r, column) for r in range(n)]


def whole_row(C, row):
    return [(row, c) for c in range(C)]


def scattered(n, num_main, C):
    """Seven cells: four main ones on three rows (two share a row), three derived ones of which one lies on an EARLIER row than
    any main cell -- the list must still open with the main cells."""
    return [(5, num_main + 1), (70, 3), (70, num_main - 1), (64, 64), (n - 1, 0), (n - 2, C - 1), (200, C - 2)]
