"""Shared by tests/test_perm_diff_host.py and tests/test_perm_diff_gpu.py: the independent reference of the permutation explain
(numpy alone: np.unique with counts and first indices on both columns of a pair; only the pair list comes from the library's
sbn_air_permutation_pair), the cells the tests change, and the comparison of a PermutationExplanation with the reference.
The per-column work on a valid trace is done once per process and shared: a corrupted copy recomputes its changed columns only."""
import numpy as np

import check_trace_cases as K

P = K.P
NO_ROW = (1 << 64) - 1
SEAM_VALUES = [0, 32767, 32768, 65535, 65536, P - 1]     # the ends and the seam of the two histogram halves; out of range

_columns = {}    # (id of a read-only valid trace, column) -> (values, first rows, counts); the traces of K.case live as long as the process


def _unique(col):
    return np.unique(col, return_index=True, return_counts=True)


def _column(trace, c, clean, changed):
    if clean is None or c in changed:
        return _unique(trace[c])
    key = (id(clean), c)
    if key not in _columns:
        assert not clean.flags.writeable
        _columns[key] = _unique(clean[c])
    return _columns[key]


def pair_reference(left, right, per_pair):
    """(differing values, excess lhs, excess rhs), [(value, count lhs, count rhs, first row lhs, first row rhs)] of the first
    per_pair differing values in ascending order, from the two np.unique results."""
    vl, il, cl = left
    vr, ir, cr = right
    if np.array_equal(vl, vr) and np.array_equal(cl, cr):
        return (0, 0, 0), []
    allv = np.union1d(vl, vr)
    count = np.zeros((2, len(allv)), dtype=np.int64)
    first = np.full((2, len(allv)), NO_ROW, dtype=np.uint64)
    for s, (v, i, c) in enumerate(((vl, il, cl), (vr, ir, cr))):
        at = np.searchsorted(allv, v)
        count[s, at], first[s, at] = c, i.astype(np.uint64)
    d = count[0] - count[1]
    differ = np.nonzero(d)[0]
    stats = (len(differ), int(d[d > 0].sum()), int(-d[d < 0].sum()))
    entries = [(int(allv[k]), int(count[0, k]), int(count[1, k]), int(first[0, k]), int(first[1, k])) for k in differ[:per_pair]]
    return stats, entries


def reference(stark, trace, zs=None, per_pair=8, clean=None, changed=()):
    """[(z, stats, entries)] per output index.  clean / changed: the read-only valid trace `trace` was copied from and the
    columns in which it differs from it."""
    zs = range(stark.num_permutation_zs()) if zs is None else [int(z) for z in zs]
    changed = set(changed)
    out = []
    for z in zs:
        lhs, rhs = stark.permutation_pair(z)
        out.append((z,) + pair_reference(_column(trace, lhs, clean, changed), _column(trace, rhs, clean, changed), per_pair))
    return out


def assert_equals_reference(got, ref):
    """A PermutationExplanation against reference(): the pair of every output index, its statistics and its entries."""
    assert len(got.zs) == len(ref) and got.stats.shape == (len(ref),)
    for k, (z, stats, entries) in enumerate(ref):
        st = got.stats[k]
        assert int(got.zs[k]) == z
        assert (int(st["differing_values"]), int(st["excess_lhs"]), int(st["excess_rhs"])) == stats, (z, st, stats)
        assert int(st["entries"]) == len(entries), (z, st, len(entries))
        assert [tuple(int(x) for x in e) for e in got.entries[k, :len(entries)]] == entries, (z, got.entries[k, :len(entries)], entries)
    failing = sorted(z for z, stats, _ in ref if stats[0])
    assert got.ok == (not failing) and [q["z"] for q in got.pairs] == failing


def other_value(trace, col, row):
    """Another value of the column's own range for one cell: the neighbour below, or above for a zero."""
    v = int(trace[col, row])
    return v - 1 if v else 1


def set_cells(trace, cells):
    """A writable copy with trace[col, row] = value for every (col, row, value); and the columns that changed."""
    bad = np.array(trace, dtype=np.uint64)
    for col, row, value in cells:
        bad[col, row] = value
    return bad, {col for col, _, _ in cells}


def lookup_matrix(n, seed):
    """A 4-column LookupStark matrix of n rows that need not satisfy the AIR: random canonical 64-bit words, column 2 a shuffle
    of column 0 and column 3 a shuffle of column 1."""
    rng = np.random.default_rng(seed)
    m = np.empty((4, n), dtype=np.uint64)
    for c in (0, 1):
        m[c] = rng.integers(0, P, size=n, dtype=np.uint64)
        m[c, 7] = m[c, 3]                                # a repeated value, on both sides
        m[c + 2] = rng.permutation(m[c])
    return m
