"""The values and rows behind a failing permutation pair, host form (sbn_explain_permutations_host; csrc/perm_diff.hpp on the host
pool) against the numpy reference of tests/perm_diff_cases.py: statistics of ALL pairs and every listed entry, on the valid traces
of the 512-row tables and on copies with cells of permuted columns changed.  No device."""
import ctypes as C

import numpy as np
import pytest

import check_trace_cases as K
import perm_diff_cases as PC

TABLES = ["g1op", "modular", "fq12exp", "lookup", "flags"]
PAIRED = [t for t in TABLES if t != "flags"]


def _check(S, c, bad, changed, zs=None, per_pair=8):
    got = S.explain_permutations_host(c["stark"], bad, zs, per_pair)
    PC.assert_equals_reference(got, PC.reference(c["stark"], bad, zs, per_pair, clean=c["trace"], changed=changed))
    return got


def _pair(c, k=0):
    """(z, lhs column, rhs column) of a pair in the middle of the table (k: another one)."""
    z = (c["stark"].num_permutation_zs() // 2 + k) % c["stark"].num_permutation_zs()
    return (z,) + c["stark"].permutation_pair(z)


@pytest.mark.parametrize("name", TABLES)
def test_valid_trace_is_clean(S, name):
    c = K.case(name)
    got = _check(S, c, c["trace"], ())
    assert got.ok and got.pairs == [] and str(got).startswith("ok")
    assert len(got.stats) == c["stark"].num_permutation_zs() and got.entries.shape == (len(got.stats), 8)
    if name == "flags":
        assert len(got.stats) == 0


@pytest.mark.parametrize("name", PAIRED)
@pytest.mark.parametrize("last", [False, True])
def test_one_cell_changed_to_another_value_in_range(S, name, last):
    """Row 0 and row n - 1 of an rhs column: exactly two differing values in that pair, no other pair touched."""
    c = K.case(name)
    z, lhs, rhs = _pair(c)
    row = c["n"] - 1 if last else 0
    bad, changed = PC.set_cells(c["trace"], [(rhs, row, PC.other_value(c["trace"], rhs, row))])
    got = _check(S, c, bad, changed)
    hit = [q for q in got.pairs if q["rhs_col"] == rhs or q["lhs_col"] == rhs]
    assert hit and [q["z"] for q in got.pairs] == [q["z"] for q in hit]
    q = [q for q in hit if q["z"] == z][0]
    assert (q["differing_values"], q["excess_lhs"], q["excess_rhs"], len(q["entries"])) == (2, 1, 1, 2)
    new = [e for e in q["entries"] if e["value"] == int(bad[rhs, row])][0]
    assert new["count_rhs"] == new["count_lhs"] + 1 and new["first_row_rhs"] <= row


@pytest.mark.parametrize("name", PAIRED)
def test_seam_end_and_out_of_range_values(S, name):
    """0, 32767 | 32768 (the seam of the two histogram halves), 65535, and 65536 and p - 1 (no bin's): each alone in a cell of an
    rhs column, then all six in one column."""
    c = K.case(name)
    z, lhs, rhs = _pair(c, 1)
    rows = [3, 100, 255, 256, 300, c["n"] - 1]
    for row, v in zip(rows, PC.SEAM_VALUES):
        bad, changed = PC.set_cells(c["trace"], [(rhs, row, v)])
        got = _check(S, c, bad, changed, zs=[z])
        assert not got.ok or int(c["trace"][rhs, row]) == v
    bad, changed = PC.set_cells(c["trace"], [(rhs, row, v) for row, v in zip(rows, PC.SEAM_VALUES)])
    got = _check(S, c, bad, changed, per_pair=16)
    q = [q for q in got.pairs if q["z"] == z][0]
    assert [e["value"] for e in q["entries"]] == sorted(e["value"] for e in q["entries"]) and q["entries"][-1]["value"] == PC.P - 1
    assert q["entries"][-1]["first_row_lhs"] is None and q["entries"][-1]["first_row_rhs"] == c["n"] - 1


@pytest.mark.parametrize("name", PAIRED)
def test_swapped_cells_leave_the_pair_clean(S, name):
    """Multiset semantics: two cells of one column exchanged."""
    c = K.case(name)
    z, lhs, rhs = _pair(c)
    col = np.array(c["trace"][rhs])
    a, b = 0, int(np.nonzero(col != col[0])[0][0]) if (col != col[0]).any() else 1
    bad, changed = PC.set_cells(c["trace"], [(rhs, a, int(col[b])), (rhs, b, int(col[a]))])
    assert _check(S, c, bad, changed).ok


@pytest.mark.parametrize("name", PAIRED)
def test_cap_lists_the_smallest_and_counts_all(S, name):
    """20 distinct wrong values in one pair with per_pair = 8: the 8 smallest are listed, the statistics stay exact; per_pair = 0
    writes no entry (entries_out NULL)."""
    c = K.case(name)
    z, lhs, rhs = _pair(c)
    wrong = [40000 + 3 * i for i in range(18)] + [65536 + 5, PC.P - 2]
    assert not np.isin(np.array(wrong, dtype=np.uint64), c["trace"][[lhs, rhs]]).any()
    bad, changed = PC.set_cells(c["trace"], [(rhs, 11 + 23 * i, v) for i, v in enumerate(wrong)])
    got = _check(S, c, bad, changed)
    q = [q for q in got.pairs if q["z"] == z][0]
    assert q["differing_values"] >= 20 and q["excess_rhs"] == 20 and q["excess_lhs"] == 20 and len(q["entries"]) == 8
    everything = _check(S, c, bad, changed, zs=[z], per_pair=64)
    assert int(everything.stats["entries"][0]) == q["differing_values"]
    assert [e["value"] for e in everything.pairs[0]["entries"]][:8] == [e["value"] for e in q["entries"]]
    assert [e["value"] for e in everything.pairs[0]["entries"]][-2:] == [65536 + 5, PC.P - 2]
    none = _check(S, c, bad, changed, per_pair=0)
    assert none.entries.shape == (len(none.stats), 0) and not none.stats["entries"].any()
    assert all(np.array_equal(none.stats[f], got.stats[f]) for f in ("differing_values", "excess_lhs", "excess_rhs"))


def test_pair_subset_in_caller_order_and_refusals(S):
    c = K.case("modular")
    stark, Z = c["stark"], c["stark"].num_permutation_zs()
    z, lhs, rhs = _pair(c)
    bad, changed = PC.set_cells(c["trace"], [(rhs, 9, 65535), (stark.permutation_pair(0)[1], 2, 40001)])
    zs = [Z - 1, z, 0, z]
    got = _check(S, c, bad, changed, zs=zs)
    assert [int(x) for x in got.zs] == zs and [q["z"] for q in got.pairs] == [0, z, z]
    assert len(_check(S, c, bad, changed, zs=[]).stats) == 0
    with pytest.raises(S.SbnError) as e:
        S.explain_permutations_host(stark, bad, zs=[0, Z])
    assert e.value.code == -1
    # a word >= p, named by its index in the column-major matrix; the smaller of two wins
    worse = np.array(bad)
    worse[5, 17] = PC.P
    worse[7, 3] = (1 << 64) - 1
    with pytest.raises(S.SbnError) as e:
        S.explain_permutations_host(stark, worse)
    assert e.value.code == -2 and "trace word %d " % (5 * c["n"] + 17) in str(e.value)
    # null arguments, an unknown table, a height the table does not prove: as the other host forms
    L, d = S.lib(), stark._d
    st = np.zeros(Z, dtype=S.PERM_PAIR_STAT)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.sbn_explain_permutations_host(None, ptr(bad), 9, None, 0, 0, ptr(st), None) == -1
    assert L.sbn_explain_permutations_host(C.byref(d), None, 9, None, 0, 0, ptr(st), None) == -1
    assert L.sbn_explain_permutations_host(C.byref(d), ptr(bad), 9, None, 0, 0, None, None) == -1
    assert L.sbn_explain_permutations_host(C.byref(d), ptr(bad), 9, None, 0, 1, ptr(st), None) == -1
    assert L.sbn_explain_permutations_host(C.byref(d), ptr(bad), 9, None, 0, 0, ptr(st), None) == 0 and st["differing_values"].any()
    assert L.sbn_explain_permutations_host(C.byref(d), ptr(bad), 8, None, 0, 0, ptr(st), None) == -7
    g1exp = S.G1ExpStark(1)
    assert L.sbn_explain_permutations_host(C.byref(g1exp._d), ptr(bad), 9, None, 0, 0, ptr(st), None) == -7


def test_text_names_values_counts_and_first_rows(S):
    """LookupStark's pair 0 (columns 0 and 2), 512 rows: 513 three times on the left and twice on the right, 514 once on the
    right only."""
    stark = S.MyStark()
    assert stark.permutation_pair(0) == (0, 2)
    m = np.zeros((4, 512), dtype=np.uint64)
    m[0] = 1000 + np.arange(512)
    m[0, [17, 100, 200]] = 513
    rest = np.delete(m[0], [17, 100, 200])
    m[2, [40, 50]] = 513
    m[2, 41] = 514
    m[2, np.delete(np.arange(512), [40, 41, 50])] = rest[::-1]
    got = S.explain_permutations_host(stark, m)
    PC.assert_equals_reference(got, PC.reference(stark, m))
    assert str(got) == ("Z 0 (cols 0, 2): 2 values differ, 1 cell more on each side; 513: 3 x lhs (first row 17), 2 x rhs (first row 40); "
                        "514: 0 x lhs, 1 x rhs (first row 41)")
    assert repr(got) == "<PermutationExplanation 1 of 2 pairs differ>"
    m[2, 50] = 515
    assert str(S.explain_permutations_host(stark, m, per_pair=1)) == (
        "Z 0 (cols 0, 2): 3 values differ, 2 cells more on each side; 513: 3 x lhs (first row 17), 1 x rhs (first row 40); 2 more not listed")


def test_exports_hold_the_new_names(S):
    for name in ("sbn_explain_permutations_host", "sbn_prover_explain_permutations", "sbn_prover_explain_permutation_times"):
        assert name in S.EXPORTS and hasattr(S.lib(), name)
