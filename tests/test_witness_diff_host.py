"""The witness diff without a device: the exports and bindings, the refusals of the header in their order, the instance list the
public inputs carry (sbn_instances_from_public_inputs) on the five seeded Exp cases, and the host twin (sbn_diff_witness_host: the
host generator into a temporary, the compare in 64 x 64 tiles, csrc/witness_diff.hpp) against the numpy reference of
tests/witness_diff_cases.py on the oracle's traces -- which it must find clean -- and on copies with planted cells."""
import ctypes as C

import numpy as np
import pytest

import tracegen_edges as T
import witness_diff_cases as W

BAD_ARG, UNSUPPORTED, WITNESS = -1, -7, -8
NEW = ("sbn_instances_from_public_inputs", "sbn_prover_diff_witness", "sbn_prover_diff_witness_times", "sbn_diff_witness_host")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _same(S, stark, case, bad, cap=16, ios=None, canonical=None):
    got = S.diff_witness_host(stark, bad, case["pi"], ios, cap)
    W.assert_equals_reference(got, W.reference(bad, case["trace"] if canonical is None else canonical, stark.num_main_columns, cap))
    return got


def test_exports_and_bindings(S):
    for name in NEW:
        assert name in S.EXPORTS and hasattr(S.lib(), name)
    assert S.WITNESS_CELL.itemsize == 32 and C.sizeof(S.api._WitnessDiff) == 80
    assert callable(S.Prover.diff_witness) and callable(S.Prover.diff_times) and callable(S.diff_witness_host) and callable(S.instances_from_public_inputs)
    assert S.lib().sbn_prover_diff_witness_times(None, None, 3) == 0


def test_refusals_in_header_order(S, fq12expu64_case):
    """Every argument refusal comes before the table, the table before the height, the height before the list; a later fault never
    hides an earlier one.  The device form refuses a null prover before it looks for a device."""
    L, c = S.lib(), fq12expu64_case
    stark = S.Fq12ExpU64Stark(16)
    trace, pi, ios = c["trace"], c["pi"], np.ascontiguousarray(c["ios"], dtype=np.uint32)
    raw = S.api._WitnessDiff(struct_size=C.sizeof(S.api._WitnessDiff))
    cells = np.zeros(4, dtype=S.WITNESS_CELL)

    def host(air=stark, tr=trace, bits=11, p=pi, n_pi=None, io=None, num_io=16, rep=raw, ce=cells, cap=4):
        return L.sbn_diff_witness_host(C.byref(air._d) if air is not None else None, _ptr(tr), bits, _ptr(p), len(pi) if n_pi is None else n_pi, _ptr(io), num_io,
                                       C.byref(rep) if rep is not None else None, None, None, _ptr(ce), cap)

    assert host() == 0 and raw.cells == 0 and raw.pi_words == 0
    assert L.sbn_prover_diff_witness(None, None, 16, C.byref(raw), None, None, None, 0) == BAD_ARG
    assert host(air=None) == BAD_ARG and host(tr=None) == BAD_ARG and host(p=None) == BAD_ARG and host(rep=None) == BAD_ARG
    wrong = S.api._WitnessDiff(struct_size=C.sizeof(S.api._WitnessDiff) - 8)
    lookup = S.MyStark()
    # 1. struct_size, the cap, a null list with a cap, num_io -- each also on a table, a height and a list that would be refused later
    assert host(air=lookup, rep=wrong, num_io=0) == BAD_ARG and "struct_size" in L.sbn_last_error().decode()
    assert host(air=lookup, cap=65537, ce=None, num_io=0) == BAD_ARG and "65536" in L.sbn_last_error().decode()
    assert host(air=lookup, ce=None, num_io=0) == BAD_ARG and "cells_out" in L.sbn_last_error().decode()
    assert host(cap=65536, ce=np.zeros(65536, dtype=S.WITNESS_CELL)) == 0 and host(cap=0, ce=None) == 0
    assert host(num_io=8, bits=5) == BAD_ARG and "instances" in L.sbn_last_error().decode()
    assert host(air=lookup, num_io=3) == BAD_ARG
    # 3. a table without an instance list, before its height is looked at
    assert host(air=lookup, num_io=0, bits=5) == UNSUPPORTED and "Exp tables" in L.sbn_last_error().decode()
    assert host(air=S.G1Stark(), num_io=0) == UNSUPPORTED
    # the shape of the arguments, before the list
    too_large = ios.copy()
    too_large[3, :8] = T.limbs(T.P, 8, 32)
    assert host(bits=12, io=too_large) == BAD_ARG and "degree_bits" in L.sbn_last_error().decode()
    assert host(n_pi=len(pi) - 1, io=too_large) == BAD_ARG and "public inputs" in L.sbn_last_error().decode()
    # 6. what the generator says about the list, behind the prefix
    assert host(io=too_large) == BAD_ARG
    assert L.sbn_last_error().decode().startswith("no canonical witness: ") and "instance 3" in L.sbn_last_error().decode()
    not_canonical = ios.copy()
    not_canonical[5, 192:194] = [0xFFFFFFFF, 0xFFFFFFFF]
    assert host(io=not_canonical) == -2 and L.sbn_last_error().decode().startswith("no canonical witness: ")
    # a public input wider than its limb, named by its index (ios == NULL: the list comes from the public inputs)
    per = len(pi) // 16
    wide = pi.copy()
    wide[2 * per + 7] = 1 << 16
    assert host(p=wide) == BAD_ARG and "public input %d " % (2 * per + 7) in L.sbn_last_error().decode()
    assert host(p=wide, io=ios) == 0 and raw.pi_words == 1 and raw.first_pi_word == 2 * per + 7      # a given list is compared as given


CASES = {"g1": ("g1exp_case", "G1ExpStark"), "g2": ("g2exp_case", "G2ExpStark"), "fq": ("fqexp_case", "FqExpStark"), "fq12": ("fq12exp_case", "Fq12ExpStark"),
         "fq12u64": ("fq12expu64_case", "Fq12ExpU64Stark")}


@pytest.mark.parametrize("table", list(CASES))
def test_instances_from_public_inputs(S, request, table):
    """The inverse of generate_public_inputs: the case's ios word for word, and the outputs Python integers give for its native
    instances (every instance of the field tables; the first four and the last of the curves, whose Python walk is slow)."""
    case = request.getfixturevalue(CASES[table][0])
    stark = getattr(S, CASES[table][1])(len(case["ios"]))
    ios, outs = S.instances_from_public_inputs(stark, case["pi"])
    assert ios.dtype == np.uint32 and np.array_equal(ios, case["ios"])
    which = range(len(case["native"])) if table in ("fq", "fq12", "fq12u64") else [0, 1, 2, 3, len(case["native"]) - 1]
    for k in which:
        want = T.expected_output(table, case["native"][k])
        flat = [want] if table == "fq" else ([want[0], want[1]] if table == "g1" else ([want[0][0], want[0][1], want[1][0], want[1][1]] if table == "g2" else list(want)))
        assert [int(v) for v in outs[k]] == [w for v in flat for w in T.limbs(v, 8, 32)], (table, k)
    assert outs.shape == (len(case["ios"]), (ios.shape[1] - (2 if table == "fq12u64" else 8)) // 2)
    # a limb out of its range is refused by its index; the exponent word of the u64 table takes any value
    per = len(case["pi"]) // len(case["ios"])
    xw_pi = (per - (1 if table == "fq12u64" else 8)) // 3
    for at in (0, per + xw_pi + 1, 3 * per - 1):
        bad = case["pi"].copy()
        bad[at] = 1 << (16 if table in ("fq12", "fq12u64") else 32)
        with pytest.raises(S.SbnError) as e:
            S.instances_from_public_inputs(stark, bad)
        assert e.value.code == BAD_ARG and "public input %d " % at in str(e.value)
    if table == "fq12u64":
        any_word = case["pi"].copy()
        any_word[2 * xw_pi] = (1 << 64) - 1
        assert S.instances_from_public_inputs(stark, any_word)[0][0, 192:194].tolist() == [0xFFFFFFFF, 0xFFFFFFFF]
    with pytest.raises(S.SbnError) as e:
        S.instances_from_public_inputs(stark, case["pi"][:-1])
    assert e.value.code == BAD_ARG
    assert S.lib().sbn_instances_from_public_inputs(1, _ptr(case["pi"]), len(case["pi"]), len(case["ios"]), _ptr(ios), None) == BAD_ARG   # G1_OP


def test_host_twin_on_the_u64_table(S, fq12expu64_case):
    """Fq12ExpU64Stark(16), 2^11 x 9,792: the oracle's trace is clean; the single cells, a whole main column, a whole row, the
    scattered cells at caps 0, 1, exact and oversize; a list from another exponent."""
    c, stark = fq12expu64_case, S.Fq12ExpU64Stark(16)
    n, num_main, Cn = c["trace"].shape[1], stark.num_main_columns, stark.num_columns
    got = _same(S, stark, c, c["trace"])
    assert got.ok and got.listed == [] and str(got).startswith("ok") and got.first_row is None
    for cell in W.single_cells(n, num_main, Cn):
        got = _same(S, stark, c, W.plant(c["trace"], [cell]))
        assert (got.cells, got.first_row, got.first_column) == (1, cell[0], cell[1]) and not got.ok
        assert got.main_cells == (1 if cell[1] < num_main else 0)
    got = _same(S, stark, c, W.plant(c["trace"], W.whole_column(n, 7)))
    assert (got.cells, got.main_cells, got.rows, got.columns, len(got.listed)) == (n, n, n, 1, 16)
    got = _same(S, stark, c, W.plant(c["trace"], W.whole_row(Cn, 129)))
    assert (got.cells, got.main_cells, got.rows, got.columns, len(got.listed)) == (Cn, num_main, 1, Cn, 16)
    cells = W.scattered(n, num_main, Cn)
    bad = W.plant(c["trace"], cells)
    for cap in (0, 1, len(cells), len(cells) + 5):
        got = _same(S, stark, c, bad, cap)
        assert len(got.listed) == min(cap, len(cells)) and got.cells == len(cells) and got.main_cells == 4
    assert [q["main"] for q in got.listed] == [True] * 4 + [False] * 3 and got.listed[0]["row"] == 64 and got.listed[4]["row"] == 5
    assert (got.first_row, got.first_column) == (64, 64)
    assert got == S.diff_witness_host(stark, bad, c["pi"], c["ios"], len(cells) + 5)          # ios given == ios from the public inputs
    # one changed exponent bit: the diff is against THAT list's host trace, and its public inputs differ from the loaded ones
    ios = np.array(c["ios"], dtype=np.uint32)
    ios[3, 192] ^= 2
    other, other_pi = stark.generate_trace_and_public_inputs(ios)
    got = _same(S, stark, c, c["trace"], 16, ios, other)
    assert got.cells > 0 and got.pi_words == int((other_pi != c["pi"]).sum()) > 0 and got.first_pi_word == int(np.nonzero(other_pi != c["pi"])[0][0])
    assert got.listed[0]["instance"] == 3 and got.listed[0]["instance_row"] == got.listed[0]["row"] - 3 * 128


def test_host_twin_on_the_ragged_column_tile(S, g1exp_case):
    """G1ExpStark(128): 1,676 = 26 * 64 + 12 columns, the main / derived boundary at 398 inside a tile."""
    c, stark = g1exp_case, S.G1ExpStark(128)
    n, num_main, Cn = c["trace"].shape[1], stark.num_main_columns, stark.num_columns
    assert (num_main, Cn) == (398, 1676)
    bad = W.plant(c["trace"], [(100, 1675), (513, 217), (513, 397), (513, 398), (n - 1, 1664), (0, 1663)])
    got = _same(S, stark, c, bad)
    assert (got.cells, got.main_cells, got.first_row, got.first_column) == (6, 2, 513, 217)
    assert [(q["row"], q["column"]) for q in got.listed] == [(513, 217), (513, 397), (0, 1663), (100, 1675), (513, 398), (n - 1, 1664)]
    text = str(got)
    assert text.startswith("6 cells differ in 6 columns on 4 rows (2 in the main columns); row 513 (instance 1, row 1 of 512) col 217 [gadget_add, gadget_double]: got 0x")
    assert ", canonical 0x" in text and repr(got) == "<WitnessDiff 6 cells, 0 public inputs differ>"
    assert all(q["checked_by"] for q in got.listed) and "col 1675 [range_check_lookup[380]]: got 0x" in text
