"""Row-major traces without a device: sbn_air_num_main_columns, the host twin sbn_trace_from_rows_host in both modes against the
oracle's traces (the rows handed in are trace[:num_main].T or trace.T of the oracle's trace), its data errors, and the refusals
sbn_prove_rows makes before it looks for a device."""
import ctypes as C

import numpy as np
import pytest

GL_P = 0xFFFFFFFF00000001
BAD_ARG, NON_CANONICAL, NO_DEVICE, UNSUPPORTED, WITNESS = -1, -2, -3, -7, -8
NO_PI = np.zeros(0, dtype=np.uint64)


def main_rows(stark, trace):
    return np.ascontiguousarray(trace[:stark.num_main_columns].T)


def test_num_main_columns(S):
    got = [s.num_main_columns for s in (S.G1ExpStark(128), S.G2ExpStark(128), S.FqExpStark(128), S.Fq12ExpStark(16), S.Fq12ExpU64Stark(16))]
    assert got == [398, 782, 158, 1742, 1734]
    assert [s.num_main_columns for s in (S.G1ExpStark(1), S.Fq12ExpU64Stark(512))] == [398, 1734]   # num_io does not enter
    others = (S.G1Stark(), S.ModularStark(), S.Fq12Stark(), S.LookupStark(), S.FlagStark(16), S.FlagU64Stark(16))
    assert [s.num_main_columns for s in others] == [0] * 6
    assert S.lib().sbn_air_num_main_columns(None) == 0
    new = {"sbn_air_num_main_columns", "sbn_trace_from_rows_host", "sbn_prover_load_trace_rows", "sbn_prover_load_trace_rows_device", "sbn_prover_prove_host_rows", "sbn_prove_rows"}
    assert new <= set(S.EXPORTS) and all(hasattr(S.lib(), f) for f in new)


def test_main_rows_of_the_split_check_table_give_the_oracle_trace(S, fq12expu64_case):
    """Fq12ExpU64Stark(16): 2^11 rows, 1,734 of 9,792 columns, the split range check."""
    stark, trace = S.Fq12ExpU64Stark(16), fq12expu64_case["trace"]
    assert trace.shape == (9792, 2048)
    assert np.array_equal(S.trace_from_rows_host(stark, main_rows(stark, trace)), trace)


def test_main_rows_of_the_u16_table_give_the_oracle_trace(S, fqexp_case):
    """FqExpStark(128): 2^16 rows, 158 of 960 columns, the u16 range check."""
    stark, trace = S.FqExpStark(128), fqexp_case["trace"]
    assert trace.shape == (960, 65536)
    assert np.array_equal(S.trace_from_rows_host(stark, main_rows(stark, trace)), trace)


def test_whole_rows_in_every_form_give_the_oracle_trace(S, g1op_case):
    """G1Stark, 512 x 2,283: packed, with row_stride = n_cols + 3 and the padding filled with 2^64 - 1 (never read: it would be
    refused), and as a list of row arrays."""
    stark, trace = S.G1Stark(), np.ascontiguousarray(g1op_case["trace"], dtype=np.uint64)
    rows = np.ascontiguousarray(trace.T)
    assert rows.shape == (512, 2283)
    assert np.array_equal(S.trace_from_rows_host(stark, rows), trace)
    padded = np.full((512, 2283 + 3), 2**64 - 1, dtype=np.uint64)
    padded[:, :2283] = rows
    view = padded[:, :2283]
    table = S.RowTable(view)
    assert (table.raw.row_stride, table.raw.n_cols, table.raw.n_rows) == (2286, 2283, 512)
    assert np.array_equal(S.trace_from_rows_host(stark, table), trace)
    got, changed = S.trace_from_rows_host(stark, view, reduce=True)
    assert changed == 0 and np.array_equal(got, trace)
    as_list = [rows[r].copy() for r in range(512)]
    assert S.RowTable(as_list).raw.flat is None
    assert np.array_equal(S.trace_from_rows_host(stark, as_list), trace)


def test_words_beyond_p_are_refused_by_row_and_column_or_reduced(S, g1op_case, fq12expu64_case):
    stark, trace = S.G1Stark(), np.ascontiguousarray(g1op_case["trace"], dtype=np.uint64)
    rows = np.ascontiguousarray(trace.T)
    for planted in ([(7, 100)], [(300, 5), (299, 2282)], [(0, 0)], [(511, 2282)], [(64, 63), (63, 64)]):
        bad = rows.copy()
        for r, c in planted:
            bad[r, c] += np.uint64(GL_P)
        first = min(planted)   # row-major order: the smaller row, then the smaller column
        with pytest.raises(S.SbnError) as e:
            S.trace_from_rows_host(stark, bad)
        assert e.value.code == NON_CANONICAL and f"row {first[0]}, column {first[1]} " in str(e.value), str(e.value)
        got, changed = S.trace_from_rows_host(stark, bad, reduce=True)
        assert changed == len(planted) and np.array_equal(got, trace)
    # main-row mode: the same scan, and the reduced trace is the oracle's with its derived columns
    st2, tr2 = S.Fq12ExpU64Stark(16), fq12expu64_case["trace"]
    bad = main_rows(st2, tr2)
    bad[2047, 1733] += np.uint64(GL_P)
    bad[2047, 400] += np.uint64(GL_P)      # a range-checked column: reduced before the range test
    with pytest.raises(S.SbnError) as e:
        S.trace_from_rows_host(st2, bad)
    assert e.value.code == NON_CANONICAL and "row 2047, column 400 " in str(e.value)
    got, changed = S.trace_from_rows_host(st2, bad, reduce=True)
    assert changed == 2 and np.array_equal(got, tr2)


def test_a_range_checked_main_column_beyond_u16_is_a_witness_error(S, fq12expu64_case):
    stark, trace = S.Fq12ExpU64Stark(16), fq12expu64_case["trace"]
    rows = main_rows(stark, trace)
    first_rc, end_rc = 384, 384 + 84 * 16 - 12      # ExpShape of the Fq12 tables: [rc_start, rc_start + num_rc)
    for r, c in ((0, first_rc), (1000, end_rc - 1), (2047, 700)):
        bad = rows.copy()
        bad[r, c] = 65536
        with pytest.raises(S.SbnError) as e:
            S.trace_from_rows_host(stark, bad)
        assert e.value.code == WITNESS and f"row {r}, column {c}" in str(e.value), str(e.value)
    for c in (first_rc - 1, end_rc):                 # the neighbours are not range-checked: no refusal
        ok = rows.copy()
        ok[5, c] = 65536
        S.trace_from_rows_host(stark, ok)


def host_rows(S, flat=None, stride=0, ptrs=None, n_rows=0, n_cols=0, size=None):
    return S.api._HostRows(C.sizeof(S.api._HostRows) if size is None else size, 0, flat, stride, ptrs, n_rows, n_cols)


def test_prove_rows_refusals_come_before_the_device(S, fq12expu64_case):
    """Every refusal of the list in include/sbn.h returns its own code without a GPU, never SBN_ERR_NO_DEVICE; a clean call gets as
    far as the device (and, on this machine, no further)."""
    L = S.lib()
    stark = S.Fq12ExpU64Stark(16)
    cfg = stark.config()
    trace, pi = fq12expu64_case["trace"], np.ascontiguousarray(fq12expu64_case["pi"], dtype=np.uint64)
    rows = main_rows(stark, trace)
    n, nc = rows.shape
    ptrs = (rows.ctypes.data + 8 * nc * np.arange(n, dtype=np.uint64)).astype(np.uint64)

    def call(r, flags=0, pis=pi, n_pi=None, st=stark, out=True, air=True, config=True):
        h = C.c_void_p(1)
        rc = L.sbn_prove_rows(C.byref(st._d) if air else None, C.byref(cfg._c) if config else None, C.byref(r) if r is not None else None, flags,
                              pis.ctypes.data_as(C.c_void_p) if pis is not None else None, len(pi) if n_pi is None else n_pi, C.byref(h) if out else None)
        assert not out or h.value is None
        return rc, L.sbn_last_error().decode()

    good = host_rows(S, rows.ctypes.data, nc, None, n, nc)
    # 1. null arguments, struct_size
    assert call(None)[0] == BAD_ARG and call(good, out=False)[0] == BAD_ARG and call(good, air=False)[0] == BAD_ARG and call(good, config=False)[0] == BAD_ARG
    assert call(host_rows(S, rows.ctypes.data, nc, None, n, nc, size=40))[0] == BAD_ARG
    # 2. both or neither of flat / row_ptrs
    assert call(host_rows(S, rows.ctypes.data, nc, ptrs.ctypes.data, n, nc))[0] == BAD_ARG
    assert call(host_rows(S, None, nc, None, n, nc))[0] == BAD_ARG
    # 3. the height
    assert call(host_rows(S, rows.ctypes.data, nc, None, n - 1, nc))[0] == BAD_ARG
    assert call(host_rows(S, rows.ctypes.data, nc, None, n // 2, nc))[0] == BAD_ARG    # a power of two, not this table's
    # 4. n_cols, row_stride
    assert call(host_rows(S, rows.ctypes.data, nc, None, n, nc - 1))[0] == BAD_ARG
    rc, msg = call(host_rows(S, rows.ctypes.data, nc - 1, None, n, nc))
    assert rc == BAD_ARG and "row_stride" in msg
    # 5. pointers: the message names the row
    rc, msg = call(host_rows(S, rows.ctypes.data + 4, nc, None, n, nc))
    assert rc == BAD_ARG and msg == "row 0 is null or not 8-byte aligned"
    bad = ptrs.copy(); bad[77] = 0
    assert call(host_rows(S, None, 0, bad.ctypes.data, n, nc)) == (BAD_ARG, "row 77 is null or not 8-byte aligned")
    bad = ptrs.copy(); bad[2047] += 2
    assert call(host_rows(S, None, 0, bad.ctypes.data, n, nc)) == (BAD_ARG, "row 2047 is null or not 8-byte aligned")
    # 6. flags
    assert call(good, flags=2)[0] == BAD_ARG and call(good, flags=3)[0] == BAD_ARG
    # 7. public inputs: count, null, canonical form (reduced with the flag)
    assert call(good, n_pi=len(pi) - 1)[0] == BAD_ARG
    assert call(good, pis=None)[0] == BAD_ARG
    pi2 = pi.copy(); pi2[3] += np.uint64(GL_P)
    assert call(good, pis=pi2) == (NON_CANONICAL, "public input 3 is not canonical")
    # 8. main-row mode where it is not covered: another table's main-column count, a u16 table below 2^16 rows
    g1 = S.G1Stark()
    assert call(host_rows(S, rows.ctypes.data, 386, None, 512, 386), pis=NO_PI, n_pi=0, st=g1)[0] == UNSUPPORTED
    small = S.FqExpStark(8)
    assert call(host_rows(S, rows.ctypes.data, 158, None, 4096, 158), pis=pi, n_pi=small.num_public_inputs, st=small)[0] == UNSUPPORTED
    # the order: a wrong struct_size wins over everything behind it, a bad n_cols over a bad pointer
    assert "struct_size" in call(host_rows(S, None, 0, None, 3, 1, size=8), flags=9, n_pi=0)[1]
    assert "n_cols" in call(host_rows(S, rows.ctypes.data + 4, nc, None, n, 5))[1]
    if L.sbn_device_count() == 0:
        assert call(good)[0] == NO_DEVICE
        assert call(good, pis=pi2, flags=1)[0] == NO_DEVICE   # (reduced on the host, so no refusal)
        assert call(host_rows(S, None, 0, ptrs.ctypes.data, n, nc))[0] == NO_DEVICE


def test_trace_from_rows_host_refusals(S, g1op_case):
    L = S.lib()
    stark = S.G1Stark()
    rows = np.ascontiguousarray(np.ascontiguousarray(g1op_case["trace"], dtype=np.uint64).T)
    out = np.zeros(rows.size, dtype=np.uint64)

    def call(r, flags=0, dst=out):
        return L.sbn_trace_from_rows_host(C.byref(stark._d), C.byref(r), flags, dst.ctypes.data_as(C.c_void_p) if dst is not None else None, None)

    assert call(host_rows(S, rows.ctypes.data, 2283, None, 512, 2283)) == 0
    assert call(host_rows(S, rows.ctypes.data, 2283, None, 512, 2283), dst=None) == BAD_ARG
    assert call(host_rows(S, rows.ctypes.data, 2283, None, 500, 2283)) == BAD_ARG
    assert call(host_rows(S, rows.ctypes.data, 2283, None, 512, 2282)) == BAD_ARG
    assert call(host_rows(S, rows.ctypes.data, 2282, None, 512, 2283)) == BAD_ARG
    assert call(host_rows(S, rows.ctypes.data, 2283, None, 512, 2283), flags=4) == BAD_ARG
    assert call(host_rows(S, rows.ctypes.data, 386, None, 512, 386)) == UNSUPPORTED
    with pytest.raises(S.SbnError):
        S.RowTable(rows.T)                              # rows not contiguous
    with pytest.raises(S.SbnError):
        S.RowTable(rows.astype(np.int64))
    with pytest.raises(S.SbnError):
        S.RowTable([rows[0], rows[1][:-1]])             # another length
