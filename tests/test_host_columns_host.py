"""A host trace held as separate columns, without a device: the gather of Prover.prove_host_columns as a building block
(sbn_gather_columns, csrc/host_columns.hpp) against numpy, the host loop of sbn_reduce_words, the Python argument forms, and
the refusals the new C ABI calls make before they look for a device.  (sbn_prover_create needs a device, so the argument checks of
sbn_prover_prove_host_columns on a real prover are in test_host_columns_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

GL_P = 0xFFFFFFFF00000001
N, NCOLS = 8, 5
BAD_ARG = -1


def flat_of(cols):
    return np.concatenate([np.asarray(c) for c in cols])


def separate_columns(seed=3):
    """NCOLS columns of N words, each its own allocation."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 2**64, size=N, dtype=np.uint64) for _ in range(NCOLS)]


def odd_offset_columns():
    """One column sits at an odd 8-byte offset of a larger buffer: whatever numpy's allocation, one of the two is 8 bytes off a
    16-byte boundary, and both are tried."""
    out = []
    for lead in (1, 2):
        cols = separate_columns(5 + lead)
        big = np.random.default_rng(40 + lead).integers(0, 2**64, size=N + 3, dtype=np.uint64)
        cols[2] = big[lead:lead + N]
        out.append(cols)
    assert {c[2].ctypes.data % 16 for c in out} == {0, 8}
    return out


def aliasing_columns():
    cols = separate_columns(9)
    cols[4] = cols[1]
    return cols


COLUMN_SETS = {"separate": separate_columns(), "odd_offset_a": odd_offset_columns()[0], "odd_offset_b": odd_offset_columns()[1], "aliasing": aliasing_columns()}


@pytest.mark.parametrize("name", sorted(COLUMN_SETS))
def test_gather_columns_matches_numpy_on_every_range(S, name):
    """Every (word0, len) with word0 + len <= 40: len = 0, ranges inside one column, ranges that span three columns, the last word."""
    cols = COLUMN_SETS[name]
    flat = flat_of(cols)
    seen = set()
    for word0 in range(NCOLS * N + 1):
        for length in range(NCOLS * N - word0 + 1):
            got = S.gather_columns(cols, word0, length)
            assert np.array_equal(got, flat[word0:word0 + length]), (word0, length)
            if length:
                seen.add((word0 + length - 1) // N - word0 // N)
    assert {0, 2, 4} <= seen   # inside one column, three columns, all five
    assert S.gather_columns(cols, NCOLS * N - 1, 1)[0] == flat[-1]
    assert len(S.gather_columns(cols, NCOLS * N, 0)) == 0


def test_gather_columns_from_a_strided_2d_array(S):
    big = np.random.default_rng(1).integers(0, 2**64, size=(2 * NCOLS, N), dtype=np.uint64)
    for view in (big[::2], big[::-1], big[1::2][::-1], big[:NCOLS]):
        assert np.array_equal(S.gather_columns(view, 0, view.size), view.reshape(-1))
        assert np.array_equal(S.gather_columns(view, N - 1, N + 2), view.reshape(-1)[N - 1:2 * N + 1])
    ro = big[::2]
    ro.flags.writeable = False
    assert np.array_equal(S.gather_columns(ro, 3, 20), ro.reshape(-1)[3:23])


def test_column_table_is_built_once_and_keeps_the_columns_alive(S):
    cols = separate_columns(21)
    flat = flat_of(cols)
    table = S.ColumnTable(cols)
    assert len(table) == NCOLS and table.n == N
    assert [int(a) for a in table.addr] == [c.ctypes.data for c in cols]
    del cols
    assert np.array_equal(S.gather_columns(table, 0, NCOLS * N), flat)
    assert np.array_equal(S.gather_columns(table, 5, 20), flat[5:25])
    big = np.random.default_rng(2).integers(0, 2**64, size=(2 * NCOLS, N), dtype=np.uint64)
    t2 = S.ColumnTable(big[::-2])
    assert np.array_equal(S.gather_columns(t2, 0, NCOLS * N), big[::-2].reshape(-1))


def test_gather_columns_refusals(S):
    L = S.lib()
    cols = separate_columns()
    table = np.array([c.ctypes.data for c in cols], dtype=np.uint64)
    out = np.zeros(NCOLS * N + 8, dtype=np.uint64)
    tp, op = table.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.sbn_gather_columns(tp, NCOLS, N, 0, NCOLS * N, op) == 0
    # a range beyond the matrix
    for word0, length in ((0, NCOLS * N + 1), (NCOLS * N, 1), (NCOLS * N + 1, 0), (1, 2**64 - 1), (2**64 - 1, 2)):
        assert L.sbn_gather_columns(tp, NCOLS, N, word0, length, op) == BAD_ARG, (word0, length)
        assert b"beyond" in L.sbn_last_error()
    assert L.sbn_gather_columns(tp, 2**62, 2**62, 0, 1, op) == BAD_ARG   # n_columns * n overflows
    # a null column pointer, a misaligned one, a null table, a null destination
    bad = table.copy(); bad[3] = 0
    assert L.sbn_gather_columns(bad.ctypes.data_as(C.c_void_p), NCOLS, N, 0, 1, op) == BAD_ARG
    assert L.sbn_last_error() == b"column 3 is null or not 8-byte aligned"
    bad = table.copy(); bad[1] += 4
    assert L.sbn_gather_columns(bad.ctypes.data_as(C.c_void_p), NCOLS, N, 0, 1, op) == BAD_ARG
    assert L.sbn_last_error() == b"column 1 is null or not 8-byte aligned"
    assert L.sbn_gather_columns(None, NCOLS, N, 0, 1, op) == BAD_ARG
    assert L.sbn_gather_columns(tp, NCOLS, N, 0, 1, None) == BAD_ARG
    assert L.sbn_gather_columns(tp, NCOLS, N, 0, 0, None) == 0
    with pytest.raises(S.SbnError):
        S.gather_columns(cols, 39, 2)


def test_column_forms_that_would_need_a_copy_are_refused(S):
    cols = separate_columns()
    with pytest.raises(S.SbnError):
        S.gather_columns([c.astype(np.int64) for c in cols], 0, 1)
    with pytest.raises(S.SbnError):
        S.gather_columns(cols[:2] + [np.zeros(2 * N, dtype=np.uint64)[::2]], 0, 1)          # strided elements
    with pytest.raises(S.SbnError):
        S.gather_columns(cols[:2] + [np.zeros(N + 1, dtype=np.uint64)], 0, 1)               # another length
    with pytest.raises(S.SbnError):
        S.gather_columns(np.zeros((N, NCOLS), dtype=np.uint64).T, 0, 1)                    # rows not contiguous
    with pytest.raises(S.SbnError):
        S.gather_columns(np.zeros((NCOLS, N), dtype=np.uint32), 0, 1)


REDUCE_WORDS = [0, GL_P - 1, GL_P, GL_P + 1, 2**64 - 1]


def reduce_reference(w):
    p = np.uint64(GL_P)
    return np.where(w >= p, w - p, w), int(np.count_nonzero(w >= p))


def test_reduce_reference_on_the_named_words():
    want, changed = reduce_reference(np.array(REDUCE_WORDS, dtype=np.uint64))
    assert [int(x) for x in want] == [0, GL_P - 1, 0, 1, 2**32 - 2] and changed == 3


@pytest.mark.parametrize("count", [0, 1, 2, 3, 1025])
def test_reduce_words_host_matches_numpy(S, count):
    for shift in range(5):
        w = np.array([REDUCE_WORDS[(i + shift) % 5] for i in range(count)], dtype=np.uint64)
        want, changed = reduce_reference(w)
        assert S.reduce_words(w, on_device=False) == changed
        assert np.array_equal(w, want)
    w = np.random.default_rng(count).integers(0, 2**64, size=count, dtype=np.uint64)
    want, changed = reduce_reference(w)
    assert S.reduce_words(w, on_device=False) == changed and np.array_equal(w, want)


def test_reduce_words_arguments(S):
    L = S.lib()
    out = C.c_uint64(7)
    assert L.sbn_reduce_words(None, 4, 0, C.byref(out)) == BAD_ARG
    assert L.sbn_reduce_words(None, 0, 0, C.byref(out)) == 0 and out.value == 0
    w = np.array([2**64 - 1, 5], dtype=np.uint64)
    assert L.sbn_reduce_words(w.ctypes.data_as(C.c_void_p), 2, 0, None) == 0     # the count is optional
    assert [int(x) for x in w] == [2**32 - 2, 5]
    ro = np.zeros(4, dtype=np.uint64); ro.flags.writeable = False
    with pytest.raises(S.SbnError):
        S.reduce_words(ro, on_device=False)


def test_prove_host_columns_refuses_null_handles_without_a_device(S):
    """What the calls check before a prover exists (sbn_prover_create needs a device; the checks on a real prover -- column
    count, null and misaligned columns, unknown flags, public inputs -- are in test_host_columns_gpu.py)."""
    L = S.lib()
    cols = separate_columns()
    table = np.array([c.ctypes.data for c in cols], dtype=np.uint64)
    tp = table.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(1)
    assert L.sbn_prover_prove_host_columns(None, tp, NCOLS, 0, None, 0, None, C.byref(h)) == BAD_ARG
    assert L.sbn_prover_prove_host_columns(None, tp, NCOLS, 0, None, 0, None, None) == BAD_ARG
    assert L.sbn_batch_prover_prove_host_columns(None, tp, NCOLS, 0, None, 0, 1, C.byref(h)) == BAD_ARG
    g1 = S.G1Stark()
    assert L.sbn_prove_columns(C.byref(g1._d), C.byref(g1.config()._c), tp, NCOLS, 9, 0, None, 0, None) == BAD_ARG
    assert S.TRACE_REDUCE == 1
    assert {"sbn_prover_prove_host_columns", "sbn_prove_columns", "sbn_batch_prover_prove_host_columns", "sbn_gather_columns", "sbn_reduce_words"} <= set(S.EXPORTS)
