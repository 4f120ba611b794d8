"""Row-major traces on a real GPU: Prover.load_trace_rows / load_trace_rows_device / prove_host_rows and the one-shot prove_rows.
Whole-row mode: read_trace() is the oracle's trace and the proof words are those of load_trace + prove on the same prover.
Main-row mode: trace, public inputs and proof words are those of generate_trace(ios) + prove() on the same prover (and, where a
session fixture holds it, the oracle's trace).  The rows handed in are trace.T or trace[:num_main].T, made contiguous."""
import ctypes as C
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GL_P = 0xFFFFFFFF00000001
NO_PI = np.zeros(0, dtype=np.uint64)
BAD_ARG, NON_CANONICAL, UNSUPPORTED, WITNESS = -1, -2, -7, -8


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    return S


def main_rows(stark, trace):
    return np.ascontiguousarray(trace[:stark.num_main_columns].T)


JUNK = 0x5EEDF00D5EED   # a canonical word no trace of these tables holds (their words are limbs, flags, inverses of small numbers)


def overwrite_trace(prover, trace, pi):
    """Fills the prover's trace buffer with JUNK through load_trace, so that a row load which writes nothing, or not everything,
    leaves words behind that differ from the expected trace in every place."""
    assert not np.any(trace == np.uint64(JUNK))
    prover.load_trace(np.full(trace.shape, JUNK, dtype=np.uint64), pi)


# ---- whole-row mode ------------------------------------------------------------------------------------------------------
def whole_case(S, O, request, name):
    if name == "lookup":       # 4 columns: less than one tile of the transposition
        ins, tab = O.lookup_inputs(512, 9)
        return S.LookupStark(), 9, O.lookup_trace(ins, tab)
    if name == "flags8":       # 49 columns: one ragged tile
        limbs, _ = O.flags_inputs(8, 8)
        return S.FlagStark(8), 12, O.flags_trace(limbs)
    return S.G1Stark(), 9, request.getfixturevalue("g1op_case")["trace"]   # 2,283 columns: a ragged last tile, fewer rows than one ring piece


@pytest.mark.parametrize("name", ["lookup", "flags8", "g1", "g1_padded"])
def test_whole_rows_load_the_oracle_trace_and_prove_to_the_same_words(gpu, O, request, name):
    S = gpu
    stark, bits, trace = whole_case(S, O, request, name)
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    assert trace.shape == (stark.num_columns, 1 << bits)
    rows = np.ascontiguousarray(trace.T)
    if name == "g1_padded":    # a stride of n_cols + 3, the padding full of words that would be refused
        wide = np.full((rows.shape[0], rows.shape[1] + 3), 2**64 - 1, dtype=np.uint64)
        wide[:, :rows.shape[1]] = rows
        rows = wide[:, :trace.shape[0]]
    p = S.Prover(stark, stark.config(), bits)
    try:
        p.load_trace(trace, NO_PI)
        want = p.prove().words
        overwrite_trace(p, trace, NO_PI)
        p.load_trace_rows(rows, NO_PI)
        assert np.array_equal(p.read_trace(), trace)
        assert np.array_equal(p.prove().words, want)
        if name == "g1":       # the pointer form: one allocation per row
            overwrite_trace(p, trace, NO_PI)
            p.load_trace_rows([rows[r].copy() for r in range(rows.shape[0])], NO_PI)
            assert np.array_equal(p.read_trace(), trace)
            assert np.array_equal(p.prove().words, want)
    finally:
        p.close()


# ---- main-row mode -------------------------------------------------------------------------------------------------------
MAIN_CASES = {   # class, num_io, degree_bits, fixture (or the seed of fresh inputs), golden key
    "fq12expu64": ("Fq12ExpU64Stark", 16, 11, "fq12expu64_case", None),          # the split range check
    "fqexp128": ("FqExpStark", 128, 16, "fqexp_case", None),                     # the u16 range check, LDS histograms
    "fqexp256": ("FqExpStark", 256, 17, 41, None),                               # 2^17 rows: the histogram scratch carved in this path
    "g1exp": ("G1ExpStark", 128, 16, "g1exp_case", "g1exp_io128_seed1"),         # 209 MB of rows: several ring pieces
}


@pytest.mark.parametrize("name", sorted(MAIN_CASES))
def test_main_rows_give_the_trace_and_proof_of_generate_trace(gpu, O, golden, request, name):
    S = gpu
    cls, num_io, bits, source, key = MAIN_CASES[name]
    stark = getattr(S, cls)(num_io)
    if isinstance(source, str):
        case = request.getfixturevalue(source)
        ios, oracle_trace = case["ios"], case["trace"]
    else:
        ios, oracle_trace = O.fqexp_inputs(num_io, source)[0], None
    p = S.Prover(stark, stark.config(), bits)
    try:
        pi = p.generate_trace(ios)
        trace = p.read_trace()
        if oracle_trace is not None:
            assert np.array_equal(trace, oracle_trace) and np.array_equal(pi, case["pi"])
        want = p.prove().words
        rows = main_rows(stark, trace)
        assert rows.shape == (1 << bits, stark.num_main_columns)
        if name == "g1exp":
            assert rows.size > 4 * (2 << 20)       # more than four 16 MiB slots: the ring goes round
        overwrite_trace(p, trace, pi)              # main and derived columns alike: every word must come from this load
        p.load_trace_rows(rows, pi)
        got = p.read_trace()
        assert np.array_equal(got, trace)
        del got
        proof = p.prove()
        assert np.array_equal(proof.words, want)
        if key:
            assert hashlib.sha256(proof.to_bytes()).hexdigest() == golden["proof_digests"][key]["proof_sha256"]
            f0, f1 = S.api.fixed_columns_range(stark)
            assert int(p.describe()["fixed_columns_skipped"]) == f1 - f0     # as after generate_trace: the derived columns are the generators'
            assert p.check_trace().ok
    finally:
        p.close()


# ---- data errors -----------------------------------------------------------------------------------------------------------
def test_data_errors_name_row_and_column_and_leave_nothing_loaded(gpu, fq12expu64_case, g1op_case):
    S = gpu
    stark = S.Fq12ExpU64Stark(16)
    trace, pi = fq12expu64_case["trace"], fq12expu64_case["pi"]
    rows = main_rows(stark, trace)
    p = S.Prover(stark, stark.config(), 11)
    try:
        p.load_trace_rows(rows, pi)
        want = p.prove().words

        def refused(bad, code, text, **kw):
            with pytest.raises(S.SbnError) as e:
                p.load_trace_rows(bad, pi, **kw)
            assert e.value.code == code and text in str(e.value), str(e.value)
            with pytest.raises(S.SbnError) as e:
                p.prove()
            assert e.value.code == BAD_ARG and "no trace loaded" in str(e.value)
            with pytest.raises(S.SbnError):
                p.read_trace()
            p.load_trace_rows(rows, pi)
            assert np.array_equal(p.prove().words, want)

        for planted in ([(1000, 1733)], [(65, 63), (64, 64)], [(0, 0)], [(2047, 1733), (2047, 1732)]):
            bad = rows.copy()
            for r, c in planted:
                bad[r, c] += np.uint64(GL_P)
            first = min(planted)
            refused(bad, NON_CANONICAL, f"row {first[0]}, column {first[1]} ")
            overwrite_trace(p, trace, pi)
            assert p.load_trace_rows(bad, pi, reduce=True) == len(planted)
            assert np.array_equal(p.read_trace(), trace)
            assert np.array_equal(p.prove().words, want)
        bad = rows.copy()
        bad[777, 500] = 65536
        refused(bad, WITNESS, "row 777, column 500")
        bad[777, 500] = np.uint64(GL_P + 65536)     # reduced first, then out of range all the same
        refused(bad, WITNESS, "row 777, column 500", reduce=True)
        refused(bad, NON_CANONICAL, "row 777, column 500 ")
    finally:
        p.close()
    # whole-row mode, the last word of the ragged last tile
    g1, tr = S.G1Stark(), np.ascontiguousarray(g1op_case["trace"], dtype=np.uint64)
    rows = np.ascontiguousarray(tr.T)
    rows[511, 2282] += np.uint64(GL_P)
    q = S.Prover(g1, g1.config(), 9)
    try:
        with pytest.raises(S.SbnError) as e:
            q.load_trace_rows(rows, NO_PI)
        assert e.value.code == NON_CANONICAL and "row 511, column 2282 " in str(e.value)
        overwrite_trace(q, tr, NO_PI)
        assert q.load_trace_rows(rows, NO_PI, reduce=True) == 1
        assert np.array_equal(q.read_trace(), tr)
    finally:
        q.close()


# ---- rows already in device memory ------------------------------------------------------------------------------------------
def test_rows_in_a_torch_tensor_on_the_device():
    """The device-pointer form on memory the library did not allocate: a torch tensor.  In a fresh process (the test is about that
    process: tests/host_rows_torch_worker.py says why torch has to come first in it)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "host_rows_torch_worker.py")], env=dict(os.environ, PYTHONPATH=root),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "torch rows ok" in out, (out[-2000:], err[-4000:])


# ---- the other entry points ----------------------------------------------------------------------------------------------
def test_one_call_forms_and_compact_storage(gpu, fq12expu64_case):
    S = gpu
    stark = S.Fq12ExpU64Stark(16)
    cfg = stark.config()
    trace, pi = fq12expu64_case["trace"], fq12expu64_case["pi"]
    rows = main_rows(stark, trace)
    p = S.Prover(stark, cfg, 11)
    try:
        p.load_trace(trace, pi)
        want = p.prove().words
        # load and prove in one call, and the one-shot call through the context cache
        overwrite_trace(p, trace, pi)
        assert np.array_equal(p.prove_host_rows(rows, pi).words, want)
        assert np.array_equal(p.read_trace(), trace)
        overwrite_trace(p, trace, pi)
        proof, changed = p.prove_host_rows(rows, pi, reduce=True)
        assert changed == 0 and np.array_equal(proof.words, want)
        assert np.array_equal(p.prove().words, want)
        assert np.array_equal(S.prove_rows(stark, cfg, rows, pi).words, want)
        assert np.array_equal(S.prove_rows(stark, cfg, np.ascontiguousarray(trace.T), pi).words, want)
    finally:
        p.close()
    # a compact rate-3 context takes the call like a full one
    cfg3 = S.StarkConfig.for_rate(3)
    full, compact = S.Prover(stark, cfg3, 11), S.Prover(stark, cfg3, 11, lde="compact")
    try:
        words = []
        for q in (full, compact):
            q.load_trace_rows(rows, pi)
            assert np.array_equal(q.read_trace(), trace)
            words.append(q.prove().words)
        assert np.array_equal(words[0], words[1])
        full.load_trace(trace, pi)
        assert np.array_equal(full.prove().words, words[0])
    finally:
        full.close()
        compact.close()


def test_refusals_on_a_real_prover(gpu, fq12expu64_case, g1op_case):
    from starky_bn254_amd import split
    S = gpu
    L = S.lib()
    stark = S.Fq12ExpU64Stark(16)
    cfg = stark.config()
    trace, pi = fq12expu64_case["trace"], np.ascontiguousarray(fq12expu64_case["pi"], dtype=np.uint64)
    rows = main_rows(stark, trace)
    n, nc = rows.shape

    def raw(handle, flat, stride, n_rows, n_cols, flags=0):
        r = S.api._HostRows(C.sizeof(S.api._HostRows), 0, flat, stride, None, n_rows, n_cols)
        return L.sbn_prover_load_trace_rows(handle, C.byref(r), flags, pi.ctypes.data_as(C.c_void_p), len(pi), None)

    p = S.Prover(stark, cfg, 11)
    try:
        p.load_trace_rows(rows, pi)
        assert raw(p._h, rows.ctypes.data, nc, n, nc - 1) == BAD_ARG            # a bad n_cols
        with pytest.raises(S.SbnError):
            p.prove()                                                           # and the trace of the call before is gone
        assert raw(p._h, rows.ctypes.data, nc - 1, n, nc) == BAD_ARG            # a short stride
        assert raw(p._h, rows.ctypes.data, nc, n, nc, flags=2) == BAD_ARG       # an unknown flag
        assert raw(p._h, rows.ctypes.data, nc, n // 2, nc) == BAD_ARG
        assert L.sbn_prover_load_trace_rows_device(p._h, None, nc, nc, 0, pi.ctypes.data_as(C.c_void_p), len(pi), None) == BAD_ARG
        assert raw(p._h, rows.ctypes.data, nc, n, nc) == 0
    finally:
        p.close()
    # main-row mode on a table it does not cover
    g1 = S.G1Stark()
    q = S.Prover(g1, g1.config(), 9)
    try:
        r = S.api._HostRows(C.sizeof(S.api._HostRows), 0, rows.ctypes.data, 386, None, 512, 386)
        assert L.sbn_prover_load_trace_rows(q._h, C.byref(r), 0, None, 0, None) == UNSUPPORTED
    finally:
        q.close()
    # a split prover at local world 1 (the handle's first word is the prover context it wraps); refused in front of any read
    st13 = S.Fq12ExpStark(16)
    zeros, pi13 = np.zeros((1 << 13, st13.num_main_columns), dtype=np.uint64), np.zeros(st13.num_public_inputs, dtype=np.uint64)
    sb, rb = split.exchange_bytes(st13, cfg, 13, 1)
    grp = split.LocalGroup(1, sb, rb)
    sp = split.SplitProver(st13, cfg, 13, transport=grp.comms[0])
    try:
        inner = C.c_void_p.from_address(sp._h.value)
        r = S.api._HostRows(C.sizeof(S.api._HostRows), 0, zeros.ctypes.data, zeros.shape[1], None, 1 << 13, zeros.shape[1])
        assert L.sbn_prover_load_trace_rows(inner, C.byref(r), 0, pi13.ctypes.data_as(C.c_void_p), len(pi13), None) == UNSUPPORTED
        assert L.sbn_last_error() == b"row-major loads cover single-GPU provers"
    finally:
        sp.close()
        grp.close()


# ---- every intake path in turn on one prover ---------------------------------------------------------------------------------
def test_intake_paths_alternate_on_one_prover(gpu, fq12expu64_case):
    """All the calls that make a trace resident share one pinned ring, one copy stream and its events (csrc/trace_load.hip).  On
    Fq12ExpU64Stark(16) -- 2^11 rows x 9,792 columns, 160 MB: the smallest table at which both upload forms go round the ring (one
    piece per 64-column chunk for the column forms; more than four 16 MiB pieces of whole rows, so the row form reuses all four
    slots and both staging buffers) -- six loads of the same trace through five entry points give the same proof words, with a
    refused prove_host_trace in the middle that must leave nothing provable and the ring and events usable."""
    S = gpu
    stark = S.Fq12ExpU64Stark(16)
    trace = np.ascontiguousarray(fq12expu64_case["trace"], dtype=np.uint64)
    pi = fq12expu64_case["pi"]
    n, ncols = 1 << 11, stark.num_columns
    assert trace.shape == (ncols, n)
    assert n * ncols > 4 * (1 << 21)                # more than four ring slots of whole rows ...
    assert (ncols + 63) // 64 > 4                   # ... and more than four column chunks
    rows = np.ascontiguousarray(trace.T)
    p = S.Prover(stark, stark.config(), 11)
    try:
        words = [p.prove_host_rows(rows, pi).words]                               # whole rows, flat
        words.append(p.prove_host_trace(trace, pi).words)
        p.load_trace_rows([rows[r] for r in range(n)], pi)                        # whole rows, one pointer per row
        words.append(p.prove().words)
        # a refused call in the middle: one word = p in a late chunk, found by the device scan behind the upload
        col, row = 5000, 1234
        bad = trace.copy()
        bad[col, row] = GL_P
        with pytest.raises(S.SbnError) as e:
            p.prove_host_trace(bad, pi)
        assert e.value.code == NON_CANONICAL and f"trace word {col * n + row} is not canonical" in str(e.value), str(e.value)
        del bad
        with pytest.raises(S.SbnError) as e:
            p.prove()
        assert "no trace loaded" in str(e.value)
        proof, reduced = p.prove_host_columns(trace, pi, reduce=True)             # (a 2-D array: its rows are the columns)
        assert reduced == 0
        words.append(proof.words)
        p.load_trace(trace, pi)
        words.append(p.prove().words)
        words.append(p.prove_host_rows(rows, pi).words)
        assert len(words) == 6
        for k in range(1, 6):
            assert np.array_equal(words[k], words[0]), k
    finally:
        p.close()
