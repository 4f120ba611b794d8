"""A host trace held as separate columns on a real GPU: Prover.prove_host_columns (the gather into the upload ring, and with
reduce=True reduce_words_kernel in the scan's place), the one-shot prove_columns through the context cache, and
BatchProver.prove_host_traces.  The expected proof is always that of load_trace + prove on the flat canonical matrix, and for two
tables the oracle's digest in tests/golden/proof_digests.json."""
import ctypes as C
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GL_P = 0xFFFFFFFF00000001
NO_PI = np.zeros(0, dtype=np.uint64)
BAD_ARG, NON_CANONICAL, UNSUPPORTED = -1, -2, -7


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    return S


def reduce_reference(w):
    p = np.uint64(GL_P)
    return np.where(w >= p, w - p, w), int(np.count_nonzero(w >= p))


# ---- the kernel --------------------------------------------------------------------------------------------------------
def words_at_phase(count, lead, seed):
    """`count` canonical words as a slice that starts `lead` words into a fresh allocation: lead 0 and 1 are the two 8-byte
    phases of a 16-byte boundary, whatever the allocation's own alignment."""
    base = np.random.default_rng(seed).integers(0, GL_P, size=count + 1, dtype=np.uint64)
    return base[lead:lead + count]


def plant_indices(count):
    """Index 0, the last index, and two words of different workgroups (one workgroup covers 512 consecutive words of a grid pass;
    at the two large counts the second lies in a later pass of the grid-stride loop)."""
    idx = {0, count - 1}
    if count > 3 * 512:
        idx |= {123457, 2 * (1 << 20) + 3} if count > 2 * (1 << 20) + 3 else {700, count - 600}
    return sorted(idx)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("count", [1, 2, 3, 255, (1 << 20) + 1, 3 * (1 << 20) + 1])
def test_reduce_words_device_matches_numpy(gpu, count, lead):
    # all canonical: nothing changes, nothing is counted
    w = words_at_phase(count, lead, count)
    keep = w.copy()
    assert gpu.reduce_words(w, on_device=True) == 0
    assert np.array_equal(w, keep)
    # planted words, every non-canonical value class; the word just outside the slice is non-canonical too and must stay
    outside = w.base
    values = [GL_P, GL_P + 1, 2**64 - 1, GL_P + 5]
    idx = plant_indices(count)
    for k, i in enumerate(idx):
        w[i] = values[k % 4]
    outside[0 if lead else count] = 2**64 - 1
    want, changed = reduce_reference(w)
    assert changed == len(idx)
    assert gpu.reduce_words(w, on_device=True) == changed
    assert np.array_equal(w, want)
    assert outside[0 if lead else count] == 2**64 - 1
    # one word in a hundred, so that most waves count and several lanes of a wave change a vector
    w = words_at_phase(count, lead, 1000 + count)
    at = np.random.default_rng(7).random(count) < 0.01
    w[at] = (w[at] & np.uint64(0xFFFFFFF)) + np.uint64(GL_P)
    assert count < 200 or at.any()
    want, changed = reduce_reference(w)
    assert gpu.reduce_words(w, on_device=True) == changed
    assert np.array_equal(w, want)


# ---- the tables --------------------------------------------------------------------------------------------------------
def separate_columns(trace, seed=0):
    """Every column of `trace` as an allocation of its own, allocated in shuffled order."""
    cols = [None] * trace.shape[0]
    for c in np.random.default_rng(seed).permutation(trace.shape[0]):
        cols[c] = trace[c].copy()
    return cols


def two_step_proof(S, stark, trace, pi):
    q = S.Prover(stark, stark.config(), trace.shape[1].bit_length() - 1)
    try:
        q.load_trace(trace, pi)
        return q.prove().words
    finally:
        q.close()


def digest(words):
    return hashlib.sha256(np.ascontiguousarray(words, dtype="<u8").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def g1(gpu, g1op_case):
    trace = np.ascontiguousarray(g1op_case["trace"], dtype=np.uint64)
    return {"stark": gpu.G1Stark(), "trace": trace, "want": two_step_proof(gpu, gpu.G1Stark(), trace, NO_PI)}


def add_p(cols, n, idxs):
    """p added to the flat words idxs of the column list (in place): another 64-bit representative of the same element."""
    for i in idxs:
        c, r = divmod(i, n)
        assert int(cols[c][r]) < 2**64 - GL_P, (i, int(cols[c][r]))
        cols[c][r] += np.uint64(GL_P)


def plant_sets(ncols, n, chunk):
    """Flat word indices: word 0; the last word; the first word of the last (partial) chunk; both sides of a chunk seam; both
    sides of a column seam inside a chunk."""
    words = ncols * n
    nchunks = (ncols + chunk - 1) // chunk
    assert nchunks >= 3 and ncols % chunk, "the table must have several chunks and a partial last one"
    last0 = (nchunks - 1) * chunk * n
    seam = (nchunks // 2) * chunk * n
    col = (chunk + 5) * n
    return {"word0": [0], "last_word": [words - 1], "last_chunk_first": [last0], "chunk_seam": [seam - 1, seam], "column_seam": [col - 1, col]}


@pytest.mark.parametrize("reduce", [False, True])
def test_g1stark_columns_give_the_two_step_proof(gpu, golden, g1, reduce):
    S, stark, trace, want = gpu, g1["stark"], g1["trace"], g1["want"]
    cols = separate_columns(trace)

    def prove(p, columns):
        r = p.prove_host_columns(columns, NO_PI, reduce=reduce)
        if reduce:
            assert r[1] == 0
            return r[0]
        return r

    p = S.Prover(stark, stark.config(), 9)
    try:
        proof = prove(p, cols)
        assert np.array_equal(proof.words, want)
        assert hashlib.sha256(proof.to_bytes()).hexdigest() == golden["proof_digests"]["g1op_rows512_seed0"]["proof_sha256"]
        assert np.array_equal(p.prove().words, want)          # the trace is resident as after load_trace
        assert np.array_equal(p.read_trace(), trace)
        assert p.check_trace().ok
        for a in cols:
            a.flags.writeable = False
        assert np.array_equal(prove(p, cols).words, want)     # read-only arrays; the ring and the events are reused
        rev = np.ascontiguousarray(trace[::-1])
        view = rev[::-1]                                      # the trace again, rows contiguous, a negative stride between them
        assert view.strides[0] < 0 and np.array_equal(view, trace)
        assert np.array_equal(prove(p, view).words, want)
        assert np.array_equal(prove(p, trace).words, want)    # and the flat matrix itself
        table = S.ColumnTable(cols)                           # the pointer table built once, for several calls
        assert np.array_equal(prove(p, table).words, want) and np.array_equal(prove(p, table).words, want)
        wide = np.zeros((2 * trace.shape[0], trace.shape[1]), dtype=np.uint64)
        wide[::2] = trace
        assert np.array_equal(prove(p, wide[::2]).words, want)
        alias = list(cols); alias[7] = alias[3]               # two entries the same pointer: the trace whose column 7 is column 3
        t2 = trace.copy(); t2[7] = t2[3]
        assert np.array_equal(prove(p, alias).words, two_step_proof(S, stark, t2, NO_PI))
        assert np.array_equal(p.read_trace(), t2)
    finally:
        p.close()


def test_g1stark_non_canonical_words_are_reduced_or_refused(gpu, g1):
    S, stark, trace, want = gpu, g1["stark"], g1["trace"], g1["want"]
    ncols, n = trace.shape
    p = S.Prover(stark, stark.config(), 9)
    try:
        chunk = int(p.describe()["ntt_chunk"])
        sets = plant_sets(ncols, n, chunk)
        sets["all"] = sorted(i for idxs in list(sets.values()) for i in idxs)
        for label, idxs in sets.items():
            cols = separate_columns(trace, 1)
            add_p(cols, n, idxs)
            proof, reduced = p.prove_host_columns(cols, NO_PI, reduce=True)
            assert reduced == len(idxs), label
            assert np.array_equal(proof.words, want), label
            assert np.array_equal(p.read_trace(), trace), label      # resident in canonical form
            assert np.array_equal(p.prove().words, want), label
            with pytest.raises(S.SbnError) as e:
                p.prove_host_columns(cols, NO_PI)
            assert e.value.code == NON_CANONICAL, label
            assert str(e.value) == f"sbn error -2: trace word {min(idxs)} is not canonical", label
            with pytest.raises(S.SbnError) as e_prove:
                p.prove()
            assert e_prove.value.code == BAD_ARG and "no trace loaded" in str(e_prove.value), label
            with pytest.raises(S.SbnError):
                p.read_trace()
            assert np.array_equal(p.prove_host_columns(separate_columns(trace, 2), NO_PI).words, want), label   # the next clean call proves
    finally:
        p.close()


def test_prove_host_columns_argument_checks(gpu, g1):
    """The refusals in front of any device work, in the header's order, on a prover that holds a trace: each leaves none loaded."""
    S, stark, trace, want = gpu, g1["stark"], g1["trace"], g1["want"]
    L = S.lib()
    ncols = trace.shape[0]
    cols = separate_columns(trace, 3)
    table = np.array([c.ctypes.data for c in cols], dtype=np.uint64)
    p = S.Prover(stark, stark.config(), 9)

    def call(tab, n_columns, flags, pi, n_pi):
        assert np.array_equal(p.prove_host_columns(cols, NO_PI).words, want)
        h, red = C.c_void_p(1), C.c_uint64(9)
        rc = L.sbn_prover_prove_host_columns(p._h, tab.ctypes.data_as(C.c_void_p) if tab is not None else None, n_columns, flags,
                                             pi.ctypes.data_as(C.c_void_p) if pi is not None else None, n_pi, C.byref(red), C.byref(h))
        msg = L.sbn_last_error().decode()
        assert h.value is None and red.value == 0
        with pytest.raises(S.SbnError) as e:
            p.prove()
        assert "no trace loaded" in str(e.value)
        return rc, msg

    try:
        assert call(table, ncols - 1, 0, None, 0) == (BAD_ARG, f"expected {ncols} columns, got {ncols - 1}")
        assert call(None, ncols, 0, None, 0)[0] == BAD_ARG
        bad = table.copy(); bad[17] = 0; bad[40] = 0
        assert call(bad, ncols, 0, None, 0) == (BAD_ARG, "column 17 is null or not 8-byte aligned")
        bad = table.copy(); bad[ncols - 1] += 4
        assert call(bad, ncols, 0, None, 0) == (BAD_ARG, f"column {ncols - 1} is null or not 8-byte aligned")
        assert call(table, ncols, 2, None, 0) == (BAD_ARG, "unknown flag bits 0x2")
        assert call(table, ncols, 0x80000001, None, 0)[0] == BAD_ARG
        one = np.array([5], dtype=np.uint64)
        assert call(table, ncols, 0, one, 1) == (BAD_ARG, "expected 0 public inputs, got 1")
        assert call(table, ncols, 1, one, 1) == (BAD_ARG, "expected 0 public inputs, got 1")
        h = C.c_void_p()
        assert L.sbn_prover_prove_host_columns(p._h, table.ctypes.data_as(C.c_void_p), ncols, 0, None, 0, None, None) == BAD_ARG
        assert L.sbn_prover_prove_host_columns(p._h, table.ctypes.data_as(C.c_void_p), ncols, 0, None, 0, None, C.byref(h)) == 0   # reduced_out is optional
        L.sbn_proof_free(h)
        with pytest.raises(S.SbnError):
            p.prove_host_columns(cols[:-1], NO_PI)
    finally:
        p.close()


def test_lookupstark_columns_take_the_single_upload_branch(gpu, O):
    """4 columns: commit_pipeline uploads the whole matrix as one chunk (ncols <= 4)."""
    S = gpu
    stark = S.LookupStark()
    ins, tab = O.lookup_inputs(512, 9)
    trace = stark.generate_trace(ins, tab)
    want = two_step_proof(S, stark, trace, NO_PI)
    p = S.Prover(stark, stark.config(), 9)
    try:
        assert np.array_equal(p.prove_host_columns(separate_columns(trace), NO_PI).words, want)
        proof, reduced = p.prove_host_columns(separate_columns(trace), NO_PI, reduce=True)
        assert reduced == 0 and np.array_equal(proof.words, want)
        cols = separate_columns(trace)
        idxs = [0, 511, 512, 4 * 512 - 1]
        add_p(cols, 512, idxs)
        proof, reduced = p.prove_host_columns(cols, NO_PI, reduce=True)
        assert reduced == 4 and np.array_equal(proof.words, want)
        assert np.array_equal(p.read_trace(), trace)
        cols[0][0] -= np.uint64(GL_P)
        with pytest.raises(S.SbnError) as e:
            p.prove_host_columns(cols, NO_PI)
        assert str(e.value) == "sbn error -2: trace word 511 is not canonical"
    finally:
        p.close()


def test_g1expstark_columns_across_ring_pieces(gpu, golden, g1exp_case):
    """G1ExpStark(128): 1676 columns of 2^16 rows cross in 52 ring pieces of 32 columns; p is added on both sides of the seam of
    the first two pieces, flat word 2^21 (the last row of column 31, the first of column 32)."""
    S = gpu
    stark = S.G1ExpStark(128)
    trace, pi = g1exp_case["trace"], g1exp_case["pi"]
    cols = separate_columns(trace)
    n = trace.shape[1]
    assert n == 1 << 16
    add_p(cols, n, [(1 << 21) - 1, 1 << 21])
    p = S.Prover(stark, stark.config(), 16)
    try:
        proof, reduced = p.prove_host_columns(cols, pi, reduce=True)
        assert reduced == 2
        assert hashlib.sha256(proof.to_bytes()).hexdigest() == golden["proof_digests"]["g1exp_io128_seed1"]["proof_sha256"]
        with pytest.raises(S.SbnError) as e:
            p.prove_host_columns(cols, pi)
        assert str(e.value) == f"sbn error -2: trace word {(1 << 21) - 1} is not canonical"
    finally:
        p.close()


def test_lookupstark_2pow22_rows_a_column_longer_than_a_ring_piece(gpu, O):
    """LookupStark at 2^22 rows: every column is two ring pieces long, so a piece is a range inside one column.  The slow case of
    this file: nearly all of its time is the host witness of 2^22 rows."""
    S = gpu
    stark = S.LookupStark()
    ins, tab = O.lookup_inputs(1 << 22, 222)
    trace = stark.generate_trace(ins, tab)
    p = S.Prover(stark, stark.config(), 22)
    try:
        want = p.prove_host_trace(trace, NO_PI).words
        cols = separate_columns(trace)
        del trace
        assert np.array_equal(p.prove_host_columns(cols, NO_PI).words, want)
    finally:
        p.close()


def test_prove_columns_goes_through_the_context_cache(gpu, g1):
    S, stark, trace = gpu, g1["stark"], g1["trace"]
    cfg = stark.config()
    cols = separate_columns(trace)
    S.prove_cache_configure(0)
    try:
        want = S.prove(stark, cfg, trace, NO_PI).words
        assert np.array_equal(want, g1["want"])
        S.prove_cache_configure(1 << 40)
        s0 = S.prove_cache_stats()
        assert np.array_equal(S.prove_columns(stark, cfg, cols, NO_PI).words, want)
        s1 = S.prove_cache_stats()
        assert (s1["hits"] - s0["hits"], s1["misses"] - s0["misses"], s1["contexts_resident"]) == (0, 1, 1)
        assert np.array_equal(S.prove_columns(stark, cfg, cols, NO_PI, reduce=True).words, want)
        s2 = S.prove_cache_stats()
        assert (s2["hits"] - s1["hits"], s2["misses"] - s1["misses"], s2["contexts_resident"]) == (1, 0, 1)
        assert np.array_equal(S.prove(stark, cfg, trace, NO_PI).words, want)     # the same key as the flat call: a hit
        assert S.prove_cache_stats()["hits"] - s2["hits"] == 1
        bad = separate_columns(trace, 4)
        add_p(bad, trace.shape[1], [5 * trace.shape[1] + 7])
        with pytest.raises(S.SbnError) as e:
            S.prove_columns(stark, cfg, bad, NO_PI)
        assert e.value.code == NON_CANONICAL and f"trace word {5 * trace.shape[1] + 7} is not canonical" in str(e.value)
        assert S.prove_cache_stats()["contexts_resident"] == 0                  # a context whose call failed is not kept
        assert np.array_equal(S.prove_columns(stark, cfg, bad, NO_PI, reduce=True).words, want)
    finally:
        S.prove_cache_configure(0)


# ---- the batch ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1_units(gpu, O, g1):
    """5 G1Stark traces from 5 seeds with their two-step proofs: a unit mix-up cannot pass."""
    units = [(g1["trace"], g1["want"])]
    for seed in (11, 12, 13, 14):
        pts, _ = O.g1op_inputs(512, seed)
        trace = O.g1op_trace(pts)
        units.append((trace, two_step_proof(gpu, g1["stark"], trace, NO_PI)))
    assert len({digest(w) for _, w in units}) == 5
    return units


@pytest.mark.parametrize("inflight", [2, 3])
def test_batch_prover_proves_host_traces(gpu, g1, g1_units, inflight):
    S, stark = gpu, g1["stark"]
    L = S.lib()
    n = 512
    b = S.BatchProver(stark, stark.config(), 9, inflight=inflight)
    try:
        units = [separate_columns(t, k) for k, (t, _) in enumerate(g1_units)]
        pis = [NO_PI] * 5
        for reduce in (False, True):
            proofs = b.prove_host_traces(units, pis, reduce=reduce)
            assert len(proofs) == 5
            for k, pr in enumerate(proofs):
                assert np.array_equal(pr.words, g1_units[k][1]), (reduce, k)
        # unit 3 holds a non-canonical word: without reduce the call fails on it, every proof slot is null, the batch prover lives on
        bad = list(units)
        bad[3] = separate_columns(g1_units[3][0], 9)
        where = 100 * n + 17
        add_p(bad[3], n, [where])
        with pytest.raises(S.SbnError) as e:
            b.prove_host_traces(bad, pis)
        assert e.value.code == NON_CANONICAL
        assert str(e.value) == f"sbn error -2: unit 3: trace word {where} is not canonical"
        addr = np.concatenate([np.array([c.ctypes.data for c in u], dtype=np.uint64) for u in bad])
        out = (C.c_void_p * 5)(*([1] * 5))
        rc = L.sbn_batch_prover_prove_host_columns(b._h, addr.ctypes.data_as(C.c_void_p), stark.num_columns, 0, None, 0, 5, out)
        assert rc == NON_CANONICAL and L.sbn_last_error().startswith(b"unit 3: ")
        assert all(out[i] is None for i in range(5))
        proofs = b.prove_host_traces(bad, pis, reduce=True)
        assert [digest(pr.words) for pr in proofs] == [digest(w) for _, w in g1_units]
        proofs = b.prove_host_traces(units, pis)
        assert [digest(pr.words) for pr in proofs] == [digest(w) for _, w in g1_units]
        assert b.prove_host_traces([], []) == []
    finally:
        b.close()


def test_batch_prover_proves_host_traces_of_an_exp_table(gpu, fq12exp_case):
    """Fq12ExpStark(16), 2 units with public inputs; the second unit's public inputs hold a word >= p, reduced on the host."""
    S = gpu
    stark = S.Fq12ExpStark(16)
    trace, pi = np.ascontiguousarray(fq12exp_case["trace"], dtype=np.uint64), np.ascontiguousarray(fq12exp_case["pi"], dtype=np.uint64)
    want = two_step_proof(S, stark, trace, pi)
    units = [separate_columns(trace, 0), separate_columns(trace, 1)]
    b = S.BatchProver(stark, stark.config(), 13, inflight=2)
    try:
        proofs = b.prove_host_traces(units, [pi, pi])
        assert all(np.array_equal(pr.words, want) for pr in proofs) and len(proofs) == 2
        k = int(np.argmax(pi < np.uint64(2**64 - GL_P)))
        pi2 = pi.copy(); pi2[k] += np.uint64(GL_P)
        with pytest.raises(S.SbnError) as e:
            b.prove_host_traces(units, [pi, pi2])
        assert str(e.value) == f"sbn error -2: unit 1: public input {k} is not canonical"
        proofs = b.prove_host_traces(units, [pi, pi2], reduce=True)
        assert all(np.array_equal(pr.words, want) for pr in proofs) and len(proofs) == 2
    finally:
        b.close()


def test_split_prover_refuses_host_columns(gpu, fq12exp_case):
    """A split prover at local world 1: SBN_ERR_UNSUPPORTED, as sbn_prover_prove_host_trace.  The split handle has no call of its
    own for host traces, so the test reaches the prover context it wraps (the handle's first word, csrc/prover.hip
    sbn_split_prover); the refusal is that of csrc/trace_load.hip sbn_prover_prove_host_columns."""
    from starky_bn254_amd import split
    S = gpu
    L = S.lib()
    stark = S.Fq12ExpStark(16)
    cfg = stark.config()
    trace, pi = np.ascontiguousarray(fq12exp_case["trace"], dtype=np.uint64), np.ascontiguousarray(fq12exp_case["pi"], dtype=np.uint64)
    sb, rb = split.exchange_bytes(stark, cfg, 13, 1)
    grp = split.LocalGroup(1, sb, rb)
    sp = split.SplitProver(stark, cfg, 13, transport=grp.comms[0])
    try:
        inner = C.c_void_p.from_address(sp._h.value)
        table = (trace.ctypes.data + np.arange(trace.shape[0], dtype=np.int64) * trace.strides[0]).astype(np.uint64)
        h = C.c_void_p(1)
        for flags in (0, 1):
            rc = L.sbn_prover_prove_host_columns(inner, table.ctypes.data_as(C.c_void_p), trace.shape[0], flags, pi.ctypes.data_as(C.c_void_p), len(pi), None, C.byref(h))
            assert rc == UNSUPPORTED and h.value is None
            assert L.sbn_last_error() == b"sbn_prover_prove_host_columns covers single-GPU provers"
    finally:
        sp.close()
        grp.close()
