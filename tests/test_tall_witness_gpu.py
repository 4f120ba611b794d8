"""Device witness generation of the u16-range-check tables (G1ExpStark, G2ExpStark, FqExpStark) above 2^18 rows: 1,024 instances
(2^19 rows) and, on Fq, 2,048 (2^20 rows).  Everything here is compared for equality with the host generators and the host
derivations of the instance lists (chain_instances, msm_batch_instances, trace_from_rows_host, diff_witness_host): no tolerance.

What is new above 2^18 rows (csrc/kernels_tracegen.cuh): the prefix counts of the range check cross a multiple of 2^16 up to 7
(2^19 rows) or 15 (2^20) times instead of 3, more than 1,024 values of a column can have more than 256 occurrences, and a chained
or segmented list no longer fits the 512 lanes of one scan workgroup (blocks of 512: heads around 511 | 512 | 513)."""
import ctypes as C
import functools

import numpy as np
import pytest

import tracegen_edges as T

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED, WITNESS = -1, -7, -8
BLOCK = 512          # instances per block of the device scan (tg::CS_LANES)


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    return S


def make(gpu, O, table, num_io, seed):
    inputs = {"g1": O.g1exp_inputs, "g2": O.g2exp_inputs, "fq": O.fqexp_inputs}[table]
    ios, _ = inputs(num_io, seed)
    stark = T.stark_class(gpu, table)(num_io)
    return stark, stark.config(), T.degree_bits(table, num_io), ios


# ---- the device trace against a host one in column blocks: the device side is never whole in host memory ---------------------------
@functools.lru_cache(maxsize=None)
def _hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemcpy.restype = C.c_int
    return h


def differing_columns(prover, want, block=256):
    """Columns in which the prover's resident trace differs from `want` ([columns][n] uint64), read `block` columns at a time."""
    cols, n = want.shape
    assert cols == prover.stark.num_columns and n == 1 << prover.degree_bits
    base = prover.trace_device_ptr()
    assert base
    buf = np.empty((block, n), dtype=np.uint64)
    bad = []
    for c0 in range(0, cols, block):
        k = min(block, cols - c0)
        assert _hip().hipMemcpy(buf.ctypes.data, base + 8 * n * c0, 8 * n * k, 2) == 0   # hipMemcpyDeviceToHost
        bad += [c0 + int(i) for i in np.nonzero((buf[:k] != want[c0:c0 + k]).any(axis=1))[0]]
    return bad


def mostly_one_value(ios, e0):
    """The variant of test_device_witness_above_2pow16_rows: every exponent 0 but one that is all ones."""
    ios = ios.copy()
    ios[:, e0:e0 + 8] = 0
    ios[3, e0:e0 + 8] = 0xFFFFFFFF
    return ios


# ---- a. explicit lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,num_io", [("g1", 1024), ("fq", 1024), ("g2", 1024), ("fq", 2048)])
def test_explicit_list_equals_the_host_generator(gpu, O, table, num_io):
    """generate_trace(ios) == stark.generate_trace_and_public_inputs(ios), public inputs and every column, on random instances
    and on instances whose range-checked columns are mostly one value.  FqExpStark(1024) also passes check_trace, proves and
    verifies."""
    stark, cfg, bits, ios = make(gpu, O, table, num_io, 40 + num_io // 1024)
    e0 = {"g1": 32, "g2": 64, "fq": 16}[table]
    prover = gpu.Prover(stark, cfg, bits)
    try:
        for variant, lst in enumerate((ios, mostly_one_value(ios, e0))):
            pi = prover.generate_trace(lst)
            t_host, pi_host = stark.generate_trace_and_public_inputs(lst)
            assert np.array_equal(pi, pi_host), variant
            bad = differing_columns(prover, t_host)
            assert not bad, f"variant {variant}: first differing columns: {bad[:8]}"
            del t_host
        if (table, num_io) == ("fq", 1024):
            assert prover.check_trace().ok
            proof = prover.prove()
            gpu.verify_stark_proof(stark, proof, cfg)
            assert proof.recover_degree_bits(cfg) == bits
    finally:
        prover.close()


# ---- b. crafted histograms through main-row mode -------------------------------------------------------------------------------------
def from_counts(n, values, counts, rest):
    """`counts[i]` copies of `values[i]`; what is missing to n rows goes to `rest` (an array cycled through, or one value)."""
    col = np.repeat(np.asarray(values, dtype=np.uint64), np.asarray(counts, dtype=np.int64))
    assert col.size <= n, (col.size, n)
    fill = np.resize(np.asarray(rest, dtype=np.uint64), n - col.size)
    return np.concatenate([col, fill])


def histogram_families(n, rng):
    """[(name, column)]: the histograms of the issue, each a column of n words below 2^16 (in sorted order; the caller shuffles)."""
    KT, every, k16 = n - 65535, n // 65536, np.arange(65536)
    fam = [(f"constant {v}", np.full(n, v, dtype=np.uint64)) for v in (0, 12345, 65535)]
    for c65 in (KT - 1, KT, KT + 1):   # the 65535 run against the KT copies of the table; the rest spread below
        fam.append((f"{c65} x 65535", from_counts(n, [65535], [c65], np.arange(65535))))
    # T reaches every multiple of 2^16 exactly at a value boundary, one short of it, one past it
    cross = (np.arange(1, every) * (65536 // every)) if every > 1 else np.zeros(0, dtype=np.int64)
    for name, d in (("T = k 2^16 at a boundary", 0), ("T = k 2^16 - 1", -1), ("T = k 2^16 + 1", 1)):
        counts = np.full(65536, every, dtype=np.int64)
        counts[cross - 1] += d
        counts[cross] -= d
        assert counts.sum() == n and np.array_equal(np.cumsum(counts)[cross - 1], np.arange(1, every) * 65536 + d)
        fam.append((name, from_counts(n, k16, counts, 0)))
    # one value carries T over three multiples of 2^16 at once: T = 2,000 below it, 2,000 + 200,000 at it
    fam.append(("one value across three multiples", from_counts(n, np.r_[np.arange(1000), 1000], np.r_[np.full(1000, 2), 200000], 1001 + np.arange(60000))))
    fam.append(("2040 values x 257", from_counts(n, 5 + 32 * np.arange(2040), np.full(2040, 257), 0)))
    for distinct in (1023, 1024, 1025):
        for occ in sorted({512, 513, n // 1024 + 1}):
            k = min(distinct, n // occ)   # as many as fit
            fam.append((f"{k} values x {occ}", from_counts(n, 7 + 60 * np.arange(k), np.full(k, occ), 65530)))
    fam.append(("values in [60000, 65535]", rng.integers(60000, 65536, n, dtype=np.uint64)))
    fam.append(("0 and 65535", rng.integers(0, 2, n, dtype=np.uint64) * np.uint64(65535)))
    fam.append(("uniform", rng.integers(0, 65536, n, dtype=np.uint64)))
    fam.append(("heavy tail", (np.minimum(rng.zipf(1.3, n), 65536) - 1).astype(np.uint64)))
    for name, col in fam:
        assert col.shape == (n,) and col.dtype == np.uint64 and int(col.max()) < 65536, name
    return fam


@pytest.fixture(scope="module")
def crafted_rows(gpu):
    """(stark, bits, rows, names): main-column rows of FqExpStark(1024) whose column c holds family c mod len(families)."""
    stark = gpu.FqExpStark(1024)
    bits = 19
    n = 1 << bits
    rng = np.random.default_rng(190)
    fam = histogram_families(n, rng)
    assert len(fam) < 143   # every family lands in a range-checked column (the first 143 main columns of FqExpStark)
    order = rng.permutation(n)
    cols = np.empty((stark.num_main_columns, n), dtype=np.uint64)
    for c in range(cols.shape[0]):
        cols[c] = fam[c % len(fam)][1][order]
    return stark, bits, np.ascontiguousarray(cols.T), [f[0] for f in fam]


def test_crafted_histograms_through_main_row_mode(gpu, crafted_rows):
    """load_trace_rows(main rows) + read_trace() == trace_from_rows_host(rows): the sorted and permuted columns of every
    histogram family.  The rows are no witness; this path checks canonical form and the u16 range only."""
    stark, bits, rows, names = crafted_rows
    want = gpu.trace_from_rows_host(stark, rows)
    prover = gpu.Prover(stark, stark.config(), bits)
    try:
        prover.load_trace_rows(rows, np.zeros(stark.num_public_inputs, dtype=np.uint64))
        bad = differing_columns(prover, want)
        assert not bad, f"first differing columns: {bad[:8]} (main columns hold {names}, cycled)"
    finally:
        prover.close()


def test_a_word_of_2pow16_is_refused_and_leaves_no_trace(gpu, crafted_rows):
    stark, bits, rows, _ = crafted_rows
    pi = np.zeros(stark.num_public_inputs, dtype=np.uint64)
    prover = gpu.Prover(stark, stark.config(), bits)
    try:
        prover.load_trace_rows(rows, pi)
        bad = rows.copy()
        bad[(1 << bits) - 3, 0] = 65536              # column 0 is range-checked
        with pytest.raises(gpu.SbnError) as e:
            prover.load_trace_rows(bad, pi)
        assert e.value.code == WITNESS, str(e.value)
        with pytest.raises(gpu.SbnError) as e:
            prover.prove()
        assert e.value.code == BAD_ARG and "no trace loaded" in str(e.value)
    finally:
        prover.close()


# ---- c. chained lists -----------------------------------------------------------------------------------------------------------------
XW = {"g1": 16, "g2": 32}
CURVE_ORDER = T.R


def terms_of(table, ios):
    xw = XW[table]
    return np.ascontiguousarray(np.concatenate([ios[:, :xw], ios[:, 2 * xw:]], axis=1))


def neg_point_words(table, w):
    """-P of an affine point in instance words: y -> p - y on every coordinate of y."""
    xw = XW[table]
    out = np.array(w, dtype=np.uint32).copy()
    for q in range(xw // 2 // 8):
        y = T.from_limbs(out[xw // 2 + 8 * q: xw // 2 + 8 * q + 8], 32)
        out[xw // 2 + 8 * q: xw // 2 + 8 * q + 8] = T.limbs((T.P - y) % T.P, 8, 32)
    return out


def chained_cases(table, ios):
    """{name: (terms, start)}; the start is the offset of instance 0 of the random list."""
    xw = XW[table]
    terms, start = terms_of(table, ios), ios[0, xw:2 * xw].copy()
    cases = {"random": (terms, start)}
    ident = terms.copy()
    ident[[0, 5, 511, 512, 513, 1023], xw:] = 0                # exponent 0: the term is the identity, the offset passes through
    cases["identity terms"] = (ident, start)
    # terms 600 and 601 are (x, 1) and (-x, 1): inside the scan the lane of 601 first holds x + (-x) = the point at infinity, while
    # the offsets are sums from the start and none of them is at infinity
    opp = terms.copy()
    opp[600, xw:] = 0
    opp[601, xw:] = 0
    opp[600, xw] = opp[601, xw] = 1
    opp[601, :xw] = neg_point_words(table, opp[600, :xw])
    cases["opposite partial sums"] = (opp, start)
    # offset[513] = start + (e_0 x_0 + ... + e_512 x_512) at infinity: terms 0..511 have exponent 0, term 512 is (-start, 1)
    inf = terms.copy()
    inf[:512, xw:] = 0
    inf[512, xw:] = 0
    inf[512, xw] = 1
    inf[512, :xw] = neg_point_words(table, start)
    cases["offset 513 at infinity"] = (inf, start)
    return cases


@pytest.mark.parametrize("table", ["g1", "g2"])
def test_chained_lists_of_1024_instances(gpu, O, table):
    """generate_trace_chained(terms, start) under the device placements of the chains (and once on the host-pool fall-back):
    the derived list and the public inputs equal chain_instances' and the host generator's; G1: the whole trace too; G2:
    check_trace().ok.  An offset at infinity at index 513 is SBN_ERR_WITNESS, on the device as on the host."""
    stark, cfg, bits, ios = make(gpu, O, table, 1024, 50)
    cases = chained_cases(table, ios)
    bad_terms, bad_start = cases.pop("offset 513 at infinity")
    with pytest.raises(gpu.SbnError) as e:
        gpu.chain_instances(stark, bad_terms, bad_start)
    assert e.value.code == WITNESS
    want, pis = {}, {}
    for name, (terms, start) in cases.items():
        lst, final = gpu.chain_instances(stark, terms, start)
        want[name] = lst
        # the public inputs of an instance are its row and its output; output[k] = offset[k + 1], the last one is `final`
        outs = np.concatenate([lst[1:, XW[table]:2 * XW[table]], final.reshape(1, -1)])
        pis[name] = np.concatenate([lst, outs], axis=1).astype(np.uint64).reshape(-1)
    t_host, pi_host = stark.generate_trace_and_public_inputs(want["random"])
    assert np.array_equal(pis["random"], pi_host)
    for env in ({"SBN_TRACEGEN_DEVICE_CHAIN": "1"}, {"SBN_TRACEGEN_DEVICE_CHAIN": "2"}, {"SBN_TRACEGEN_DEVICE_CHAIN": "0"}):
        with T.placement(gpu, stark, cfg, bits, env) as pr:
            fallback = env["SBN_TRACEGEN_DEVICE_CHAIN"] == "0"
            for name, (terms, start) in cases.items():
                if fallback and name != "random":
                    continue
                pi, lst = pr.generate_trace_chained(terms, start)
                assert np.array_equal(lst, want[name]), (env, name)
                assert np.array_equal(pi, pis[name]), (env, name)
                if name == "random":
                    if table == "g1":
                        bad = differing_columns(pr, t_host)
                        assert not bad, (env, bad[:8])
                    else:
                        assert pr.check_trace().ok, env
            if not fallback:
                with pytest.raises(gpu.SbnError) as e:
                    pr.generate_trace_chained(bad_terms, bad_start)
                assert e.value.code == WITNESS, (env, str(e.value))


# ---- d. segmented lists ---------------------------------------------------------------------------------------------------------------
def lengths_with_heads(heads, M):
    heads = sorted(set([0] + [h for h in heads if 0 < h < M]))
    return [b - a for a, b in zip(heads, heads[1:] + [M])]


SEGMENT_SHAPES = {
    "1024 segments of 1": [1] * 1024,
    "one segment of 1024": [1024],
    "heads at 511 512 513": lengths_with_heads([511, 512, 513], 1024),
    "heads at block +-1": lengths_with_heads([BLOCK * b + d for b in range(1, 1024 // BLOCK + 1) for d in (-1, 0, 1)] + [100, 700], 1024),
    "a head on 512 only": lengths_with_heads([512], 1024),
    "heads at 511 and 513, none on 512": lengths_with_heads([300, 511, 513], 1024),
    "M < K, the last block partly real": lengths_with_heads([200, 510, 512, 600], 777),
    "M < K, one block of real instances": lengths_with_heads([17, 300], 400),
}


def test_segmented_lists_on_1024_instances(gpu, O):
    """generate_trace_msms(terms, lengths, starts) on G1ExpStark(1024), device placements: the list, finals, sums and infinity
    flags equal msm_batch_instances'; heads on, before and behind the block boundary of the device scan, padded rows, per-segment
    starts and one shared start."""
    stark, cfg, bits, ios = make(gpu, O, "g1", 1024, 60)
    terms = terms_of("g1", ios)
    # a pair (x, e), (-x, e) at 511 | 512: where they share a segment its running sum returns to the sum before them
    terms[512, :16] = neg_point_words("g1", terms[511, :16])
    terms[512, 16:] = terms[511, 16:]
    calls = []
    for name, lengths in SEGMENT_SHAPES.items():
        M = sum(lengths)
        per = ios[:len(lengths), 16:32].copy()                  # per-segment starts: offsets of the random list
        calls.append((name, terms[:M], lengths, per))
    calls.append(("heads at 511 512 513, shared start", terms, SEGMENT_SHAPES["heads at 511 512 513"], ios[7, 16:32].copy()))
    calls.append(("one segment of 1024, default start", terms, [1024], None))
    want = {name: gpu.msm_batch_instances(stark, t, np.array(l, dtype=np.uint64), s) for name, t, l, s in calls}
    for env in ({"SBN_TRACEGEN_DEVICE_CHAIN": "2"}, {"SBN_TRACEGEN_DEVICE_CHAIN": "1"}):
        with T.placement(gpu, stark, cfg, bits, env) as pr:
            for name, t, l, s in calls:
                if env["SBN_TRACEGEN_DEVICE_CHAIN"] == "1" and not name.startswith(("heads at block", "M < K, the last")):
                    continue   # the scan kernels are the same under both placements: the two widest shapes again
                _, finals, sums, infinity, lst = pr.generate_trace_msms(t, np.array(l, dtype=np.uint64), s)
                w_ios, w_finals, w_sums, w_inf = want[name]
                assert w_ios.shape[0] == 1
                assert np.array_equal(lst, w_ios[0]), (env, name)
                assert np.array_equal(finals, w_finals) and np.array_equal(sums, w_sums) and np.array_equal(infinity, w_inf), (env, name)


# ---- e. diff_witness ------------------------------------------------------------------------------------------------------------------
def test_diff_witness_at_2pow19_rows(gpu, O):
    """Clean after generate_trace; with one cell of a loaded host trace changed by 1 the report names that cell and equals
    diff_witness_host's."""
    stark, cfg, bits, ios = make(gpu, O, "fq", 1024, 70)
    prover = gpu.Prover(stark, cfg, bits)
    try:
        prover.generate_trace(ios)
        clean = prover.diff_witness(ios)
        assert clean.ok, str(clean)
        trace, pi = stark.generate_trace_and_public_inputs(ios)
        col, row = 77, (1 << bits) - 12345
        trace[col, row] += 1
        prover.load_trace(trace, pi)
        got = prover.diff_witness(ios)
        assert not got.ok
        assert [(c["column"], c["row"]) for c in got.listed] == [(col, row)], str(got)
        assert got == gpu.diff_witness_host(stark, trace, pi, ios)
    finally:
        prover.close()


# ---- f. refusals that stay ------------------------------------------------------------------------------------------------------------
def test_refusals_that_stay(gpu, O):
    """A prover whose degree_bits does not match num_io is refused at creation (BAD_ARG); an instance count other than the
    prover's is BAD_ARG; a table that is not an Exp table has no device witness (UNSUPPORTED)."""
    stark, cfg, bits, ios = make(gpu, O, "fq", 1024, 80)
    with pytest.raises(gpu.SbnError) as e:
        gpu.Prover(stark, cfg, bits - 1)
    assert e.value.code == BAD_ARG
    prover = gpu.Prover(stark, cfg, bits)
    try:
        with pytest.raises(gpu.SbnError) as e:
            prover.generate_trace(ios[:512])
        assert e.value.code == BAD_ARG
    finally:
        prover.close()
    other = gpu.ModularStark()
    q = gpu.Prover(other, other.config(), 9)
    try:
        pi = np.zeros(1, dtype=np.uint64)
        rc = gpu.lib().sbn_prover_generate_trace(q._h, ios.ctypes.data_as(C.c_void_p), 1024, pi.ctypes.data_as(C.c_void_p))
        assert rc == UNSUPPORTED
    finally:
        q.close()
