"""Prover.prove_host_trace (the upload inside the commit pipeline, the canonical-form scan on the device) and the context cache of
the one-shot prove(), on a real GPU, all in this process.  The yardstick of every proof is load_trace + prove on a second
prover, and for two tables the oracle's digest in tests/golden/proof_digests.json.

Mutations tried against this file, once each (library rebuilt with the one change):
  (a) the wait on upload_done[k] removed from commit_pipeline: a race; in its one run the same-proof test failed for ModularStark,
      Fq12ExpStark and G1ExpStark (G1Stark, FlagStark, LookupStark passed by luck), both refusal tests and the cache test failed;
  (b) the scan kernel skipping the single word behind the last whole vector: 24 cases of
      test_first_non_canonical_device_matches_numpy and both test_first_non_canonical_device_last_partial_vector cases fail;
  (c) `loaded` left true on refusal: both test_prove_host_trace_refuses_non_canonical_words cases fail;
  (d) the cache key without fri_variant: test_prove_cache fails (the plain-FRI call is handed the other protocol's context)."""
import hashlib
import threading

import numpy as np
import pytest

from test_host_trace import GL_P, canonical_words, reference_index, scan_cases

pytestmark = pytest.mark.gpu
NO_PI = np.zeros(0, dtype=np.uint64)


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    return S


# ---- the scan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,words", scan_cases(), ids=[n for n, _ in scan_cases()])
def test_first_non_canonical_device_matches_numpy(gpu, name, words):
    assert gpu.first_non_canonical(words, on_device=True) == reference_index(words)


@pytest.mark.parametrize("lead", [0, 1])
def test_first_non_canonical_device_last_partial_vector(gpu, lead):
    """A few million words whose only bad word is the very last one, which no whole 16-byte vector covers (odd count; lead = 1
    also shifts the slice by 8 bytes, so one of the two runs has the single word in front AND the one behind)."""
    count = 3 * (1 << 20) + 1
    base = canonical_words(count + 1, 42)
    w = base[lead:lead + count - lead]
    assert gpu.first_non_canonical(w, on_device=True) == len(w)
    w[len(w) - 1] = GL_P
    assert gpu.first_non_canonical(w, on_device=True) == len(w) - 1
    w[len(w) - 1] = GL_P - 1
    w[0] = 2**64 - 1
    assert gpu.first_non_canonical(w, on_device=True) == 0
    w[0] = 0
    w[123457] = GL_P + 5; w[2 * (1 << 20) + 3] = GL_P   # two bad words in different workgroups: the smaller index wins
    assert gpu.first_non_canonical(w, on_device=True) == 123457


# ---- same proof --------------------------------------------------------------------------------------------------------
def table_case(S, O, name, request):
    """(stark, trace, public inputs, golden key or None)"""
    if name == "G1Stark":
        c = request.getfixturevalue("g1op_case")
        return S.G1Stark(), c["trace"], c["pi"], "g1op_rows512_seed0"
    if name == "ModularStark":
        stark = S.ModularStark()
        ops, _ = O.modular_inputs(512, 6)
        return stark, stark.generate_trace(ops), NO_PI, None
    if name == "FlagStark":
        stark = S.FlagStark(4)
        limbs, _ = O.flags_inputs(4, 8)
        return stark, stark.generate_trace(limbs), NO_PI, None
    if name == "LookupStark":
        stark = S.LookupStark()
        ins, tab = O.lookup_inputs(512, 9)
        return stark, stark.generate_trace(ins, tab), NO_PI, None
    if name == "Fq12ExpStark":
        c = request.getfixturevalue("fq12exp_case")
        return S.Fq12ExpStark(16), c["trace"], c["pi"], None
    if name == "G1ExpStark":
        c = request.getfixturevalue("g1exp_case")
        return S.G1ExpStark(128), c["trace"], c["pi"], "g1exp_io128_seed1"
    raise KeyError(name)


def two_step_proof(S, stark, cfg, db, trace, pi):
    q = S.Prover(stark, cfg, db)
    try:
        q.load_trace(trace, pi)
        return q.prove().words
    finally:
        q.close()


@pytest.mark.parametrize("name", ["G1Stark", "ModularStark", "FlagStark", "LookupStark", "Fq12ExpStark", "G1ExpStark"])
def test_prove_host_trace_gives_the_proof_of_load_trace_and_prove(gpu, O, golden, request, name):
    S = gpu
    stark, trace, pi, key = table_case(S, O, name, request)
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    cfg = stark.config()
    db = trace.shape[1].bit_length() - 1
    assert trace.shape[0] == stark.num_columns
    want = two_step_proof(S, stark, cfg, db, trace, pi)
    p = S.Prover(stark, cfg, db)
    try:
        proof = p.prove_host_trace(trace, pi)
        assert np.array_equal(proof.words, want)
        if key:
            assert hashlib.sha256(proof.to_bytes()).hexdigest() == golden["proof_digests"][key]["proof_sha256"]
        assert np.array_equal(p.prove().words, want)          # the trace is resident as after load_trace
        assert np.array_equal(p.read_trace(), trace)
        ro = trace.view()
        ro.flags.writeable = False
        assert np.array_equal(p.prove_host_trace(ro, pi).words, want)
        assert np.array_equal(p.prove_host_trace(trace, pi).words, want)   # the ring and the events are reused
    finally:
        p.close()


# ---- device memory: one list allocates, plans and frees -------------------------------------------------------------------
# LookupStark at 2^9 rows: 4 columns and 2 Z columns, the one-launch commitment (no chunk pipeline); FlagStark(16) at 2^13 rows: 81
# columns in two chunks, and no Z (no permutation stage, no Z commitment).  One context per table.
@pytest.mark.parametrize("name", ["LookupStark", "FlagStark16"])
def test_dev_bytes_are_the_plan_and_the_lazy_scan_word_through_prove_host_trace(gpu, O, name):
    """describe()["dev_bytes"] counts what the context allocated: the memory plan after creation, the plan + 8 after the first
    prove_host_trace (d_first_bad, allocated by that call and outside the plan, include/sbn.h), and the same after the second; both
    proofs are the words of load_trace + prove."""
    S = gpu
    if name == "LookupStark":
        stark = S.LookupStark()
        trace = stark.generate_trace(*O.lookup_inputs(512, 9))
    else:
        stark = S.FlagStark(16)
        trace = stark.generate_trace(O.flags_inputs(16, 8)[0])
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    cfg = stark.config()
    db = trace.shape[1].bit_length() - 1
    assert (stark.num_columns, stark.num_permutation_zs(), db) == ((4, 2, 9) if name == "LookupStark" else (81, 0, 13))
    plan = S.prover_memory_plan(stark, cfg, db)
    p = S.Prover(stark, cfg, db)
    try:
        assert int(p.describe()["dev_bytes"]) == plan
        first = p.prove_host_trace(trace, NO_PI).words
        assert int(p.describe()["dev_bytes"]) == plan + 8
        second = p.prove_host_trace(trace, NO_PI).words
        assert int(p.describe()["dev_bytes"]) == plan + 8
        p.load_trace(trace, NO_PI)
        want = p.prove().words
        assert np.array_equal(first, want) and np.array_equal(second, want)
    finally:
        p.close()


# ---- refusal -----------------------------------------------------------------------------------------------------------
def plant_sets(ncols, n, chunk):
    """Flat word indices to set to p: word 0; the last word; the first word of the last (partial) chunk; a chunk seam."""
    words = ncols * n
    nchunks = (ncols + chunk - 1) // chunk
    assert nchunks >= 3 and ncols % chunk, "the table must have several chunks and a partial last one"
    last0 = (nchunks - 1) * chunk * n
    seam = (nchunks // 2) * chunk * n
    return {"word0": [0], "last_word": [words - 1], "last_chunk_first": [last0], "seam": [seam - 1, seam]}


@pytest.mark.parametrize("name", ["G1Stark", "G1ExpStark"])
def test_prove_host_trace_refuses_non_canonical_words(gpu, O, request, name):
    S = gpu
    stark, trace, pi, _ = table_case(S, O, name, request)
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    cfg = stark.config()
    ncols, n = trace.shape
    db = n.bit_length() - 1
    want = two_step_proof(S, stark, cfg, db, trace, pi)
    p = S.Prover(stark, cfg, db)
    q = S.Prover(stark, cfg, db)   # load_trace's message for the same input
    try:
        chunk = int(p.describe()["ntt_chunk"])
        bad = trace.copy()
        flat = bad.reshape(-1)
        for label, idxs in plant_sets(ncols, n, chunk).items():
            assert np.array_equal(p.prove_host_trace(trace, pi).words, want), label   # a valid trace is loaded before every refusal
            keep = flat[idxs].copy()
            flat[idxs] = GL_P
            with pytest.raises(S.SbnError) as e_load:
                q.load_trace(bad, pi)
            with pytest.raises(S.SbnError) as e_host:
                p.prove_host_trace(bad, pi)
            flat[idxs] = keep
            assert e_host.value.code == -2, label
            assert str(e_host.value) == str(e_load.value) == f"sbn error -2: trace word {min(idxs)} is not canonical", label
            with pytest.raises(S.SbnError) as e_prove:
                p.prove()
            assert e_prove.value.code == -1 and "no trace loaded" in str(e_prove.value), label
            with pytest.raises(S.SbnError):
                p.read_trace()
        assert np.array_equal(bad, trace)
        # a non-canonical public input (or, for a table without public inputs, one too many) is refused on the host
        if len(pi):
            bad_pi = pi.copy(); bad_pi[len(pi) // 2] = GL_P
            code = -2
        else:
            bad_pi, code = np.array([GL_P], dtype=np.uint64), -1
        assert np.array_equal(p.prove_host_trace(trace, pi).words, want)
        with pytest.raises(S.SbnError) as e_pi:
            p.prove_host_trace(trace, bad_pi)
        assert e_pi.value.code == code
        with pytest.raises(S.SbnError) as e_prove:
            p.prove()
        assert e_prove.value.code == -1 and "no trace loaded" in str(e_prove.value)
        # streams and ring are left in order: the same prover proves the clean trace
        assert np.array_equal(p.prove_host_trace(trace, pi).words, want)
        assert np.array_equal(p.prove().words, want)
    finally:
        p.close(); q.close()


# ---- the cache ---------------------------------------------------------------------------------------------------------
def test_prove_cache(gpu, O, g1op_case):
    S = gpu
    g1, md = S.G1Stark(), S.ModularStark()
    ops, _ = O.modular_inputs(512, 6)
    cases = [(g1, g1.config(), np.ascontiguousarray(g1op_case["trace"]), NO_PI), (md, md.config(), md.generate_trace(ops), NO_PI)]
    S.prove_cache_configure(0)
    want = [S.prove(st, cfg, tr, pi).words for st, cfg, tr, pi in cases]     # the cache off
    assert S.prove_cache_stats()["contexts_resident"] == 0
    try:
        # the two context sizes, from the stats after one cached call each
        sizes = []
        for (st, cfg, tr, pi), w in zip(cases, want):
            S.prove_cache_configure(1 << 40)
            assert np.array_equal(S.prove(st, cfg, tr, pi).words, w)
            s = S.prove_cache_stats()
            assert s["contexts_resident"] == 1 and s["bytes_resident"] > 0
            sizes.append(s["bytes_resident"])
            S.prove_cache_configure(0)
            assert S.prove_cache_stats()["contexts_resident"] == 0 and S.prove_cache_stats()["bytes_resident"] == 0
        # each context holds at least its trace, coefficients and LDE
        for (st, cfg, tr, pi), b in zip(cases, sizes):
            assert b >= tr.size * 8 * 4

        # a budget that holds both: two threads alternate the tables, 6 calls each
        budget = sum(sizes)
        S.prove_cache_configure(budget)
        before = S.prove_cache_stats()
        errors = []

        def worker(first):
            try:
                for i in range(6):
                    k = (first + i) % 2
                    st, cfg, tr, pi = cases[k]
                    got = S.prove(st, cfg, tr, pi).words
                    if not np.array_equal(got, want[k]):
                        errors.append(f"thread {first} call {i}: proof differs")
                    s = S.prove_cache_stats()
                    if s["bytes_resident"] > s["budget"]:
                        errors.append(f"thread {first} call {i}: {s}")
            except Exception as e:   # noqa: BLE001
                errors.append(repr(e))

        th = [threading.Thread(target=worker, args=(f,)) for f in (0, 1)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
        s = S.prove_cache_stats()
        assert s["hits"] - before["hits"] > 0
        assert (s["hits"] - before["hits"]) + (s["misses"] - before["misses"]) == 12
        assert s["bytes_resident"] <= budget and s["contexts_resident"] <= 2

        # a key that differs in fri_variant alone is another context, and its proof is the other protocol's
        S.prove_cache_configure(0)
        S.prove_cache_configure(budget + sizes[0])
        st, cfg, tr, pi = cases[0]
        cfg2 = st.config(); cfg2.fri_variant = 2
        want_plain = S.prove(st, cfg2, tr, pi).words
        assert not np.array_equal(want_plain, want[0])
        assert np.array_equal(S.prove(st, cfg, tr, pi).words, want[0])
        assert np.array_equal(S.prove(st, cfg2, tr, pi).words, want_plain)
        assert np.array_equal(S.prove(st, cfg, tr, pi).words, want[0])
        assert S.prove_cache_stats()["contexts_resident"] == 2

        # a budget that holds the larger but not both: alternating calls evict
        S.prove_cache_configure(0)
        budget = max(sizes)
        assert budget < sum(sizes)
        S.prove_cache_configure(budget)
        before = S.prove_cache_stats()
        for i in range(6):
            st, cfg, tr, pi = cases[i % 2]
            assert np.array_equal(S.prove(st, cfg, tr, pi).words, want[i % 2])
            s = S.prove_cache_stats()
            assert s["bytes_resident"] <= budget, s
        assert S.prove_cache_stats()["evictions"] - before["evictions"] > 0

        # a failing call does not raise the number of resident contexts (its context is destroyed, not given back)
        st, cfg, tr, pi = cases[0]
        S.prove_cache_configure(0)
        S.prove_cache_configure(sum(sizes))
        assert np.array_equal(S.prove(st, cfg, tr, pi).words, want[0])
        resident = S.prove_cache_stats()["contexts_resident"]
        assert resident == 1
        bad = tr.copy(); bad[5, 7] = GL_P
        with pytest.raises(S.SbnError) as e:
            S.prove(st, cfg, bad, pi)
        assert e.value.code == -2 and f"trace word {5 * tr.shape[1] + 7} is not canonical" in str(e.value)
        assert S.prove_cache_stats()["contexts_resident"] <= resident
        assert np.array_equal(S.prove(st, cfg, tr, pi).words, want[0])
    finally:
        S.prove_cache_configure(0)
    s = S.prove_cache_stats()
    assert s["contexts_resident"] == 0 and s["bytes_resident"] == 0 and s["budget"] == 0
