"""The host-trace entry points without a device: the canonical-form scan of Prover.prove_host_trace as a building block (host
loop), the context cache's configuration and counters, and the null-argument refusals of the new C ABI functions."""
import ctypes as C

import numpy as np
import pytest

GL_P = 0xFFFFFFFF00000001
COUNTS = [0, 1, 3, 4, 5, 255, 256, 257]
BAD_VALUES = [GL_P, GL_P + 1, 2**64 - 1]


def reference_index(words):
    """numpy's answer: the first index whose word is >= p, or len(words)."""
    bad = np.nonzero(np.asarray(words, dtype=np.uint64) >= np.uint64(GL_P))[0]
    return int(bad[0]) if len(bad) else len(words)


def canonical_words(count, seed):
    return np.random.default_rng(seed).integers(0, GL_P, size=count, dtype=np.uint64)


def scan_cases():
    """(name, array) pairs shared with the device test: clean arrays, planted words at the ends and at two places, p - 1
    everywhere, every listed count, and a slice that starts 8 bytes off a 16-byte boundary."""
    cases = []
    for count in COUNTS:
        w = canonical_words(count, count)
        cases.append((f"clean_{count}", w))
        cases.append((f"pm1_{count}", np.full(count, GL_P - 1, dtype=np.uint64)))
        if count == 0:
            continue
        for v in BAD_VALUES:
            a = w.copy(); a[0] = v
            cases.append((f"first_{count}_{v:x}", a))
            b = w.copy(); b[count - 1] = v
            cases.append((f"last_{count}_{v:x}", b))
            if count >= 3:
                c = w.copy(); c[count - 1] = v; c[count // 2] = v
                cases.append((f"two_{count}_{v:x}", c))
    for count in (1, 2, 5, 256, 257):
        for lead in (0, 1):   # one of the two slices starts 8 bytes off a 16-byte boundary, whatever numpy's allocation
            base = canonical_words(count + 2, 100 + count)
            view = base[lead:lead + count]
            cases.append((f"offset{lead}_clean_{count}", view))
            base2 = base.copy(); base2[lead] = GL_P
            cases.append((f"offset{lead}_first_{count}", base2[lead:lead + count]))
            base3 = base.copy(); base3[lead + count - 1] = GL_P + 1
            cases.append((f"offset{lead}_last_{count}", base3[lead:lead + count]))
            base4 = base.copy(); base4[lead + count] = GL_P   # just outside the slice: must not be seen
            cases.append((f"offset{lead}_outside_{count}", base4[lead:lead + count]))
    return cases


def test_scan_cases_cover_an_unaligned_slice():
    offs = {a.ctypes.data % 16 for name, a in scan_cases() if name.startswith("offset")}
    assert 8 in offs


@pytest.mark.parametrize("name,words", scan_cases(), ids=[n for n, _ in scan_cases()])
def test_first_non_canonical_host_matches_numpy(S, name, words):
    assert S.first_non_canonical(words, on_device=False) == reference_index(words)


def test_first_non_canonical_smaller_index_wins(S):
    w = canonical_words(1000, 7)
    w[700] = GL_P; w[33] = 2**64 - 1
    assert S.first_non_canonical(w, on_device=False) == 33


def test_first_non_canonical_null_arguments(S):
    L = S.lib()
    out = C.c_uint64(0)
    assert L.sbn_first_non_canonical(None, 4, 0, C.byref(out)) == -1
    w = canonical_words(4, 1)
    assert L.sbn_first_non_canonical(w.ctypes.data_as(C.c_void_p), 4, 0, None) == -1
    assert L.sbn_first_non_canonical(None, 0, 0, C.byref(out)) == 0 and out.value == 0


def test_prove_cache_configure_and_stats_need_no_device(S):
    L = S.lib()
    try:
        S.prove_cache_configure(0)
        assert S.prove_cache_stats() == {"hits": 0, "misses": 0, "evictions": 0, "contexts_resident": 0, "bytes_resident": 0, "budget": 0}
        S.prove_cache_configure(12345)
        st = S.prove_cache_stats()
        assert st["budget"] == 12345 and all(v == 0 for k, v in st.items() if k != "budget")
        assert L.sbn_prove_cache_stats(None) == -1   # SBN_ERR_BAD_ARG
        assert L.sbn_last_error() == b"null argument"
    finally:
        S.prove_cache_configure(0)
    assert S.prove_cache_stats()["budget"] == 0


def test_prove_host_trace_refuses_a_null_prover(S):
    L = S.lib()
    w = canonical_words(8, 2)
    h = C.c_void_p(1)
    assert L.sbn_prover_prove_host_trace(None, w.ctypes.data_as(C.c_void_p), None, 0, C.byref(h)) == -1
    assert L.sbn_prover_prove_host_trace(None, w.ctypes.data_as(C.c_void_p), None, 0, None) == -1


def test_public_input_refusals_read_the_same_without_a_prover(S, fq12expu64_case):
    """One routine takes the public inputs of every intake call (csrc/trace_load.hip take_public_inputs): the count, the pointer,
    then canonical form, in that order and with these exact words.  The calls with a prover need a device; sbn_prove_rows reaches
    the routine through its precheck, in front of any device, and sbn_trace_from_rows_host shares its flag check."""
    L = S.lib()
    stark = S.Fq12ExpU64Stark(16)
    cfg = stark.config()
    pi = np.ascontiguousarray(fq12expu64_case["pi"], dtype=np.uint64)
    npi = len(pi)
    assert npi == stark.num_public_inputs and npi > 3
    rows = np.ascontiguousarray(fq12expu64_case["trace"][:stark.num_main_columns].T)
    n, nc = rows.shape
    table = S.api._HostRows(C.sizeof(S.api._HostRows), 0, rows.ctypes.data, nc, None, n, nc)

    def prove_rows(pis, n_pi, flags=0):
        h = C.c_void_p(1)
        rc = L.sbn_prove_rows(C.byref(stark._d), C.byref(cfg._c), C.byref(table), flags, pis.ctypes.data_as(C.c_void_p) if pis is not None else None, n_pi, C.byref(h))
        assert h.value is None
        return rc, L.sbn_last_error().decode()

    two_bad = pi.copy(); two_bad[npi - 1] = 2**64 - 1; two_bad[2] += np.uint64(GL_P)
    for flags in (0, 1):   # SBN_TRACE_REDUCE changes nothing in front of the canonical-form check
        assert prove_rows(pi, npi - 1, flags) == (-1, f"expected {npi} public inputs, got {npi - 1}")
        assert prove_rows(pi, npi + 1, flags) == (-1, f"expected {npi} public inputs, got {npi + 1}")
        assert prove_rows(None, npi, flags) == (-1, "null public inputs")
        assert prove_rows(None, npi - 1, flags) == (-1, f"expected {npi} public inputs, got {npi - 1}")   # the count comes first
        assert prove_rows(two_bad, npi + 1, flags) == (-1, f"expected {npi} public inputs, got {npi + 1}")
    for i in (0, 3, npi - 1):
        bad = pi.copy(); bad[i] = GL_P
        assert prove_rows(bad, npi) == (-2, f"public input {i} is not canonical")
    assert prove_rows(two_bad, npi) == (-2, "public input 2 is not canonical")      # the smallest index
    # the flag check stands in front of the public inputs, and reads the same where there are none
    assert prove_rows(None, npi - 1, flags=6) == (-1, "unknown flag bits 0x6")
    out = np.zeros(1, dtype=np.uint64)
    assert L.sbn_trace_from_rows_host(C.byref(stark._d), C.byref(table), 6, out.ctypes.data_as(C.c_void_p), None) == -1
    assert L.sbn_last_error() == b"unknown flag bits 0x6"
    if L.sbn_device_count() == 0:   # under the flag the words are reduced, not refused: the call gets as far as the device
        assert prove_rows(two_bad, npi, flags=1)[0] == -3   # SBN_ERR_NO_DEVICE
