"""The batch verifier on the device (run on the MI355X box with `-m gpu`).  The reference for every verdict is the host verifier
sbn_verify on the same bytes: code AND reason string of every entry of a batch must be the host's.  Proofs come from the CPU oracle
(as in test_config_matrix.py) or, where noted, from the device prover; tampering goes through config_matrix.bump, which keeps words
canonical, so a tampered proof only produces a digest that does not match."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import config_matrix as M

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
NO_PI = np.zeros(0, dtype=np.uint64)


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    return S


def query_words(words):
    """Word indices inside the LAST query's answers (layout: include/sbn.h): for every initial oracle the last leaf word and a word of
    the last sibling, for every FRI layer the first and the last leaf word (two different extension values: at most one of them is
    the value the fold-consistency check reads) and a word of the first sibling; then the proof-of-work witness and, where the
    table has public inputs, the first of them.  A tree whose path has no sibling has no sibling entry."""
    degree_bits, ncol, nz, nq, npi, cap_h, rate_bits, layers, arity_bits, fpl, nqueries = M.header(words)
    capw, lde = 4 << cap_h, degree_bits + rate_bits
    queries = 12 + (3 if nz else 2) * capw + 2 * (2 * ncol + 2 * nz + nq) + layers * capw
    widths = [ncol] + ([nz] if nz else []) + [nq]
    stride, bits = sum(w + 4 * (lde - cap_h) for w in widths), lde
    for _ in range(layers):
        bits -= arity_bits
        stride += (2 << arity_bits) + 4 * (bits - cap_h)
    pos, out = queries + (nqueries - 1) * stride, {}
    for t, w in enumerate(widths):
        out[f"initial{t}_leaf"] = pos + w - 1
        pos += w
        nsib = lde - cap_h
        if nsib:
            out[f"initial{t}_sibling"] = pos + 4 * (nsib - 1) + 2
        pos += 4 * nsib
    bits = lde
    for l in range(layers):
        bits -= arity_bits
        out[f"fri{l}_leaf_first"] = pos
        out[f"fri{l}_leaf_last"] = pos + (2 << arity_bits) - 1
        pos += 2 << arity_bits
        nsib = bits - cap_h
        if nsib:
            out[f"fri{l}_sibling"] = pos + 1
        pos += 4 * nsib
    assert pos == queries + nqueries * stride
    out["pow_witness"] = pos + 2 * fpl
    if npi:
        out["public_input"] = pos + 2 * fpl + 1
    assert pos + 2 * fpl + 1 + npi == len(words)
    return out


def host_verdicts(S, stark, cfg, batch):
    """(code, reason) of sbn_verify for every proof of the batch; the message is read on the thread that made the call."""
    L = S.lib()

    def one(words):
        b = np.asarray(words, dtype="<u8").tobytes()
        rc = L.sbn_verify(C.byref(stark._d), C.byref(cfg._c), b, len(b))
        return (rc, L.sbn_last_error().decode() if rc else "")
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(one, batch))


def tampered_batch(words):
    """The proof, then one copy per section_words entry and per query_words entry with that word bumped."""
    where = dict(M.section_words(words))
    where.update(query_words(words))
    names = ["good"] + list(where)
    return names, [words] + [M.bump(words, where[n]) for n in names[1:]]


def check_batch(S, stark, cfg, bits, names, batch):
    want = host_verdicts(S, stark, cfg, batch)
    v = S.Verifier(stark, cfg, bits, max_batch=len(batch))
    try:
        got = v.verify([S.Proof(np.asarray(w, dtype=np.uint64), bits) for w in batch])
    finally:
        v.close()
    for n, g, w in zip(names, got, want):
        assert g == w, (n, g, w)
    return want


@pytest.fixture(scope="module")
def tables(gpu, O):
    """G1Stark at 512 rows (leaf rows of 2283 words = 285 blocks + 3 and of 1264 = 158 full blocks), LookupStark at 512 rows (a
    4-word trace leaf and a 2-word Z leaf, both their own digests), FlagStark(2) at 1024 rows (25 columns = 3 blocks + 1, no Z tree)."""
    pts, _ = O.g1op_inputs(512, 0)
    ins, tab = O.lookup_inputs(512, 9)
    limbs, _ = O.flags_inputs(2, 28)
    return {"g1op": (gpu.G1Stark(), O.AIR_G1_OP, 0, O.g1op_trace(pts)), "lookup": (gpu.LookupStark(), O.AIR_LOOKUP, 0, O.lookup_trace(ins, tab)),
            "flags": (gpu.FlagStark(2), O.AIR_FLAGS, 2, O.flags_trace(limbs))}


@pytest.mark.parametrize("table", ["g1op", "lookup", "flags"])
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_every_config_row_gets_the_host_verdicts(gpu, O, tables, table, case):
    stark, kind, num_io, trace = tables[table]
    row, times_x = case
    bits = trace.shape[1].bit_length() - 1
    words, _ = O.prove(kind, num_io, trace, NO_PI, config=row + (times_x,))
    names, batch = tampered_batch(words)
    want = check_batch(gpu, stark, M.make_config(gpu, row, times_x), bits, names, batch)
    assert want[0] == (0, "") and all(code == -6 for code, _ in want[1:]), list(zip(names, want))
    # the Merkle checks themselves were reached: a sibling of the last query is read by nothing else
    by_name = dict(zip(names, want))
    for n in names:
        if n.endswith("_sibling"):
            assert by_name[n][1].startswith("invalid Merkle proof"), (n, by_name[n])


def test_wide_leaf_and_public_inputs(gpu, O, fq12expu64_case):
    """Fq12ExpU64Stark(16): 2^11 rows x 9792 columns = 1224 full sponge blocks per trace leaf, 9232 public inputs; proved on the device."""
    stark = gpu.Fq12ExpU64Stark(16)
    cfg = stark.config()
    prover = gpu.Prover(stark, cfg, 11)
    try:
        prover.load_trace(fq12expu64_case["trace"], fq12expu64_case["pi"])
        words = prover.prove().words
    finally:
        prover.close()
    where = query_words(words)
    assert M.header(words)[1] == 9792 and M.header(words)[4] == 9232
    names = ["good", "public_input", "initial0_leaf"]
    want = check_batch(gpu, stark, cfg, 11, names, [words] + [M.bump(words, where[n]) for n in names[1:]])
    assert [c for c, _ in want] == [0, -6, -6]
    assert want[2][1].startswith("invalid Merkle proof (initial oracle 0, query 83)")


def test_batch_mechanics(gpu, g1op_case):
    stark = gpu.G1Stark()
    cfg = stark.config()
    good = g1op_case["proof"]
    where = query_words(good)
    bad = [M.bump(good, where[n]) for n in ("initial0_leaf", "initial1_sibling", "fri0_sibling", "pow_witness")]
    batch = [good, bad[0], good, bad[1], good, bad[2], good, bad[3]]
    want = host_verdicts(gpu, stark, cfg, batch)
    assert [c for c, _ in want] == [0, -6] * 4
    L = gpu.lib()
    v = gpu.Verifier(stark, cfg, 9, max_batch=8)
    try:
        as_proofs = lambda ws: [gpu.Proof(np.asarray(w, dtype=np.uint64), 9) for w in ws]
        assert v.verify(as_proofs(batch)) == want
        assert v.verify(as_proofs(batch[::-1])) == want[::-1]   # nothing leaks between slots or calls
        assert v.verify(as_proofs([bad[1]])) == [want[3]]
        assert v.verify(as_proofs([good])) == [(0, "")] and L.sbn_verifier_reason(v._h, 1) == b""
        # count 9 and count 0: a call-level refusal that leaves status_out alone
        bufs = [gpu.Proof(good, 9).to_bytes()] * 9
        ptrs, lens = (C.c_char_p * 9)(*bufs), (C.c_size_t * 9)(*[len(b) for b in bufs])
        for count in (9, 0):
            status = (C.c_int32 * 9)(*[77] * 9)
            assert L.sbn_verifier_verify(v._h, ptrs, lens, count, status) == -1
            assert list(status) == [77] * 9
        # a word >= p in a query leaf and a truncated proof: -5, as the host says, and their neighbours stay accepted
        noncanonical = np.array(good, dtype=np.uint64, copy=True)
        noncanonical[where["initial0_leaf"]] = P
        mixed = [good, noncanonical, good, good[:-1], good]
        want = host_verdicts(gpu, stark, cfg, mixed)
        assert [c for c, _ in want] == [0, -5, 0, -5, 0]
        assert v.verify(as_proofs(mixed)) == want
    finally:
        v.close()


def test_close_twice_and_a_verifier_of_another_config(gpu, g1op_case):
    """Row (6, 16, 2, 3, 28) implies another header than the default config's proof carries: -5, as expected_code in
    test_config_matrix.py says of the host verifier."""
    stark = gpu.G1Stark()
    cfg = M.make_config(gpu, (6, 16, 2, 3, 28))
    v = gpu.Verifier(stark, cfg, 9, max_batch=2)
    try:
        got = v.verify([gpu.Proof(g1op_case["proof"], 9)])
        assert got == host_verdicts(gpu, stark, cfg, [g1op_case["proof"]]) and got[0][0] == -5
    finally:
        v.close()
        v.close()


def test_a_proof_of_another_height_gets_the_host_verdict(gpu, O, g1op_case):
    """G1Stark has no fixed height: a 1024-row proof handed to a verifier created for 512 rows has another layout than its device
    slots.  sbn_verify accepts it, so the batch verifier must too (it finishes such a proof with the host sources), next to a
    512-row proof and to tampered copies of both."""
    stark = gpu.G1Stark()
    cfg = stark.config()
    pts, _ = O.g1op_inputs(1024, 3)
    tall, _ = O.prove(O.AIR_G1_OP, 0, O.g1op_trace(pts), NO_PI)
    good = g1op_case["proof"]
    batch = [tall, good, M.bump(tall, query_words(tall)["initial0_sibling"]), M.bump(good, query_words(good)["fri0_leaf_last"]), tall]
    want = host_verdicts(gpu, stark, cfg, batch)
    assert [c for c, _ in want] == [0, 0, -6, -6, 0]
    v = gpu.Verifier(stark, cfg, 9, max_batch=5)
    try:
        assert v.verify([gpu.Proof(np.asarray(w, dtype=np.uint64), 9) for w in batch]) == want
        assert v.verify([gpu.Proof(np.asarray(tall, dtype=np.uint64), 10)]) == [(0, "")]   # a batch with nothing for the device
    finally:
        v.close()
