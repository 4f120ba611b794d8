"""Every word of a proof through the batch verifier on the device (run on the MI355X box with `-m gpu`): the lists of
test_verifier_sweep_host.py, sent as batches.  The reference for every verdict is the host verifier sbn_verify on the same bytes,
code AND reason, as in test_verifier_gpu.py.  One work item of verify_items_kernel is (proof, query, tree), sixteen to a workgroup,
blockIdx.y the tree: the batches here put a tampered word in every item, leaf block and sibling level, at every batch position and
on both sides of the pinned ring's slot boundary (2^19 words)."""
import numpy as np
import pytest

import config_matrix as M
import parity_kit
import proof_words as W
import verifier_sweep as V

pytestmark = pytest.mark.gpu
CASES = [(t, r) for t in V.SMALL_TABLES for r in V.SMALL_ROWS]
case_id = lambda c: c[0] + "-" + "-".join(str(v) for v in c[1])   # noqa: E731
G1_ROW = (8, 8, 1, 0, 3)
SLOT_WORDS = 1 << 19   # VERIFY_SLOT_WORDS of csrc/verifier_device.hip


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    return S


def as_bytes(words):
    return np.asarray(words, dtype="<u8").tobytes()


def assert_device_is_host(names, got, want):
    assert len(got) == len(want) == len(names)
    for n, g, w in zip(names, got, want):
        assert g == w, ("device", g, "host", w, n)


def device_equals_host(S, c, names, batch, verifier=None):
    """batch: byte strings.  Returns the host verdicts."""
    want = V.host_verdicts(S, c.stark, c.cfg, batch)
    v = verifier or S.Verifier(c.stark, c.cfg, c.bits, max_batch=len(batch))
    try:
        got = v.verify(batch)
    finally:
        if verifier is None:
            v.close()
    assert_device_is_host(names, got, want)
    return want


def interleaved(c, idxs):
    """The bumped copies with the untampered proof at every 7th slot and at the last one; names are labels, None = the good proof."""
    good, slots = as_bytes(c.words), []
    for i in idxs:
        if len(slots) % 7 == 0:
            slots.append((None, good))
        slots.append(((i,) + W.label_of(c.words, i), as_bytes(M.bump(c.words, i))))
    slots.append((None, good))
    return [n for n, _ in slots], [b for _, b in slots]


def check_verdicts(c, names, want):
    for n, (code, reason) in zip(names, want):
        if n is None:
            assert (code, reason) == (0, ""), (code, reason)
        else:
            assert code == (-5 if n[0] < 12 else -6), (n, code, reason)
            predicted = W.expected_reason(c.words, c.indices, n[0])
            assert predicted is None or reason == predicted, (n, reason, predicted)


@pytest.mark.parametrize("tr", CASES, ids=case_id)
def test_every_word_bumped_in_one_batch(gpu, O, tr):
    c = V.case(gpu, O, *tr)
    clock = V.Clock()
    names, batch = interleaved(c, range(len(c.words)))
    assert names[0] is None and names[7] is None and names[-1] is None and len(batch) * len(c.words) * 8 < 320 << 20
    want = device_equals_host(gpu, c, names, batch)
    check_verdicts(c, names, want)
    print(f"\n{case_id(tr)}: {len(batch)} proofs of {len(c.words)} words in one batch, {clock.lap():.1f} s")


def test_one_item_per_proof_around_a_workgroup(gpu, O):
    """Row (4,16,4,5,1): one query, so one item per proof and tree and sixteen proofs per workgroup.  Batches of 15, 16, 17 and 33."""
    c = V.case(gpu, O, "lookup", (4, 16, 4, 5, 1))
    assert c.layout.nqueries == 1 and c.layout.query_stride >= 33
    bad = [as_bytes(M.bump(c.words, c.layout.query_off + k)) for k in range(33)]
    names = [(c.layout.query_off + k,) + W.label_of(c.words, c.layout.query_off + k) for k in range(33)]
    v = gpu.Verifier(c.stark, c.cfg, c.bits, max_batch=33)
    try:
        for n in (15, 16, 17, 33):
            want = device_equals_host(gpu, c, names[:n], bad[:n], verifier=v)
            check_verdicts(c, names[:n], want)
        assert v.verify([as_bytes(c.words)]) == [(0, "")]
    finally:
        v.close()


@pytest.mark.parametrize("tr", CASES, ids=case_id)
def test_valid_answers_at_the_wrong_place(gpu, O, tr):
    """The structural mutations of the host sweep, and a word that is no field element in every kind of section."""
    c = V.case(gpu, O, *tr)
    batch, _ = V.structural_batch(gpu, O, c)
    muts = [m for cls in sorted(batch) for m in batch[cls]]
    for cc in {id(m[2]): m[2] for m in muts}.values():
        mine = [m for m in muts if m[2] is cc]
        slots = [(None, cc.words)] + [(name, words) for name, words, _, _ in mine]
        if cc is c:
            slots += [(f"{kind} word {i} = {value:#x}", V.with_word(c.words, i, value))
                      for kind, i in V.one_index_per_kind(c.words).items() for value in (V.P, 2**64 - 1)]
        slots.append((None, cc.words))
        want = device_equals_host(gpu, cc, [n for n, _ in slots], [as_bytes(w) for _, w in slots])
        assert want[0] == want[-1] == (0, "")
        for (name, _, _, reason), got in zip(mine, want[1:]):
            assert got == (-6, reason), (name, got, reason)
        assert all(code == -5 for code, _ in want[1 + len(mine):-1])


def test_stratified_sweep_of_a_wide_proof(gpu, O):
    """G1Stark (leaves of 285 sponge blocks + 3 words and of 158 full blocks) in chunks of at most 1024 proofs through one verifier,
    then the first chunk again, reversed: nothing leaks between calls."""
    c = V.case(gpu, O, "g1op", G1_ROW)
    clock = V.Clock()
    names, batch = interleaved(c, W.stratified_indices(c.words))
    v = gpu.Verifier(c.stark, c.cfg, c.bits, max_batch=1024)
    try:
        first = None
        for k in range(0, len(batch), 1024):
            want = device_equals_host(gpu, c, names[k:k + 1024], batch[k:k + 1024], verifier=v)
            check_verdicts(c, names[k:k + 1024], want)
            first = first or want
        assert_device_is_host(names[:1024][::-1], v.verify(batch[:1024][::-1]), first[::-1])
    finally:
        v.close()
    print(f"\ng1op stratified: {len(batch)} proofs of {len(c.words)} words, {clock.lap():.1f} s")


def test_slot_boundaries_and_batch_offsets(gpu, O, fq12expu64_case):
    """Fq12ExpU64Stark(16), proved on the device: a proof longer than one slot of the pinned ring.  The words on both sides of every
    slot boundary, the last word before the public inputs and sixteen public inputs, each tampered copy at batch positions 0, 1 and
    last with good proofs between (a proof at position a starts at word a * proof_words of the device buffer)."""
    stark = gpu.Fq12ExpU64Stark(16)
    cfg = stark.config()
    prover = gpu.Prover(stark, cfg, 11)
    try:
        prover.load_trace(fq12expu64_case["trace"], fq12expu64_case["pi"])
        words = prover.prove().words
    finally:
        prover.close()
    clock = V.Clock()
    n = len(words)
    assert n > SLOT_WORDS
    L = W.Layout(words)
    assert (L.ncol, L.npi, L.pow_off) == (9792, 9232, n - 9232 - 1)
    indices = parity_kit.stage_digests(words, O.poseidon_permute, pow_bits=cfg.proof_of_work_bits)["query_indices"]
    idxs = [i for k in range(1, -(-n // SLOT_WORDS)) for i in (k * SLOT_WORDS - 1, k * SLOT_WORDS)]
    idxs += [L.pow_off] + [L.pi_off + (k * (L.npi - 1)) // 15 for k in range(16)]
    assert len(set(idxs)) == len(idxs) and all(i < n for i in idxs) and idxs[-1] == n - 1
    good = as_bytes(words)
    bad = [as_bytes(M.bump(words, i)) for i in idxs]
    want = V.host_verdicts(gpu, stark, cfg, [good] + bad, threads=8)
    assert want[0] == (0, "")
    in_queries = 0
    for i, (code, reason) in zip(idxs, want[1:]):
        lab = W.label_of(words, i)
        assert code == -6, (i, lab, code, reason)
        predicted = W.expected_reason(words, indices, i)
        if predicted is not None:
            in_queries += 1
            assert reason == predicted, (i, lab, reason, predicted)
        elif lab[0] == "public_input":
            assert reason == W.QUOTIENT_MISMATCH, (i, lab, reason)
    assert in_queries >= 2   # the first slot boundary lies among the query answers
    v = gpu.Verifier(stark, cfg, 11, max_batch=5)
    try:
        for i, b, w in zip(idxs, bad, want[1:]):
            got = v.verify([b, b, good, good, b])
            assert got == [w, w, (0, ""), (0, ""), w], (i, W.label_of(words, i), got, w)
    finally:
        v.close()
    print(f"\nfq12expu64: {n} words, {len(idxs)} tampered words at batch positions 0, 1 and 4, {clock.lap():.1f} s after the proof")
