"""Every word of a proof through the two CPU verifiers: the product's host verifier sbn_verify (code AND reason) and the oracle's
independent one.  The proofs are the oracle's, of the inputs test_verifier_gpu.py uses; the map of their words is proof_words.py.
Tampering is of three sorts: +1 on every single word (config_matrix.bump keeps it canonical), a word that is no field element, and
valid answers moved to the wrong place (verifier_sweep.structural_batch).  The device verifier runs the same lists in
test_verifier_sweep_gpu.py.  Every failure names the label of the word."""
import pytest

import config_matrix as M
import proof_words as W
import verifier_sweep as V

CASES = [(t, r) for t in V.SMALL_TABLES for r in V.SMALL_ROWS]
case_id = lambda c: c[0] + "-" + "-".join(str(v) for v in c[1])   # noqa: E731
G1_ROW = (8, 8, 1, 0, 3)


def check_single_word_verdicts(c, idxs, got):
    """got[k]: host verdict of the proof with word idxs[k] bumped."""
    for i, (code, reason) in zip(idxs, got):
        lab = W.label_of(c.words, i)
        assert code == (-5 if i < 12 else -6), (lab, i, code, reason)
        want = W.expected_reason(c.words, c.indices, i)
        if want is not None:
            assert reason == want, (lab, i, reason, want)


def check_oracle_rejects(O, c, idxs):
    for i in idxs:
        assert O.verify(c.kind, c.num_io, M.bump(c.words, i), config=c.ocfg)[0] != 0, ("the oracle accepts", W.label_of(c.words, i), i)


@pytest.mark.parametrize("tr", CASES + [("g1op", G1_ROW)], ids=case_id)
def test_the_word_map_tiles_the_proof(S, O, tr):
    """classify() against the two older maps and against the parity kit's cut of the same words."""
    import test_verifier_gpu as G
    import parity_kit
    c = V.case(S, O, *tr)
    labels = W.classify(c.words)
    assert len(labels) == len(c.words) and all(W.label_of(c.words, i) == lab for i, lab in enumerate(labels))
    L, last = c.layout, c.layout.nqueries - 1
    cut = parity_kit.parse_proof(c.words)
    assert L.query_stride == cut["query_stride"] and L.final_off - L.query_off == len(cut["query_rounds"])
    assert [labels[i][0] for i in M.section_words(c.words).values()] == ["trace_cap", "opening", "final_poly", "fri_eval"][:3 + (L.layers > 0)]
    for name, i in G.query_words(c.words).items():
        kind = "initial_" + name.split("_")[1] if name.startswith("initial") else name
        if name.startswith("fri"):
            kind = "fri_sibling" if name.endswith("sibling") else "fri_eval"
        assert labels[i][0] == kind and (len(labels[i]) < 3 or labels[i][1] == last), (name, labels[i])
    assert labels[11] == ("header", 11) and labels[12] == ("trace_cap", 0) and labels[L.query_off] == ("initial_leaf", 0, 0, 0)
    assert labels[L.final_off - 1][1] == last and labels[L.final_off] == ("final_poly", 0) and labels[-1] == ("pow_witness",)
    assert O.verify(c.kind, c.num_io, c.words, config=c.ocfg) == (0, "") and V.host_verdicts(S, c.stark, c.cfg, [c.words]) == [(0, "")]


@pytest.mark.parametrize("tr", CASES, ids=case_id)
def test_every_word_bumped(S, O, tr):
    c = V.case(S, O, *tr)
    clock, n = V.Clock(), len(c.words)
    got = V.host_verdicts(S, c.stark, c.cfg, (M.bump(c.words, i) for i in range(n)))
    t_host = clock.lap()
    check_single_word_verdicts(c, range(n), got)
    in_queries = sum(W.expected_reason(c.words, c.indices, i) is not None for i in range(n))
    assert in_queries == c.layout.nqueries * c.layout.query_stride
    k, sample = V.oracle_sample(c.words)
    assert 400 <= len(sample) <= 600 + len(W.kind_indices(c.words))
    assert {W.label_of(c.words, i)[0] for i in sample} == set(W.kind_indices(c.words))
    clock.lap()
    check_oracle_rejects(O, c, sample)
    print(f"\n{case_id(tr)}: {n} words bumped ({in_queries} with a predicted reason), host {t_host:.1f} s; oracle every {k}th word = {len(sample)} calls, {clock.lap():.1f} s")


@pytest.mark.parametrize("tr", CASES, ids=case_id)
def test_a_word_that_is_no_field_element(S, O, tr):
    """p and 2^64 - 1 at one word of every label kind: malformed (-5) whichever section holds it."""
    c = V.case(S, O, *tr)
    where = V.one_index_per_kind(c.words)
    assert set(where) == {lab[0] for lab in W.classify(c.words)}
    for value in (V.P, 2**64 - 1):
        got = V.host_verdicts(S, c.stark, c.cfg, [V.with_word(c.words, i, value) for i in where.values()])
        for (kind, i), (code, reason) in zip(where.items(), got):
            assert code == -5, (kind, i, hex(value), code, reason)
            assert kind == "header" or "non-canonical" in reason, (kind, i, reason)
            assert O.verify(c.kind, c.num_io, V.with_word(c.words, i, value), config=c.ocfg)[0] != 0, (kind, i)


@pytest.mark.parametrize("tr", CASES, ids=case_id)
def test_valid_answers_at_the_wrong_place(S, O, tr):
    """The mutations no +1 reaches: both CPU verifiers reject, and the host names the first check the move breaks -- for a move among
    the queries the first tree of the first affected query (or the tree whose path was reordered), for a move inside the trace cap the
    quotient check, since every challenge follows from the cap."""
    c = V.case(S, O, *tr)
    clock = V.Clock()
    batch, skipped = V.structural_batch(S, O, c)
    report = []
    for cls, muts in sorted(batch.items()):
        assert len(muts) >= V.FLOOR, (cls, len(muts), skipped[cls])
        for cc in {id(m[2]): m[2] for m in muts}.values():
            mine = [m for m in muts if m[2] is cc]
            got = V.host_verdicts(S, cc.stark, cc.cfg, [m[1] for m in mine])
            for (name, words, _, want), (code, reason) in zip(mine, got):
                assert (code, reason) == (-6, want), (name, code, reason, want)
                assert O.verify(cc.kind, cc.num_io, words, config=cc.ocfg)[0] != 0, ("the oracle accepts", name)
        own = sum(m[2] is c for m in muts)
        report.append(f"{cls}: {len(muts)} effective ({own} in this proof, {len(muts) - own} in the default row's), {skipped[cls]} skipped")
    print(f"\n{case_id(tr)}: " + "; ".join(report) + f"; {clock.lap():.1f} s")


def test_stratified_sweep_of_a_wide_proof(S, O):
    """G1Stark: leaves of 2283 words (285 sponge blocks + 3) and of 1264 (158 full blocks)."""
    c = V.case(S, O, "g1op", G1_ROW)
    assert (len(c.words), c.layout.ncol, c.layout.nz) == (30346, 2283, 1264)
    clock = V.Clock()
    idxs = W.stratified_indices(c.words)
    kinds = {W.label_of(c.words, i)[0] for i in idxs}
    assert kinds == set(W.kind_indices(c.words)) - {"header"}
    for q in range(c.layout.nqueries):   # every query, tree and sibling level is there
        for t in c.layout.trees:
            hit = {W.label_of(c.words, i) for i in idxs if c.layout.leaf(q, t)[0] <= i < c.layout.leaf(q, t)[1] + 4 * t.nsib}
            assert len([lab for lab in hit if lab[0].endswith("sibling")]) == t.nsib and len(hit) - t.nsib >= min(t.leaf_len, 2), (q, t, hit)
    got = V.host_verdicts(S, c.stark, c.cfg, (M.bump(c.words, i) for i in idxs))
    t_host = clock.lap()
    check_single_word_verdicts(c, idxs, got)
    check_oracle_rejects(O, c, idxs[::10])
    print(f"\ng1op stratified: {len(idxs)} of {len(c.words)} words, host {t_host:.1f} s, oracle on {len(idxs[::10])}: {clock.lap():.1f} s")
