"""A map of a proof's words (layout: include/sbn.h), for the verifier sweeps (test_verifier_sweep_host.py, test_verifier_sweep_gpu.py).
Pure Python over the twelve header words; it generalises query_words() of test_verifier_gpu.py and section_words() of config_matrix.py.

A label is a tuple whose first entry is its KIND:
  ("header", k)                                          ("opening",)
  ("trace_cap", e)  ("z_cap", e)  ("quotient_cap", e)    ("fri_cap", l, e)            e = cap entry (four words each)
  ("initial_leaf", q, t, j)  ("initial_sibling", q, t, s)     query q, initial oracle t: leaf word j / sibling level s
  ("fri_eval", q, l, j)      ("fri_sibling", q, l, s)         query q, FRI layer l: eval word j (value j // 2) / sibling level s
  ("final_poly", j)  ("pow_witness",)  ("public_input", j)

expected_reason() is the verdict a correct verifier gives when ONE word of the query section changes.  Query answers are not absorbed
by the transcript, so challenges and indices stay and the first failing check is fixed by position, in the order of verify_finish
(csrc/verifier.hip): per query, the Merkle paths of the initial oracles in order, then per FRI layer the fold-consistency check of the
one eval the previous layer determines, then that layer's Merkle path."""
from bisect import bisect_right
from collections import namedtuple

import numpy as np

import config_matrix as M

Span = namedtuple("Span", "start length kind coords unit")   # words [start, start + length): label (kind, *coords, offset // unit)
Tree = namedtuple("Tree", "kind number leaf_off leaf_len nsib shift")   # offsets relative to the query's block; kind "initial" / "fri"


class Layout:
    """Offsets of every section of a proof with this header."""

    def __init__(self, words):
        self.nwords = len(words)
        (self.degree_bits, self.ncol, self.nz, self.nq, self.npi, self.cap_h, self.rate_bits, self.layers, self.arity_bits, self.fpl,
         self.nqueries) = M.header(words)
        self.capw, self.lde_bits = 4 << self.cap_h, self.degree_bits + self.rate_bits
        self.widths = [self.ncol] + ([self.nz] if self.nz else []) + [self.nq]
        self.ninit = len(self.widths)
        pos = 12
        self.cap_off = {}
        for name in ["trace_cap"] + (["z_cap"] if self.nz else []) + ["quotient_cap"]:
            self.cap_off[name] = pos
            pos += self.capw
        self.openings_off, self.openings_len = pos, 2 * (2 * self.ncol + 2 * self.nz + self.nq)
        pos += self.openings_len
        self.fri_cap_off = []
        for _ in range(self.layers):
            self.fri_cap_off.append(pos)
            pos += self.capw
        self.query_off = pos
        self.trees, off = [], 0
        for t, w in enumerate(self.widths):
            self.trees.append(Tree("initial", t, off, w, self.lde_bits - self.cap_h, 0))
            off += w + 4 * (self.lde_bits - self.cap_h)
        bits = self.lde_bits
        for l in range(self.layers):
            bits -= self.arity_bits
            self.trees.append(Tree("fri", l, off, 2 << self.arity_bits, bits - self.cap_h, (l + 1) * self.arity_bits))
            off += (2 << self.arity_bits) + 4 * (bits - self.cap_h)
        self.query_stride = off
        self.final_off = self.query_off + self.nqueries * self.query_stride
        self.pow_off = self.final_off + 2 * self.fpl
        self.pi_off = self.pow_off + 1
        assert self.pi_off + self.npi == self.nwords, "the header does not describe a proof of this length"

    def block(self, q):
        """(start, end) of query q's answers."""
        return self.query_off + q * self.query_stride, self.query_off + (q + 1) * self.query_stride

    def leaf(self, q, tree):
        s = self.query_off + q * self.query_stride + tree.leaf_off
        return s, s + tree.leaf_len

    def sibling(self, q, tree, s):
        a = self.query_off + q * self.query_stride + tree.leaf_off + tree.leaf_len + 4 * s
        return a, a + 4

    def spans(self):
        out = [Span(0, 12, "header", (), 1)]
        for name, off in self.cap_off.items():
            out.append(Span(off, self.capw, name, (), 4))
        out.append(Span(self.openings_off, self.openings_len, "opening", None, 0))
        for l, off in enumerate(self.fri_cap_off):
            out.append(Span(off, self.capw, "fri_cap", (l,), 4))
        for q in range(self.nqueries):
            for tr in self.trees:
                a, b = self.leaf(q, tr)
                out.append(Span(a, tr.leaf_len, "initial_leaf" if tr.kind == "initial" else "fri_eval", (q, tr.number), 1))
                if tr.nsib:
                    out.append(Span(b, 4 * tr.nsib, tr.kind + "_sibling", (q, tr.number), 4))
        out.append(Span(self.final_off, 2 * self.fpl, "final_poly", (), 1))
        out.append(Span(self.pow_off, 1, "pow_witness", None, 0))
        if self.npi:
            out.append(Span(self.pi_off, self.npi, "public_input", (), 1))
        return [s for s in out if s.length]


def _label(span, i):
    return (span.kind,) if span.coords is None else (span.kind,) + span.coords + ((i - span.start) // span.unit,)


def classify(words):
    """The label of every word index; the labels tile [0, len(words)) exactly."""
    spans = Layout(words).spans()
    pos = 0
    for s in spans:
        assert s.start == pos, ("sections do not tile the proof", s, pos)
        pos += s.length
    assert pos == len(words), ("sections do not tile the proof", pos, len(words))
    out = [_label(s, i) for s in spans for i in range(s.start, s.start + s.length)]
    assert len(out) == len(words)
    return out


def label_of(words, i, _cache={}):
    """classify(words)[i] without the list (a wide proof has a million words)."""
    key = tuple(int(x) for x in words[:12]) + (len(words),)
    if key not in _cache:
        spans = Layout(words).spans()
        _cache[key] = ([s.start for s in spans], spans)
    starts, spans = _cache[key]
    s = spans[bisect_right(starts, i) - 1]
    assert s.start <= i < s.start + s.length
    return _label(s, i)


def kind_indices(words):
    """{kind: the word indices of that kind, ascending} (ranges)."""
    out = {}
    for s in Layout(words).spans():
        out.setdefault(s.kind, []).append(range(s.start, s.start + s.length))
    return out


QUERY_KINDS = ("initial_leaf", "initial_sibling", "fri_eval", "fri_sibling")


def expected_reason(words, indices, i):
    """The reason string of a correct verifier for a proof that differs from the valid `words` in word i alone; None when word i
    is outside the query section.  indices: the proof's query indices (parity_kit.stage_digests(...)["query_indices"])."""
    lab = label_of(words, i)
    if lab[0] not in QUERY_KINDS:
        return None
    kind, q, n, j = lab
    if kind in ("initial_leaf", "initial_sibling"):
        return f"invalid Merkle proof (initial oracle {n}, query {q})"
    if kind == "fri_eval":
        arity_bits = M.header(words)[8]
        x_index = int(indices[q]) >> (n * arity_bits)   # the query index shifted down by the earlier layers' arity bits
        if j // 2 == x_index & ((1 << arity_bits) - 1):
            return f"FRI fold consistency check failed (query {q}, layer {n})"
    return f"invalid Merkle proof (FRI layer {n}, query {q})"


def reason_of_tree(tree, q):
    """The Merkle message of a path that does not end at its cap entry."""
    return f"invalid Merkle proof ({'initial oracle' if tree.kind == 'initial' else 'FRI layer'} {tree.number}, query {q})"


# ---------------------------------------------------------------- mutations no "+1" reaches: a valid answer at the wrong place
def _swapped(words, a, b, n):
    t = np.array(words, dtype=np.uint64, copy=True)
    t[a:a + n], t[b:b + n] = np.array(words[b:b + n], dtype=np.uint64), np.array(words[a:a + n], dtype=np.uint64)
    return t


QUOTIENT_MISMATCH = "mismatch between evaluation and opening of quotient polynomial"


def structural_mutations(words, indices, limit=12):
    """{class: [(name, mutated words or None, expected host reason)]}: at most `limit` candidates per class, spread over the queries.
    None marks a mutation that leaves the word stream unchanged (a swap of equal values, two queries with one index): callers skip
    it and count the rest.
      a  swap the whole answer blocks of queries i < j: query i then holds the leaf of another index
      b  swap the initial-oracle-0 leaf and path of two queries whose indices agree in the low nsib bits and differ above them: a valid
         path that ends at another cap entry
      c  swap two adjacent sibling digests of one path
      d  swap two entries of the trace cap (the transcript absorbs the cap: every challenge changes, the quotient check fails first)
      e  copy query 0's block over another query's block, and over all of them at once"""
    L = Layout(words)
    w = np.asarray(words, dtype=np.uint64)
    nq, stride = L.nqueries, L.query_stride
    idx = [int(x) for x in indices]
    mark = lambda t: None if np.array_equal(t, w) else t   # noqa: E731
    first_tree_reason = lambda q: reason_of_tree(L.trees[0], q)   # noqa: E731
    out = {}

    def spread(cands):
        if len(cands) <= limit:
            return cands
        return [cands[(k * len(cands)) // limit] for k in range(limit)]

    pairs = [(i, j) for i in range(nq) for j in range(i + 1, nq)]
    out["a"] = [(f"a: blocks of queries {i} and {j}", mark(_swapped(w, L.block(i)[0], L.block(j)[0], stride)), first_tree_reason(i))
                for i, j in spread([p for p in pairs if idx[p[0]] != idx[p[1]]] or pairs[:1])]

    t0 = L.trees[0]
    low = (1 << t0.nsib) - 1
    same_low = [(i, j) for i, j in pairs if idx[i] != idx[j] and (idx[i] & low) == (idx[j] & low)]
    out["b"] = [(f"b: trace leaf and path of queries {i} and {j}", mark(_swapped(w, L.leaf(i, t0)[0], L.leaf(j, t0)[0], t0.leaf_len + 4 * t0.nsib)),
                 first_tree_reason(i)) for i, j in spread(same_low)]

    levels = [(q, tr, s) for q in range(nq) for tr in L.trees for s in range(tr.nsib - 1)]
    out["c"] = [(f"c: siblings {s} and {s + 1} of {tr.kind} {tr.number}, query {q}", mark(_swapped(w, L.sibling(q, tr, s)[0], L.sibling(q, tr, s + 1)[0], 4)),
                 reason_of_tree(tr, q)) for q, tr, s in spread(levels)]

    capn, c0 = 1 << L.cap_h, L.cap_off["trace_cap"]
    entries = spread([(e, (e + 1 + k) % capn) for k, e in enumerate(range(0, capn, max(1, capn // limit))) if (e + 1 + k) % capn != e])
    out["d"] = [(f"d: trace cap entries {e} and {f}", mark(_swapped(w, c0 + 4 * e, c0 + 4 * f, 4)), QUOTIENT_MISMATCH) for e, f in entries]

    b0 = np.array(w[L.block(0)[0]:L.block(0)[1]])
    out["e"] = []
    for q in spread(list(range(1, nq))):
        t = np.array(w, copy=True)
        t[L.block(q)[0]:L.block(q)[1]] = b0
        out["e"].append((f"e: query 0's block over query {q}'s", mark(t), first_tree_reason(q)))
    t = np.array(w, copy=True)
    for q in range(1, nq):
        t[L.block(q)[0]:L.block(q)[1]] = b0
    first = next((q for q in range(1, nq) if idx[q] != idx[0]), 1)
    out["e"].append(("e: query 0's block over every other query's", mark(t), first_tree_reason(first)))
    return out


def stratified_indices(words, blocks=8, stride=16):
    """The thinned sweep of a wide proof: for every query and tree the first and the last leaf word, one word in each of `blocks` evenly
    spaced sponge blocks (eight words each) and one word of every sibling level; every `stride`-th word of the caps, the openings and
    the final polynomial; the proof-of-work witness.  Sorted, without repeats."""
    L = Layout(words)
    out = {L.pow_off}
    for q in range(L.nqueries):
        for tr in L.trees:
            a, b = L.leaf(q, tr)
            nblocks = -(-tr.leaf_len // 8)
            out.update((a, b - 1))
            for k in range(blocks):
                blk = (k * (nblocks - 1)) // max(blocks - 1, 1)
                out.add(min(a + 8 * blk + (k + q) % 8, b - 1))   # another lane of the sponge's rate in every block
            for s in range(tr.nsib):
                out.add(L.sibling(q, tr, s)[0] + (s + q) % 4)
    for off in list(L.cap_off.values()) + L.fri_cap_off:
        out.update(range(off, off + L.capw, stride))
    out.update(range(L.openings_off, L.openings_off + L.openings_len, stride))
    out.update(range(L.final_off, L.pow_off, stride))
    return sorted(out)
