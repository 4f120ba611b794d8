"""What test_verifier_sweep_host.py (CPU) and test_verifier_sweep_gpu.py (device) share: the proofs they sweep, the host verdicts that
are the device's reference, and the lists of tampered copies.  The word map itself is proof_words.py."""
import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import config_matrix as M
import parity_kit
import proof_words as W

P = 0xFFFFFFFF00000001
NO_PI = np.zeros(0, dtype=np.uint64)
SMALL_ROWS = [(8, 8, 1, 0, 3), (6, 16, 2, 3, 28)]
SMALL_TABLES = ["lookup", "flags"]
FLOOR = 8   # effective mutations every structural class keeps per proof

_tables, _cases = {}, {}


def table(S, O, name):
    """(stark, oracle kind, num_io, trace): the inputs of test_verifier_gpu.py."""
    if name not in _tables:
        if name == "lookup":
            ins, tab = O.lookup_inputs(512, 9)
            _tables[name] = (S.LookupStark(), O.AIR_LOOKUP, 0, O.lookup_trace(ins, tab))
        elif name == "flags":
            limbs, _ = O.flags_inputs(2, 28)
            _tables[name] = (S.FlagStark(2), O.AIR_FLAGS, 2, O.flags_trace(limbs))
        else:
            pts, _ = O.g1op_inputs(512, 0)
            _tables[name] = (S.G1Stark(), O.AIR_G1_OP, 0, O.g1op_trace(pts))
    return _tables[name]


class Case:
    """An oracle proof with everything the sweeps ask of it; made once per (table, row) and never changed."""

    def __init__(self, S, O, name, row):
        self.name, self.row = name, row
        self.stark, self.kind, self.num_io, trace = table(S, O, name)
        self.bits = trace.shape[1].bit_length() - 1
        self.cfg, self.ocfg = M.make_config(S, row), row + (True,)
        self.words = O.prove(self.kind, self.num_io, trace, NO_PI, config=self.ocfg)[0]
        self.words.setflags(write=False)
        self.indices = parity_kit.stage_digests(self.words, O.poseidon_permute, pow_bits=row[1])["query_indices"]
        self.layout = W.Layout(self.words)

    def with_words(self, words, indices):
        """The same table and config around a proof made elsewhere (the device prover's)."""
        self.words, self.indices, self.layout = words, indices, W.Layout(words)
        return self


def case(S, O, name, row):
    if (name, row) not in _cases:
        _cases[(name, row)] = Case(S, O, name, row)
    return _cases[(name, row)]


def host_verdicts(S, stark, cfg, batch, threads=16):
    """(code, reason) of sbn_verify for every proof of the batch (an iterable of word arrays or byte strings, consumed lazily); the
    message is read on the thread that made the call."""
    L = S.lib()

    def one(words):
        b = words if isinstance(words, bytes) else np.asarray(words, dtype="<u8").tobytes()
        rc = L.sbn_verify(C.byref(stark._d), C.byref(cfg._c), b, len(b))
        return (rc, L.sbn_last_error().decode() if rc else "")
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, batch))


def with_word(words, i, value):
    t = np.array(words, dtype=np.uint64, copy=True)
    t[i] = value
    return t


def oracle_sample(words, n_calls=500):
    """Every k-th word index, k chosen for about n_calls of them, plus the first index of every label kind the stride misses."""
    k = max(1, len(words) // n_calls)
    picked = set(range(0, len(words), k))
    for kind, ranges in W.kind_indices(words).items():
        if not any(i in picked for r in ranges for i in r):
            picked.add(ranges[0][0])
    return k, sorted(picked)


def one_index_per_kind(words):
    """{kind: a word index of it}: the middle word of the kind's middle stretch (a middle query's, where the kind is per query)."""
    out = {}
    for kind, ranges in W.kind_indices(words).items():
        r = ranges[len(ranges) // 2]
        out[kind] = r[len(r) // 2]
    return out


def effective(cands):
    """(kept, skipped): the mutations that change the word stream, and how many did not."""
    kept = [c for c in cands if c[1] is not None]
    return kept, len(cands) - len(kept)


def structural_batch(S, O, c, limit=12):
    """{class: [(name, words, config, expected host reason)]} for the proof of case c, every class with at least FLOOR effective
    mutations.  A proof with three queries has three pairs of queries and two other blocks: where a class finds fewer than FLOOR in
    the proof itself, the table's default-row proof (84 queries) supplies the rest, under its own config."""
    out, skipped = {}, {}
    own = W.structural_mutations(c.words, c.indices, limit)
    for cls, cands in own.items():
        kept, skipped[cls] = effective(cands)
        out[cls] = [(f"{c.name} {c.row} {n}", w, c, r) for n, w, r in kept]
    if any(len(v) < FLOOR for v in out.values()):
        d = case(S, O, c.name, M.DEFAULT)
        more = W.structural_mutations(d.words, d.indices, limit)
        for cls in out:
            if len(out[cls]) < FLOOR:
                kept, sk = effective(more[cls])
                skipped[cls] += sk
                out[cls] += [(f"{d.name} {d.row} {n}", w, d, r) for n, w, r in kept]
    return out, skipped


class Clock:
    def __init__(self):
        self.t = time.perf_counter()

    def lap(self):
        now = time.perf_counter()
        dt, self.t = now - self.t, now
        return dt
