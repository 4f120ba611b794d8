"""The cases of test_split_matrix_gpu.py: every kind of table the split prover (sbn_split_prover_*) accepts, at the smallest height
at which it exists, over every world size that height admits; the edge shapes of the column dealing (prover_ctx.hpp ColShare)
each (table, world) reaches; and the helpers that run the ranks of a local group as threads which are always joined.

A table row is (id, stark constructor name, constructor arguments, rows, witness, worlds):
  witness "load"     -- a host trace through sbn_split_prover_load_trace, reference = the CPU oracle's proof (O.prove);
  witness "generate" -- an instance list through sbn_split_prover_generate_trace, reference = the proof of a single-GPU Prover
                        on the same list (which test_gpu_parity.py and test_config_matrix_gpu.py pin to the oracle)."""
import contextlib
import os
import threading

import numpy as np

from starky_bn254_amd import split

BLOCK = 64                     # columns per ownership block (prover.hip SPLIT_BLOCK)
ALL_WORLDS = (2, 4, 8, 16)
NO_PI = np.zeros(0, dtype=np.uint64)

TABLES = [
    ("g1op-512", "G1Stark", (), 512, "load", ALL_WORLDS),
    ("g1op-1024", "G1Stark", (), 1024, "load", ALL_WORLDS),
    ("modular-512", "ModularStark", (), 512, "load", ALL_WORLDS),
    ("fq12mul-512", "Fq12Stark", (), 512, "load", ALL_WORLDS),
    ("fq12expu64-4", "Fq12ExpU64Stark", (4,), 512, "generate", ALL_WORLDS),   # the wide table at its minimum height
    ("fqexp-128", "FqExpStark", (128,), 1 << 16, "generate", (16,)),          # 15 trace blocks: rank 15 of 16 owns none
    ("g2exp-128", "G2ExpStark", (128,), 1 << 16, "generate", (4,)),           # the two planes at 2^16 rows
]
TABLE_WORLDS = [(t[0], w) for t in TABLES for w in t[5]]
# (oracle kind name, oracle input generator name, seed) of the loaded tables: the sizes and seeds of test_gpu_parity.py
LOADED = {"g1op-512": ("AIR_G1_OP", "g1op_inputs", 0), "g1op-1024": ("AIR_G1_OP", "g1op_inputs", 3),
          "modular-512": ("AIR_MODULAR", "modular_inputs", 6), "fq12mul-512": ("AIR_FQ12_MUL", "fq12mul_inputs", 7)}
# (oracle input generator name, seed) of the generated tables
GENERATED = {"fq12expu64-4": ("fq12expu64_inputs", 5), "fqexp-128": ("fqexp_inputs", 4), "g2exp-128": ("g2exp_inputs", 2)}

NO_TRACE_BLOCK, NO_Z_BLOCK, PARTIAL_INSIDE = "a rank without a trace block", "a rank without a Z block", "a partial last block on a rank other than the last"
EDGES = (NO_TRACE_BLOCK, NO_Z_BLOCK, PARTIAL_INSIDE)


def table(name):
    return next(t for t in TABLES if t[0] == name)


def make_stark(S, name):
    _, cls, args, _, _, _ = table(name)
    return getattr(S, cls)(*args)


def shares(stark, cfg, world):
    """[(own trace columns, own Z columns)] of every rank, from the table's real column counts."""
    C, Z = stark.num_columns, stark.num_permutation_zs(cfg)
    return [(split.own_columns(C, world, r, BLOCK), split.own_columns(Z, world, r, BLOCK)) for r in range(world)]


def owner_of_last_block(total, world):
    return (-(-total // BLOCK) - 1) % world


def edge_shapes(stark, cfg, world):
    """The edges of the column dealing this (table, world) reaches."""
    own = shares(stark, cfg, world)
    out = set()
    if any(c == 0 for c, _ in own):
        out.add(NO_TRACE_BLOCK)
    if any(z == 0 for _, z in own):
        out.add(NO_Z_BLOCK)
    for total in (stark.num_columns, stark.num_permutation_zs(cfg)):
        if total % BLOCK and owner_of_last_block(total, world) != world - 1:
            out.add(PARTIAL_INSIDE)
    return out


@contextlib.contextmanager
def switches(env):
    """The SBN_* switches `env` in the environment while a transport or a prover is created (both read them at creation), restored
    afterwards: what tracegen_edges.placement does for a single-GPU Prover."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# a rank that waits for another gives up after this long (SBN_COMM_TIMEOUT_S, read when the group and the provers are created), so
# that a wrong exchange plan fails the test instead of hanging it; the threads are joined a little later than that
TIMEOUT = {"SBN_COMM_TIMEOUT_S": "60"}
JOIN_S = 120


def on_ranks(world, fn, group=None):
    """fn(rank) on one thread per rank; every thread is joined with a timeout and none may be left alive.  -> the list of results,
    an exception in place of the result of a rank that raised (which also aborts `group`, releasing the ranks that wait for it)."""
    res = [None] * world

    def go(r):
        try:
            res[r] = fn(r)
        except Exception as e:  # noqa: BLE001
            res[r] = e
            if group is not None:
                group.abort()
    th = [threading.Thread(target=go, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=JOIN_S)
    assert not any(t.is_alive() for t in th), "a rank hangs"
    return res


class Ranks:
    """`world` split provers of one local group on the current device, created under the short transport timeout.  Creation runs
    no collective, so the provers are made one after the other on the calling thread; each() runs a call on all of them side by side."""

    def __init__(self, stark, cfg, degree_bits, world):
        self.world, self.provers = world, []
        sb, rb = split.exchange_bytes(stark, cfg, degree_bits, world)
        with switches(TIMEOUT):
            self.group = split.LocalGroup(world, sb, rb)
            try:
                for r in range(world):
                    self.provers.append(split.SplitProver(stark, cfg, degree_bits, transport=self.group.comms[r]))
            except Exception:
                self.close()
                raise

    def each(self, fn, collective=True):
        """fn(prover, rank) on every rank; -> results, exceptions in place (see on_ranks).  collective=False: a call that meets no
        other rank, so a rank that raises leaves the group usable."""
        return on_ranks(self.world, lambda r: fn(self.provers[r], r), self.group if collective else None)

    def prove(self):
        """One proof by all ranks; raises the first rank's exception."""
        out = self.each(lambda p, r: p.prove())
        for x in out:
            if isinstance(x, Exception):
                raise x
        return out

    def close(self):
        for p in self.provers:
            p.close()
        self.provers = []
        self.group.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
