#!/usr/bin/env python3
"""Time of a proof whose trace is held as SEPARATE host columns (the reference's Vec<PolynomialValues<F>>), G1ExpStark(128)
seed 1, all forms in ONE process, alternating after a warm-up of each, a host clock around calls that return finished proofs:
  1  np.concatenate of the column list (the stand-in for the Rust shim's flatten) + prove_host_trace, the two parts timed apart
  2  prove_host_columns on the same list, and on a ColumnTable built from it once (the list form builds the pointer table of 1676
     arrays in Python on every call; a Rust caller's table is a map over a Vec)
  3  the same with reduce=True, on the canonical trace and on one with 1 % of its words non-canonical (p added)
  4  8 units through BatchProver.prove_host_traces at inflight 1, 2 and 3 beside 8 sequential prove_host_trace calls (the same
     columns 8 times, so host memory stays at one trace)
Forms 1 to 3 and the sequential calls of 4 alternate on ONE live prover; each batch prover is then created, measured and closed on
its own, so that no measurement shares the process with contexts it does not use.  The rounds run in 3 groups; every form reports the median over all rounds and the medians of the groups, and the spread of
prove_host_trace's group medians (max - min) is the yardstick the column forms are held against: they move the same bytes as the
memcpy they replace.  Writes profiles/host_columns_time.json and prints it.
usage: host_columns_time.py [rounds=10] [output=profiles/host_columns_time.json]"""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import starky_bn254_amd as S
import oracle_lib as O          # seeded input generator only

GL_P = 0xFFFFFFFF00000001
GROUPS, UNITS = 3, 8
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
stark = S.G1ExpStark(128); cfg = stark.config()
ios, _ = O.g1exp_inputs(128, 1)
trace, pi = stark.generate_trace_and_public_inputs(ios)
trace = np.ascontiguousarray(trace, dtype=np.uint64)
cols = [None] * trace.shape[0]
for c in np.random.default_rng(0).permutation(trace.shape[0]):   # one allocation per column, allocated in shuffled order
    cols[c] = trace[c].copy()
rng = np.random.default_rng(1)
dirty, planted = [], 0
for c in cols:                                                # 1 % of the words: p added where the sum stays below 2^64
    d = c.copy()
    at = (rng.random(len(d)) < 0.01) & (d < np.uint64(2**64 - GL_P))
    d[at] += np.uint64(GL_P)
    planted += int(at.sum())
    dirty.append(d)
digests = set()


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def note(proof):
    digests.add(hashlib.sha256(proof.to_bytes()).hexdigest())


p = S.Prover(stark, cfg, 16)
table, dirty_table = S.ColumnTable(cols), S.ColumnTable(dirty)
t = {}


def add(name, ms):
    t.setdefault(name, [[] for _ in range(GROUPS)])[group].append(ms)


def one_round():
    ms, flat = clock(lambda: np.concatenate(cols).reshape(trace.shape))
    add("concatenate", ms)
    ms2, proof = clock(lambda: p.prove_host_trace(flat, pi)); note(proof)
    add("prove_host_trace", ms2); add("concatenate_then_prove_host_trace", ms + ms2)
    del flat
    ms, proof = clock(lambda: p.prove_host_columns(cols, pi)); note(proof)
    add("prove_host_columns", ms)
    ms, proof = clock(lambda: p.prove_host_columns(table, pi)); note(proof)
    add("prove_host_columns_table", ms)
    add("column_table_build", clock(lambda: S.ColumnTable(cols))[0])
    ms, (proof, red) = clock(lambda: p.prove_host_columns(table, pi, reduce=True)); note(proof)
    assert red == 0
    add("prove_host_columns_reduce_canonical", ms)
    ms, (proof, red) = clock(lambda: p.prove_host_columns(dirty_table, pi, reduce=True)); note(proof)
    assert red == planted
    add("prove_host_columns_reduce_1pct", ms)


def sequential_round():
    ms, proofs = clock(lambda: [p.prove_host_trace(trace, pi) for _ in range(UNITS)])
    add("sequential_8_prove_host_trace", ms)
    for pr in proofs:
        note(pr)


def batch_round(b, k):
    ms, proofs = clock(lambda: b.prove_host_traces([table] * UNITS, [pi] * UNITS))
    add(f"prove_host_traces_8_inflight{k}", ms)
    for pr in proofs:
        note(pr)


batch_rounds = max(1, rounds // 3)
try:
    group = 0
    one_round(); sequential_round()                           # warm-up of every form
    t.clear()
    for group in range(GROUPS):
        for _ in range(rounds):
            one_round()
        for _ in range(batch_rounds):
            sequential_round()
finally:
    p.close()
for k in (1, 2, 3):
    b = S.BatchProver(stark, cfg, 16, inflight=k)
    try:
        group = 0
        batch_round(b, k)                                     # warm-up
        t.pop(f"prove_host_traces_8_inflight{k}")
        for group in range(GROUPS):
            for _ in range(batch_rounds):
                batch_round(b, k)
    finally:
        b.close()

out = {"table": "G1ExpStark(128)", "seed": 1, "rounds_per_group": rounds, "groups": GROUPS, "units": UNITS, "unit": "ms", "trace_bytes": int(trace.nbytes),
       "words_planted_1pct": planted, "host_threads": S.api.settings_check().get("host_threads")}
for name, groups in t.items():
    flat = [x for g in groups for x in g]
    out[name] = {"median": round(statistics.median(flat), 3), "min": round(min(flat), 3), "max": round(max(flat), 3),
                 "group_medians": [round(statistics.median(g), 3) for g in groups]}
gm = out["prove_host_trace"]["group_medians"]
out["prove_host_trace_spread_of_group_medians"] = round(max(gm) - min(gm), 3)
for name in ("prove_host_columns", "prove_host_columns_table", "prove_host_columns_reduce_canonical"):
    out[name + "_minus_prove_host_trace"] = round(out[name]["median"] - out["prove_host_trace"]["median"], 3)
    out[name + "_within_spread"] = out[name]["median"] - out["prove_host_trace"]["median"] <= max(gm) - min(gm)
for k in (1, 2, 3):
    out[f"inflight{k}_over_sequential"] = round(out[f"prove_host_traces_8_inflight{k}"]["median"] / out["sequential_8_prove_host_trace"]["median"], 4)
out["proof_sha256"] = sorted(digests)
committed = json.load(open(os.path.join(ROOT, "tests", "golden", "proof_digests.json")))["g1exp_io128_seed1"]["proof_sha256"]
out["equals_committed_digest"] = sorted(digests) == [committed]      # the oracle's digest of this proof, every form and unit
line = json.dumps(out)
with open(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "host_columns_time.json"), "w") as f:
    f.write(line + "\n")
print(line, flush=True)
sys.exit(0 if out["equals_committed_digest"] else 1)
