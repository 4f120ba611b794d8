#!/usr/bin/env python3
"""Time of a proof whose trace is held ROW-major on the host (the reference's `rows` in front of its `transpose`), G1ExpStark(128)
seed 1, all forms on ONE live prover in ONE process, alternating, a host clock around calls that return finished proofs; medians of
`rounds` after `warmups` rounds of every form:
  1  prove_host_rows in main-row mode: 398 of 1,676 columns cross PCIe (209 MB), the derived columns are written on the device
  2  prove_host_rows in whole-row mode: all 1,676 columns cross (879 MB), the device only transposes and checks
  3  trace_from_rows_host (transposition and derived columns on the host pool) + prove_host_trace, the two parts timed apart: what
     the holder of main rows pays without the row-major calls
  4  prove_host_columns on ready columns (a ColumnTable built once): no transposition anywhere, the floor for 879 MB
The host pool runs on 16 threads unless SBN_HOST_THREADS says otherwise (form 3 is host work: a pool wider than the CPUs the process
may use slows it down and widens its spread).  Writes profiles/host_rows_time.json and prints it.
usage: host_rows_time.py [rounds=20] [warmups=3] [output=profiles/host_rows_time.json]"""
import hashlib
import json
import os
import statistics
import sys
import time

os.environ.setdefault("SBN_HOST_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import starky_bn254_amd as S
import oracle_lib as O          # seeded input generator only

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warmups = int(sys.argv[2]) if len(sys.argv) > 2 else 3
stark = S.G1ExpStark(128); cfg = stark.config()
ios, _ = O.g1exp_inputs(128, 1)
trace, pi = stark.generate_trace_and_public_inputs(ios)
trace = np.ascontiguousarray(trace, dtype=np.uint64)
main = np.ascontiguousarray(trace[:stark.num_main_columns].T)
whole = np.ascontiguousarray(trace.T)
main_table, whole_table, col_table = S.RowTable(main), S.RowTable(whole), S.ColumnTable(trace)
digests = set()
t = {}


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def add(name, ms, proof=None):
    t.setdefault(name, []).append(ms)
    if proof is not None:
        digests.add(hashlib.sha256(proof.to_bytes()).hexdigest())


p = S.Prover(stark, cfg, 16)


def one_round():
    ms, proof = clock(lambda: p.prove_host_rows(main_table, pi))
    add("prove_host_rows_main", ms, proof)
    ms, proof = clock(lambda: p.prove_host_rows(whole_table, pi))
    add("prove_host_rows_whole", ms, proof)
    ms, flat = clock(lambda: S.trace_from_rows_host(stark, main_table))
    add("trace_from_rows_host", ms)
    ms2, proof = clock(lambda: p.prove_host_trace(flat, pi))
    add("prove_host_trace", ms2, proof); add("trace_from_rows_host_then_prove_host_trace", ms + ms2)
    del flat
    ms, proof = clock(lambda: p.prove_host_columns(col_table, pi))
    add("prove_host_columns", ms, proof)
    ms, _ = clock(lambda: p.load_trace_rows(main_table, pi))
    add("load_trace_rows_main", ms)
    ms, _ = clock(lambda: p.load_trace_rows(whole_table, pi))
    add("load_trace_rows_whole", ms)


try:
    for _ in range(warmups):
        one_round()
    t.clear()
    for _ in range(rounds):
        one_round()
finally:
    p.close()

out = {"table": "G1ExpStark(128)", "seed": 1, "rounds": rounds, "warmups": warmups, "unit": "ms", "main_row_bytes": int(main.nbytes), "whole_row_bytes": int(whole.nbytes),
       "host_threads": S.api.settings_check().get("host_threads")}
for name, xs in t.items():
    out[name] = {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}
out["proof_sha256"] = sorted(digests)
committed = json.load(open(os.path.join(ROOT, "tests", "golden", "proof_digests.json")))["g1exp_io128_seed1"]["proof_sha256"]
out["equals_committed_digest"] = sorted(digests) == [committed]      # the oracle's digest of this proof, every form
line = json.dumps(out)
with open(sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "host_rows_time.json"), "w") as f:
    f.write(line + "\n")
print(line, flush=True)
sys.exit(0 if out["equals_committed_digest"] else 1)
