#!/usr/bin/env python3
"""Time of a proof whose trace starts in HOST memory, G1ExpStark(128) seed 1, four forms in ONE process, alternating after a
warm-up of each, a host clock around calls that return a finished proof:
  A  load_trace + prove on a live prover          (the two-step path: host check, one synchronous copy, then the proof)
  B  prove_host_trace on a live prover            (the upload inside the trace commitment, the check on the device)
  C  prove(stark, config, trace, pi), cache off   (the one-shot call: context created and destroyed per call)
  D  the same with the context cache on           (second and later calls; every round re-enables the cache and makes one
                                                   untimed call first, because turning the cache off for C releases it)
Prints one JSON line: median / min / max of each form in ms and the proofs' sha256 (all equal to the committed oracle digest).
usage: one_shot_time.py [rounds=10]"""
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

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
stark = S.G1ExpStark(128); cfg = stark.config()
ios, _ = O.g1exp_inputs(128, 1)
trace, pi = stark.generate_trace_and_public_inputs(ios)
trace = np.ascontiguousarray(trace, dtype=np.uint64)
pa, pb = S.Prover(stark, cfg, 16), S.Prover(stark, cfg, 16)
digests = set()


def timed(f):
    t0 = time.perf_counter()
    proof = f()
    dt = (time.perf_counter() - t0) * 1e3
    digests.add(hashlib.sha256(proof.to_bytes()).hexdigest())
    return dt


def form_a():
    pa.load_trace(trace, pi)
    return pa.prove()


def form_d_round():
    S.prove_cache_configure(1 << 36)
    S.prove(stark, cfg, trace, pi)                      # untimed: creates the context the timed call finds
    dt = timed(lambda: S.prove(stark, cfg, trace, pi))
    stats = S.prove_cache_stats()
    S.prove_cache_configure(0)
    return dt, stats


S.prove_cache_configure(0)
try:
    for f in (form_a, lambda: pb.prove_host_trace(trace, pi), lambda: S.prove(stark, cfg, trace, pi)):   # warm-up of each form
        timed(f)
    form_d_round()
    t = {"A": [], "B": [], "C": [], "D": []}
    hits = 0
    for _ in range(rounds):
        t["A"].append(timed(form_a))
        t["B"].append(timed(lambda: pb.prove_host_trace(trace, pi)))
        t["C"].append(timed(lambda: S.prove(stark, cfg, trace, pi)))
        dt, stats = form_d_round()
        t["D"].append(dt); hits = stats["hits"]
finally:
    S.prove_cache_configure(0)
    pa.close(); pb.close()
names = {"A": "load_trace_then_prove", "B": "prove_host_trace", "C": "one_shot_cache_off", "D": "one_shot_cache_on"}
out = {"table": "G1ExpStark(128)", "seed": 1, "rounds": rounds, "unit": "ms", "cache_hits": hits, "context_bytes": stats["bytes_resident"],
       "host_threads": S.api.settings_check().get("host_threads")}
for k, v in t.items():
    out[names[k]] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
out["proof_sha256"] = sorted(digests)
committed = json.load(open(os.path.join(ROOT, "tests", "golden", "proof_digests.json")))["g1exp_io128_seed1"]["proof_sha256"]
out["equals_committed_digest"] = sorted(digests) == [committed]      # the oracle's digest of this proof
print(json.dumps(out), flush=True)
sys.exit(0 if out["equals_committed_digest"] else 1)
