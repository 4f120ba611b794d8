#!/usr/bin/env python3
"""Times the 16-node final exponentiation (include/sbn.h, "Mapped links and the final exponentiation") in one process on the GPU
box.  On one prover of Fq12ExpU64Stark(16), in alternating rounds (program, host_form, prove, program, host_form, prove, ...), the
host clock around
  program    Prover.generate_trace_program(nodes, values, exps) with the mapped nodes of S.final_exponentiation: the links and their
             Frobenius maps are resolved on the device, one launch per level and a pre-pass in front of every level with a mapped
             operand;
  host_form  program_instances(stark, nodes, values, exps) followed by Prover.generate_trace on its list: the host pool walks the
             sixteen nodes, then the explicit list runs its chains side by side in one launch;
  prove      Prover.prove() on the trace the round loaded;
and, on a batch prover of Fq12ExpU64Stark(128), BatchProver.prove_final_exponentiations for --inputs (8) inputs, which are one unit
of 128 instances.  Medians and min-max of --calls rounds (7) after --warmup rounds (2).  Writes the JSON file and prints one row per
form.

    python tools/final_exp_time.py [--out profiles/final_exp_time.json] [--calls 7] [--warmup 2] [--inputs 8]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def rounds(calls, warmup, forms):
    """forms: {name: f}; one round calls every form once, in order: alternating, so drift hits all of them alike."""
    wall = {k: [] for k in forms}
    for i in range(warmup + calls):
        for name, f in forms.items():
            t0 = time.perf_counter()
            f()
            if i >= warmup:
                wall[name].append((time.perf_counter() - t0) * 1e3)
    return {k: {"host_clock_ms": summary(wall[k]), "calls": calls, "warmup": warmup} for k in forms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "final_exp_time.json"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inputs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    if args.calls < 7 or args.warmup < 2:
        raise SystemExit("at least 7 rounds after 2 warm-up rounds")
    import starky_bn254_amd as S
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("final_exp_time.py needs a GPU")
    rng = random.Random(args.seed)
    fs = np.array([[w for _ in range(12) for w in S.api._int_limbs(rng.randrange(S.BN_P), 8)] for _ in range(args.inputs)], dtype=np.uint32)

    stark = S.Fq12ExpU64Stark(16)
    pg = S.Program(stark)
    S.final_exponentiation(pg, fs[0])
    nodes, values, exps = pg.arrays()
    level, depth = S.program_levels(nodes)
    prover = S.Prover(stark, stark.config(), 11)
    ios, outs = S.program_instances(stark, nodes, values, exps)
    pi = prover.generate_trace(ios[0])
    pi_p, outs_p, ios_p = prover.generate_trace_program(nodes, values, exps)
    assert np.array_equal(pi, pi_p) and np.array_equal(ios[0], ios_p) and np.array_equal(outs, outs_p)
    one = rounds(args.calls, args.warmup, {"program": lambda: prover.generate_trace_program(nodes, values, exps),
                                           "host_form": lambda: prover.generate_trace(S.program_instances(stark, nodes, values, exps)[0][0]),
                                           "prove": lambda: prover.prove()})
    d = prover.describe()
    prover.close()

    big = S.Fq12ExpU64Stark(128)
    bp = S.BatchProver(big, big.config(), 14)
    try:
        proofs, results, _ = bp.prove_final_exponentiations(fs)
        assert np.array_equal(S.verify_final_exponentiations(big, big.config(), proofs, fs), results)
        batch = rounds(args.calls, args.warmup, {"prove_final_exponentiations": lambda: bp.prove_final_exponentiations(fs)})
    finally:
        bp.close()

    cases = {"Fq12ExpU64Stark(16) final exponentiation": dict(one, nodes=int(len(nodes)), levels=int(depth),
                                                              nodes_per_level=np.bincount(level, minlength=depth).tolist(),
                                                              mapped_operands=int(np.count_nonzero(nodes[:, 3] & 0xFF) + np.count_nonzero(nodes[:, 3] >> 8)),
                                                              fq12_host_chain=d.get("fq12_host_chain")),
             f"Fq12ExpU64Stark(128) {args.inputs} final exponentiations": dict(batch, nodes=16 * args.inputs, units=len(proofs))}
    for key, forms in cases.items():
        for name, v in forms.items():
            if isinstance(v, dict) and "host_clock_ms" in v:
                h = v["host_clock_ms"]
                print(f"| {key} | {name} | {h['median']:.2f} ({h['min']:.2f}-{h['max']:.2f}) |", flush=True)
    out = {"workload": f"seeded Fq12 elements (seed {args.seed}); {args.calls} alternating rounds per form after {args.warmup} warm-up rounds, the three "
                       "forms of the one-unit case on the same prover",
           "clock": "host_clock_ms: perf_counter around the whole call",
           "columns": "| case | form | host clock median (min-max) ms |",
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
