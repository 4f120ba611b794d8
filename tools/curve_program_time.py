#!/usr/bin/env python3
"""Times the curve programs in one process on the GPU box.  On one prover per table and device chain placement
(SBN_TRACEGEN_DEVICE_CHAIN = 1: one lane per node, 2: one wave per node), in alternating pairs (program, host_form, program,
host_form, ...), the host clock around
  program    Prover.generate_trace_curve_program(nodes, points, exps): the links resolved on the device, one level launch and one
             status launch per level, the blinds derived on the host pool meanwhile, the values computed on the device;
  host_form  curve_program_instances(stark, nodes, points, exps) followed by Prover.generate_trace on its list: what the call
             replaces (the host pool walks every node and every blind, then the explicit list runs its chains in one launch);
and the device_tracegen_ms entry of stage_times() after each, on one unit of G1ExpStark(128) and of G2ExpStark(128), for
  128 independent nodes (one level), a 3-level diamond (4 nodes) and an x-chain of 16 (16 levels).
The literals are seeded multiples of the generator (values the library itself derives), the exponents seeded.  Per
case the level count and the nodes per level are recorded, and the SBN_TRACE_TIMING spans of one more call on a prover created
under that switch: curve_program_levels is the span of all the level and status launches, curve_program_values the span from there
to the values.  Medians and min-max of --calls rounds (7) after --warmup rounds (2).  Writes the JSON file and prints one row per
case.

    python tools/curve_program_time.py [--out profiles/curve_program_time.json] [--calls 7] [--warmup 2]
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from program_time import rounds, stderr_of  # noqa: E402


def created_under(env, make):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curve_program_time.json"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    if args.calls < 7 or args.warmup < 2:
        raise SystemExit("at least 7 rounds after 2 warm-up rounds")
    import starky_bn254_amd as S
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("curve_program_time.py needs a GPU")
    rng = random.Random(args.seed)
    OUT, START = S.NODE_OUTPUT, S.NODE_START
    exps = np.array([S.api._int_limbs(rng.randrange(1 << 255, 1 << 256), 8) for _ in range(128)], dtype=np.uint32)
    shapes = [("128 independent nodes", np.array([(g % 9, START, g) for g in range(128)], dtype=np.uint32)),
              ("diamond", np.array([(0, START, 0), (OUT | 0, START, 1), (OUT | 0, 1, 2), (OUT | 1, OUT | 2, 3)], dtype=np.uint32)),
              ("x-chain of 16", np.array([(0, START, 0)] + [(OUT | (k - 1), START, k) for k in range(1, 16)], dtype=np.uint32))]
    cases = {}
    for make in (S.G1ExpStark, S.G2ExpStark):
        stark = make(128)
        # nine literals with no relation to the start candidates: seeded multiples of the generator, as the library itself states them
        gen = np.array([S.generator(stark)], dtype=np.uint32)
        points = S.curve_program_instances(stark, np.array([(0, START, k) for k in range(9)], dtype=np.uint32), gen, exps[100:109])[2]
        for mode in ("1", "2"):
            prover = created_under({"SBN_TRACEGEN_DEVICE_CHAIN": mode}, lambda: S.Prover(stark, stark.config(), 16))
            marked = created_under({"SBN_TRACEGEN_DEVICE_CHAIN": mode, "SBN_TRACE_TIMING": "1"}, lambda: S.Prover(stark, stark.config(), 16))
            placement = prover.describe()["curve_chains"]
            dev = lambda: prover.stage_times()["device_tracegen_ms"]   # noqa: E731
            for name, nodes in shapes:
                level, depth = S.program_levels(nodes)
                ios, outs, values, infinity, choice = S.curve_program_instances(stark, nodes, points, exps)
                pi = prover.generate_trace(ios[0])
                got = prover.generate_trace_curve_program(nodes, points, exps)
                assert np.array_equal(pi, got[0]) and np.array_equal(outs, got[1]) and np.array_equal(values, got[2]) and np.array_equal(ios[0], got[5])
                assert choice == got[4] == 0   # the device tries candidate 0 only: another choice would time the fallback
                forms = {"program": lambda: prover.generate_trace_curve_program(nodes, points, exps),
                         "host_form": lambda: prover.generate_trace(S.curve_program_instances(stark, nodes, points, exps)[0][0])}
                res = rounds(args.calls, args.warmup, forms, dev)
                marked.generate_trace_curve_program(nodes, points, exps)   # warm-up of the marked prover
                spans = {}
                for line in stderr_of(lambda: marked.generate_trace_curve_program(nodes, points, exps)).splitlines():
                    if line.startswith("[device tracegen]"):
                        span, ms = line[len("[device tracegen]"):].rsplit("ms", 1)[0].rsplit(None, 1)
                        spans[span.strip()] = float(ms)
                key = f"{make.__name__}(128) {placement} {name}"
                p, h = res["program"]["host_clock_ms"], res["host_form"]["host_clock_ms"]
                cases[key] = dict(res, nodes=int(len(nodes)), pads=int(128 - len(nodes)), levels=int(depth), level_launches=int(depth), status_launches=int(depth),
                                  nodes_per_level=np.bincount(level, minlength=depth).tolist(), program_spans_ms=spans, curve_chains=placement,
                                  program_minus_host_form_median_ms=p["median"] - h["median"], host_form_spread_ms=h["max"] - h["min"])
                print(f"| {key} | {depth} | {p['median']:.2f} ({p['min']:.2f}-{p['max']:.2f}) | {h['median']:.2f} ({h['min']:.2f}-{h['max']:.2f}) | "
                      f"{res['program']['device_tracegen_ms']['median']:.2f} | {res['host_form']['device_tracegen_ms']['median']:.2f} | "
                      f"{spans.get('curve_program_levels', float('nan')):.3f} | {spans.get('curve_program_values', float('nan')):.3f} |", flush=True)
            prover.close()
            marked.close()
    out = {"workload": f"nine seeded multiples of the generator as literals, seeded 256-bit exponents (seed {args.seed}); {args.calls} alternating rounds per "
                       f"case after {args.warmup} warm-up rounds, both forms of a case on the same prover",
           "clock": "host_clock_ms: perf_counter around the whole call; device_tracegen_ms: HIP events on the prover's stream (stage_times), the "
                    "device span of the generate_trace inside the call only; program_spans_ms: the SBN_TRACE_TIMING spans of one call",
           "columns": "| case | levels | program host clock (min-max) | host_form host clock (min-max) | program device | host_form device | "
                      "curve_program_levels span | curve_program_values span |",
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
