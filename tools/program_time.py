#!/usr/bin/env python3
"""Times the field programs in one process on the GPU box.  On one prover per table, in alternating pairs (program, host_form,
program, host_form, ...), the host clock around
  program    Prover.generate_trace_program(nodes, values, exps): on the Fq12 tables the links are resolved on the device, one launch
             per level, one workgroup per node of that level;
  host_form  program_instances(stark, nodes, values, exps) followed by Prover.generate_trace on its list: what the call replaces
             (the host pool walks every node, then the explicit list runs its chains side by side in one launch);
and the device_tracegen_ms entry of stage_times() after each, for
  the diamond and the x-chain of 16 on Fq12ExpStark(16), an x-chain of 512 and 512 independent nodes on Fq12ExpStark(512).
The x-chains are towers, so Prover.generate_trace_powers (one workgroup walks all levels in ONE launch) is timed as a third member
of the round: the reference point for what fusing levels would buy.  Per case the level count (= launches of the level kernel) and
the nodes per level are recorded, and the SBN_TRACE_TIMING spans of one more call on a prover created under that switch (the
library prints them to stderr): program_levels is the span of all the level launches.  Medians and min-max of --calls rounds (7)
after --warmup rounds (2).  Writes the JSON file and prints one row per case.

    python tools/program_time.py [--out profiles/program_time.json] [--calls 7] [--warmup 2] [--small]
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stderr_of(f):
    """What the library writes to file descriptor 2 while f() runs."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            f()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def rounds(calls, warmup, forms, dev):
    """forms: {name: f}; one round calls every form once, in order: alternating, so drift hits all of them alike."""
    wall, d = {k: [] for k in forms}, {k: [] for k in forms}
    for i in range(warmup + calls):
        for name, f in forms.items():
            t0 = time.perf_counter()
            f()
            if i >= warmup:
                wall[name].append((time.perf_counter() - t0) * 1e3)
                d[name].append(dev())
    return {k: {"host_clock_ms": summary(wall[k]), "device_tracegen_ms": summary(d[k]), "calls": calls, "warmup": warmup} for k in forms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "program_time.json"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--small", action="store_true", help="Fq12ExpStark(16) only")
    args = ap.parse_args()
    if args.calls < 7 or args.warmup < 2:
        raise SystemExit("at least 7 rounds after 2 warm-up rounds")
    import starky_bn254_amd as S
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("program_time.py needs a GPU")
    rng = random.Random(args.seed)
    OUT, ONE = S.NODE_OUTPUT, S.NODE_ONE

    def elems(count):
        return np.array([[w for _ in range(12) for w in S.api._int_limbs(rng.randrange(S.BN_P), 8)] for _ in range(count)], dtype=np.uint32)

    def x_chain(n):
        return np.array([(0, ONE, 0)] + [(OUT | (k - 1), ONE, 0) for k in range(1, n)], dtype=np.uint32)

    exp = np.array([S.api._int_limbs(rng.randrange(1 << 255, 1 << 256), 8)], dtype=np.uint32)
    diamond = np.array([(0, ONE, 0), (0, ONE, 0), (OUT | 0, OUT | 1, 0), (OUT | 2, OUT | 2, 0)], dtype=np.uint32)
    tables = [(16, 13, [("diamond", diamond, 1, None), ("x-chain of 16", x_chain(16), 1, 16)])]
    if not args.small:
        tables.append((512, 18, [("x-chain of 512", x_chain(512), 1, 512),
                                 ("512 independent nodes", np.array([(k, ONE, 0) for k in range(512)], dtype=np.uint32), 512, None)]))
    cases = {}
    for num_io, bits, shapes in tables:
        stark = S.Fq12ExpStark(num_io)
        prover = S.Prover(stark, stark.config(), bits)
        os.environ["SBN_TRACE_TIMING"] = "1"
        try:
            marked = S.Prover(stark, stark.config(), bits)
        finally:
            del os.environ["SBN_TRACE_TIMING"]
        d = prover.describe()
        dev = lambda: prover.stage_times()["device_tracegen_ms"]   # noqa: E731
        for name, nodes, n_values, tower_depth in shapes:
            values = elems(n_values)
            level, depth = S.program_levels(nodes)
            ios, outs = S.program_instances(stark, nodes, values, exp)
            pi = prover.generate_trace(ios[0])
            pi_p, outs_p, ios_p = prover.generate_trace_program(nodes, values, exp)
            assert np.array_equal(pi, pi_p) and np.array_equal(ios[0], ios_p) and np.array_equal(outs, outs_p)
            forms = {"program": lambda: prover.generate_trace_program(nodes, values, exp),
                     "host_form": lambda: prover.generate_trace(S.program_instances(stark, nodes, values, exp)[0][0])}
            if tower_depth:
                pi_t, powers, ios_t = prover.generate_trace_powers(values, exp, tower_depth)
                assert np.array_equal(pi, pi_t) and np.array_equal(ios[0], ios_t) and np.array_equal(outs, powers.reshape(-1, 96))
                forms["powers"] = lambda: prover.generate_trace_powers(values, exp, tower_depth)
            got = rounds(args.calls, args.warmup, forms, dev)
            marked.generate_trace_program(nodes, values, exp)   # warm-up of the marked prover
            spans = {}
            for line in stderr_of(lambda: marked.generate_trace_program(nodes, values, exp)).splitlines():
                if line.startswith("[device tracegen]"):
                    span, ms = line[len("[device tracegen]"):].rsplit("ms", 1)[0].rsplit(None, 1)
                    spans[span.strip()] = float(ms)
            key = f"Fq12ExpStark({num_io}) {name}"
            p, h = got["program"]["host_clock_ms"], got["host_form"]["host_clock_ms"]
            cases[key] = dict(got, nodes=int(len(nodes)), pads=int(num_io - len(nodes)), levels=int(depth), level_launches=int(depth),
                              nodes_per_level=np.bincount(level, minlength=depth).tolist(), program_spans_ms=spans,
                              fq12_host_chain=d.get("fq12_host_chain"), program_minus_host_form_median_ms=p["median"] - h["median"],
                              host_form_spread_ms=h["max"] - h["min"])
            tw = f" | {got['powers']['host_clock_ms']['median']:.2f}" if tower_depth else " | -"
            print(f"| {key} | {depth} | {p['median']:.2f} ({p['min']:.2f}-{p['max']:.2f}) | {h['median']:.2f} ({h['min']:.2f}-{h['max']:.2f}){tw} | "
                  f"{got['program']['device_tracegen_ms']['median']:.2f} | {got['host_form']['device_tracegen_ms']['median']:.2f} | "
                  f"{spans.get('program_levels', float('nan')):.3f} |", flush=True)
        prover.close()
        marked.close()
    out = {"workload": f"seeded Fq12 elements and one seeded 256-bit exponent (seed {args.seed}); {args.calls} alternating rounds per case after "
                       f"{args.warmup} warm-up rounds, every form of a case on the same prover",
           "clock": "host_clock_ms: perf_counter around the whole call; device_tracegen_ms: HIP events on the prover's stream (stage_times), the "
                    "device span of the generate_trace inside the call only; program_spans_ms: the SBN_TRACE_TIMING spans of one call",
           "columns": "| case | levels | program host clock (min-max) | host_form host clock (min-max) | powers host clock | program device | "
                      "host_form device | program_levels span |",
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
