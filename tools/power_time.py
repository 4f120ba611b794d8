#!/usr/bin/env python3
"""Times the field powers and power towers in one process on the GPU box.  For one unit of FqExpStark(128), Fq12ExpStark(16) and
Fq12ExpU64Stark(16), at depth 1 (num_io independent powers) and depth 3 (num_io // 3 towers, the rest pads), the host clock around
  powers     Prover.generate_trace_powers(bases, exps, depth): on the Fq12 tables one workgroup per tower links and walks its levels
             on the device; on FqExpStark the call walks the towers on the host pool itself;
  host_form  power_instances(stark, bases, exps, depth) followed by Prover.generate_trace on its list: what the call replaces, and
             the honest comparison (a depth-d tower serialises d chains per workgroup, the explicit list runs them side by side);
and the device_tracegen_ms entry of stage_times() after each.  Then BatchProver.prove_bn_x_powers of --inputs Fq12 elements beside
BatchProver.prove_ios on the same units already at hand.  Medians and min-max of --calls calls (7) after --warmup calls (2) of each
form.  Bases are seeded, the exponents BN_X on the u64 table and a seeded 256-bit one elsewhere.  Writes the JSON file and prints
one row per case.

    python tools/power_time.py [--out profiles/power_time.json] [--calls 7] [--warmup 2] [--inputs 1000]
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

TABLES = [("FqExpStark", 128, 16, 1), ("Fq12ExpStark", 16, 13, 12), ("Fq12ExpU64Stark", 16, 11, 12)]   # class, instances, degree bits, coefficients


def timed(calls, warmup, f, dev=None):
    wall, d = [], []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        f()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            if dev:
                d.append(dev())
    out = {"host_clock_ms": {"median": statistics.median(wall), "min": min(wall), "max": max(wall)}, "calls": len(wall), "warmup": warmup}
    if d:
        out["device_tracegen_ms"] = {"median": statistics.median(d), "min": min(d), "max": max(d)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_time.json"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inputs", type=int, default=1000)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    if args.calls < 7 or args.warmup < 2:
        raise SystemExit("at least 7 calls after 2 warm-up calls per form")
    import starky_bn254_amd as S
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("power_time.py needs a GPU")
    rng = random.Random(args.seed)

    def elems(count, coeffs):
        return np.array([[w for _ in range(coeffs) for w in S.api._int_limbs(rng.randrange(S.BN_P), 8)] for _ in range(count)], dtype=np.uint32)

    trace_cases, prove_cases = {}, {}
    for cls, num_io, bits, coeffs in TABLES:
        stark = getattr(S, cls)(num_io)
        exp = S.BN_X if cls == "Fq12ExpU64Stark" else rng.randrange(1 << 255, 1 << 256)
        prover = S.Prover(stark, stark.config(), bits)
        d = prover.describe()
        dev = lambda: prover.stage_times()["device_tracegen_ms"]   # noqa: E731
        for depth in (1, 3):
            bases = elems(num_io // depth, coeffs)
            ios, powers = S.power_instances(stark, bases, exp, depth)
            pi = prover.generate_trace(ios[0])
            pi_p, powers_p, ios_p = prover.generate_trace_powers(bases, exp, depth)
            assert np.array_equal(pi, pi_p) and np.array_equal(ios[0], ios_p) and np.array_equal(powers, powers_p)
            pw = timed(args.calls, args.warmup, lambda: prover.generate_trace_powers(bases, exp, depth), dev)
            hf = timed(args.calls, args.warmup, lambda: prover.generate_trace(S.power_instances(stark, bases, exp, depth)[0][0]), dev)
            name = f"{cls}({num_io}) depth {depth}: {len(bases)} towers"
            h = hf["host_clock_ms"]
            trace_cases[name] = {"fq12_host_chain": d.get("fq12_host_chain"), "powers": pw, "host_form": hf,
                                 "powers_minus_host_form_median_ms": pw["host_clock_ms"]["median"] - h["median"],
                                 "host_form_spread_ms": h["max"] - h["min"]}
            print(f"| {name} | {pw['host_clock_ms']['median']:.2f} | {h['median']:.2f} ({h['min']:.2f}-{h['max']:.2f}) | "
                  f"{pw['device_tracegen_ms']['median']:.2f} | {hf['device_tracegen_ms']['median']:.2f} |", flush=True)
        prover.close()
    # f^x, f^(x^2), f^(x^3) of --inputs elements: towers of depth 3 across the units of Fq12ExpU64Stark(16)
    stark = S.Fq12ExpU64Stark(16)
    fs = elems(args.inputs, 12)
    units, powers = S.power_instances(stark, fs, S.BN_X, 3)
    bp = S.BatchProver(stark, stark.config(), 11, inflight=args.inflight)
    proofs, got, _ = bp.prove_bn_x_powers(fs)
    want = bp.prove_ios(units)
    assert np.array_equal(got, powers) and all(np.array_equal(a.words, b.words) for a, b in zip(proofs, want))
    del proofs, want
    bx = timed(args.calls, args.warmup, lambda: bp.prove_bn_x_powers(fs))
    pi = timed(args.calls, args.warmup, lambda: bp.prove_ios(units))
    bp.close()
    name = f"Fq12ExpU64Stark(16) x {len(units)} units, {args.inputs} inputs, inflight {args.inflight}"
    prove_cases[name] = {"prove_bn_x_powers": bx, "prove_ios": pi}
    print(f"| {name} | {bx['host_clock_ms']['median']:.1f} | {pi['host_clock_ms']['median']:.1f} |", flush=True)
    out = {"workload": f"seeded field elements (seed {args.seed}); exponent BN_X on Fq12ExpU64Stark, a seeded 256-bit one elsewhere; {args.calls} calls "
                       f"per form after {args.warmup} warm-up calls; BN-parameter powers: {args.inputs} seeded Fq12 elements, depth 3",
           "clock": "host_clock_ms: perf_counter around the whole call; device_tracegen_ms: HIP events on the prover's stream (stage_times), "
                    "the device span of the generate_trace inside the call only",
           "columns": "| case | powers host clock | host_form host clock (min-max) | powers device | host_form device |",
           "trace_cases": trace_cases, "prove_cases": prove_cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
