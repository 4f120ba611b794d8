#!/usr/bin/env python3
"""Times the independent scalar multiplications (every instance carries the same offset, the caller wants e_k x_k) in one process
on the GPU box.  For G1ExpStark(128) and G2ExpStark(128), per placement of the curve chains (SBN_TRACEGEN_DEVICE_CHAIN 0, 1, 2),
the host clock around
  scalar_muls  Prover.generate_trace_scalar_muls(points, scalars): in placements 1 and 2 the list is expanded on the device and the
               products are computed there; in placement 0 the call derives the list on the host pool itself;
  host_form    scalar_mul_instances(stark, points, scalars) followed by Prover.generate_trace on its list: what the call replaces;
  explicit     Prover.generate_trace alone on the explicit list already at hand (no derivation, no products): the yardstick;
and the device_tracegen_ms entry of stage_times() after each.  Then BatchProver.prove_mul_by_cofactor of --points twist points
beside BatchProver.prove_ios on the same units already at hand.  Medians and min-max of --calls calls each, after a warm-up of
every form.  The points are the seeded points of bench.py, the scalars its exponents (not reduced), the offset the generator.
Writes the JSON file and prints one row per case.

    python tools/scalar_mul_time.py [--out profiles/scalar_mul_time.json] [--calls 20] [--points 1000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CURVE_ENVS = [{"SBN_TRACEGEN_DEVICE_CHAIN": c} for c in "012"]
TABLES = {"g1": ("G1ExpStark", 128, 16, 16), "g2": ("G2ExpStark", 128, 16, 32)}   # class, instances, degree bits, u32 words of x


def under(env, make):
    """make() with the switches `env` set (they are read when a prover is created), restored afterwards."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)


def timed(calls, f, dev=None):
    wall, d = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        wall.append((time.perf_counter() - t0) * 1e3)
        if dev:
            d.append(dev())
    out = {"host_clock_ms": {"median": statistics.median(wall), "min": min(wall), "max": max(wall)}, "calls": len(wall)}
    if d:
        out["device_tracegen_ms"] = {"median": statistics.median(d), "min": min(d), "max": max(d)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar_mul_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    if args.calls < 20:
        raise SystemExit("at least 20 calls per form")
    import starky_bn254_amd as S
    from bench import synthetic_ios
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("scalar_mul_time.py needs a GPU")
    trace_cases, prove_cases = {}, {}
    for key, (cls, num_io, bits, xw) in TABLES.items():
        stark = getattr(S, cls)(num_io)
        seeded = synthetic_ios(num_io, args.seed, key)
        points, scalars = np.ascontiguousarray(seeded[:, :xw]), np.ascontiguousarray(seeded[:, 2 * xw:])
        ios, products, infinity = S.scalar_mul_instances(stark, points, scalars)
        for env in CURVE_ENVS:
            prover = under(env, lambda: S.Prover(stark, stark.config(), bits))
            d = prover.describe()
            dev = lambda: prover.stage_times()["device_tracegen_ms"]   # noqa: E731
            pi = prover.generate_trace(ios[0])                          # warm-up of every form: code objects, pinned staging
            pi_s, prod_s, inf_s, ios_s = prover.generate_trace_scalar_muls(points, scalars)
            assert np.array_equal(pi, pi_s) and np.array_equal(ios[0], ios_s) and np.array_equal(products, prod_s) and np.array_equal(infinity, inf_s)
            sm = timed(args.calls, lambda: prover.generate_trace_scalar_muls(points, scalars), dev)
            hf = timed(args.calls, lambda: prover.generate_trace(S.scalar_mul_instances(stark, points, scalars)[0][0]), dev)
            ex = timed(args.calls, lambda: prover.generate_trace(ios[0]), dev)
            prover.close()
            name = f"{cls}({num_io})" + "".join(f" {k}={v}" for k, v in env.items())
            h = hf["host_clock_ms"]
            trace_cases[name] = {"curve_chains": d.get("curve_chains"), "scalar_muls": sm, "host_form": hf, "explicit": ex,
                                 "scalar_muls_minus_host_form_median_ms": sm["host_clock_ms"]["median"] - h["median"],
                                 "host_form_spread_ms": h["max"] - h["min"]}
            print(f"| {name} | {sm['host_clock_ms']['median']:.2f} | {h['median']:.2f} ({h['min']:.2f}-{h['max']:.2f}) | "
                  f"{ex['host_clock_ms']['median']:.2f} | {sm['device_tracegen_ms']['median']:.2f} | {ex['device_tracegen_ms']['median']:.2f} |", flush=True)
    # cofactor clearing of --points twist points: the rows of bench.py's G2 list hold two random twist points each
    stark = S.G2ExpStark(128)
    seeded = synthetic_ios((args.points + 1) // 2, args.seed + 1, "g2")
    points = np.ascontiguousarray(seeded[:, :64].reshape(-1, 32)[:args.points])
    units, cleared, infinity = S.scalar_mul_instances(stark, points, S.G2_COFACTOR)
    bp = S.BatchProver(stark, stark.config(), 16, inflight=args.inflight)
    proofs, got, inf, _ = bp.prove_mul_by_cofactor(points)              # warm-up of both forms
    want = bp.prove_ios(units)
    assert np.array_equal(got, cleared) and np.array_equal(inf, infinity) and all(np.array_equal(a.words, b.words) for a, b in zip(proofs, want))
    co = timed(args.calls, lambda: bp.prove_mul_by_cofactor(points))
    pi = timed(args.calls, lambda: bp.prove_ios(units))
    bp.close()
    name = f"G2ExpStark(128) x {len(units)} units, {args.points} points, inflight {args.inflight}"
    prove_cases[name] = {"prove_mul_by_cofactor": co, "prove_ios": pi}
    print(f"| {name} | {co['host_clock_ms']['median']:.1f} | {pi['host_clock_ms']['median']:.1f} |", flush=True)
    out = {"workload": f"seeded points and exponents of bench.py (seed {args.seed}), offset = the generator; {args.calls} calls per form after a "
                       f"warm-up of every form; cofactor clearing: {args.points} seeded twist points (seed {args.seed + 1})",
           "clock": "host_clock_ms: perf_counter around the whole call; device_tracegen_ms: HIP events on the prover's stream (stage_times), "
                    "the device span of the generate_trace inside the call only",
           "columns": "| case | scalar_muls host clock | host_form host clock (min-max) | explicit host clock | scalar_muls device | explicit device |",
           "trace_cases": trace_cases, "prove_cases": prove_cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
