#!/usr/bin/env python3
"""Times Prover.generate_trace on an explicit instance list against Prover.generate_trace_chained on its terms (the reference's
*_msm call shape: offset[0] = start, offset[k+1] = output[k]), in one process on the GPU box: G1ExpStark(128), G2ExpStark(128),
Fq12ExpStark(16) and Fq12ExpU64Stark(16).  The terms are the seeded instances of bench.py without their offsets, start is the
offset of instance 0; the explicit list is what chain_instances() derives from them on the host pool.  Per table and placement of
the chains (G1 / G2: SBN_TRACEGEN_DEVICE_CHAIN 0, 1, 2; Fq12: the default, chains on the device), medians over --calls calls of
  explicit  the device_tracegen_ms entry of stage_times() after generate_trace(ios), and the host clock around the call;
  chained   the same after generate_trace_chained(terms, start);
  host_list the host clock around chain_instances(), what a caller of the explicit form pays first.
The entry covers the device span of a call only (upload to drained stream); where the list is derived on the host pool inside the
chained call (placement 0) that part shows in the host clock alone.  Both forms must return the same public inputs.  Writes
the JSON file and prints one row per case.

    python tools/chained_trace_time.py [--out profiles/chained_trace_time.json] [--calls 20]
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

# table -> (class, instances, degree bits, u32 words of x, placements)
CURVE_ENVS = [{"SBN_TRACEGEN_DEVICE_CHAIN": c} for c in "012"]
TABLES = {"g1": ("G1ExpStark", 128, 16, 16, CURVE_ENVS), "g2": ("G2ExpStark", 128, 16, 32, CURVE_ENVS),
          "fq12": ("Fq12ExpStark", 16, 13, 96, [{}]), "fq12u64": ("Fq12ExpU64Stark", 16, 11, 96, [{}])}


def seeded_terms(key, num_io, seed):
    from bench import synthetic_ios, synthetic_ios_fq12
    if key in ("g1", "g2"):
        ios = synthetic_ios(num_io, seed, key)
    else:
        ios = synthetic_ios_fq12(num_io, seed)
        if key == "fq12u64":
            ios = np.ascontiguousarray(ios[:, :194])
            ios[:, 193] &= 0x7FFFFFFF              # a canonical field element
    xw = TABLES[key][3]
    return np.ascontiguousarray(np.concatenate([ios[:, :xw], ios[:, 2 * xw:]], axis=1)), np.ascontiguousarray(ios[0, xw:2 * xw])


def median_ms(calls, f):
    wall, dev = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        d = f()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(d)
    return {"device_tracegen_ms": statistics.median(dev), "host_clock_ms": statistics.median(wall), "device_calls_ms": dev}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chained_trace_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--tables", default="g1,g2,fq12,fq12u64")
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    import starky_bn254_amd as S
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("chained_trace_time.py needs a GPU")
    results = {}
    for key in args.tables.split(","):
        cls, num_io, bits, _, envs = TABLES[key]
        stark = getattr(S, cls)(num_io)
        terms, start = seeded_terms(key, num_io, args.seed)
        ios, _ = S.chain_instances(stark, terms, start)
        t = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            S.chain_instances(stark, terms, start)
            t.append((time.perf_counter() - t0) * 1e3)
        host_list = statistics.median(t)
        for env in envs:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                prover = S.Prover(stark, stark.config(), bits)
            finally:
                for k, v in old.items():
                    os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
            d = prover.describe()
            pi = prover.generate_trace(ios)                      # warm-up of both forms: code objects, pinned staging
            pi_c, ios_c = prover.generate_trace_chained(terms, start)
            assert np.array_equal(pi, pi_c) and np.array_equal(ios, ios_c)

            def explicit():
                prover.generate_trace(ios)
                return prover.stage_times()["device_tracegen_ms"]

            def chained():
                prover.generate_trace_chained(terms, start)
                return prover.stage_times()["device_tracegen_ms"]
            e, c = median_ms(args.calls, explicit), median_ms(args.calls, chained)
            prover.close()
            name = f"{cls}({num_io})" + ("".join(f" {k}={v}" for k, v in env.items()))
            results[name] = {"curve_chains": d.get("curve_chains"), "explicit": e, "chained": c, "host_list_ms": host_list,
                             "chained_over_explicit_device": c["device_tracegen_ms"] / e["device_tracegen_ms"],
                             "chained_over_host_list_plus_explicit_host_clock": c["host_clock_ms"] / (host_list + e["host_clock_ms"])}
            print(f"| {name} | {e['device_tracegen_ms']:.2f} | {c['device_tracegen_ms']:.2f} | {e['host_clock_ms']:.2f} | {c['host_clock_ms']:.2f} | "
                  f"{host_list:.2f} | {results[name]['chained_over_host_list_plus_explicit_host_clock']:.2f} |", flush=True)
    out = {"workload": f"seeded instances of bench.py (seed {args.seed}) without their offsets, start = the offset of instance 0; "
                       f"medians of {args.calls} calls after a warm-up of both forms",
           "clock": "device_tracegen_ms: HIP events on the prover's stream (stage_times); host_clock_ms: perf_counter around the whole call",
           "columns": "| case | explicit device | chained device | explicit host clock | chained host clock | chain_instances host clock | chained / (chain_instances + explicit) |",
           "cases": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
