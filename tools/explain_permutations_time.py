#!/usr/bin/env python3
"""Times Prover.explain_permutations on G1ExpStark(128) (2^16 rows, 762 pairs) beside Prover.check_trace and
Prover.explain_trace, in one process on the GPU box: the device form on the clean device witness and on a copy in which EVERY
pair fails (one cell of each rhs column changed to another value of its range), and the host form (explain_permutations_host,
SBN_HOST_THREADS=16 unless set) on both.  After a warm-up the device calls alternate for --calls calls, each timed on the host
clock around the whole call; the split of the median call is the library's own (two kernels by HIP events, download + host
merge by the host clock).  Device and host results must be equal, and clean / failing as built.

    python tools/explain_permutations_time.py [--out profiles/explain_permutations_time.json] [--calls 20] [--host-calls 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SBN_HOST_THREADS", "16")


def timed(f, *a, **k):
    t0 = time.perf_counter()
    r = f(*a, **k)
    return (time.perf_counter() - t0) * 1e3, r


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls_ms": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_permutations_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    import numpy as np
    import starky_bn254_amd as S
    from bench import synthetic_ios
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("explain_permutations_time.py needs a GPU")
    num_io, bits = 128, 16
    stark = S.G1ExpStark(num_io)
    n, Z = 1 << bits, stark.num_permutation_zs()
    prover = S.Prover(stark, stark.config(), bits)
    pi = prover.generate_trace(synthetic_ios(num_io, args.seed, "g1"))
    clean = prover.read_trace()
    failing = clean.copy()
    for k, col in enumerate(sorted({stark.permutation_pair(z)[1] for z in range(Z)})):
        row = (37 * k) % n
        failing[col, row] = int(failing[col, row]) - 1 if failing[col, row] else 1
    results = {}
    for name, trace in (("clean", clean), ("every_pair_fails", failing)):
        prover.load_trace(trace, pi)
        t = {"explain_permutations": [], "check_trace": [], "explain_trace": [], "explain_permutations_host": []}
        dev = prover.explain_permutations()                          # warm-up
        prover.check_trace(seed=args.seed), prover.explain_trace(seed=args.seed)
        assert dev.ok == (name == "clean") and len(dev.pairs) == (0 if name == "clean" else Z)
        split = []
        for _ in range(args.calls):
            ms, e = timed(prover.explain_permutations)
            t["explain_permutations"].append(ms)
            split.append(prover.explain_permutation_times())
            assert e == dev
            ms, _ = timed(prover.check_trace, seed=args.seed)
            t["check_trace"].append(ms)
            ms, _ = timed(prover.explain_trace, seed=args.seed)
            t["explain_trace"].append(ms)
        routes = prover.describe()["perm_diff_routes"]
        for _ in range(args.host_calls):
            ms, h = timed(S.explain_permutations_host, stark, trace)
            t["explain_permutations_host"].append(ms)
            assert h == dev
        entry = {k: summary(v) for k, v in t.items()}
        mid = sorted(range(args.calls), key=lambda i: t["explain_permutations"][i])[args.calls // 2]
        entry["explain_permutations"]["split_ms_of_median_call"] = split[mid]
        entry["explain_permutations"]["routes_bins_list_download"] = routes
        results[name] = entry
        print(name, {k: round(v["median_ms"], 3) for k, v in entry.items()}, split[mid], routes, flush=True)
    prover.close()
    out = {"workload": f"G1ExpStark({num_io}), {n} rows, {Z} pairs, per_pair = 8; device witness of seed {args.seed}; 'every_pair_fails' = one cell of every "
                       f"rhs column changed to a neighbouring value; explain_permutations(), check_trace() and explain_trace() alternate, {args.calls} calls "
                       f"each after a warm-up; the host form {args.host_calls} calls on {os.environ['SBN_HOST_THREADS']} threads",
           "clock": "host perf_counter around the whole call; split_ms: the two kernels by HIP events on the prover's stream, download + host merge by the host clock",
           "traces": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
