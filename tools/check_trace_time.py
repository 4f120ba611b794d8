#!/usr/bin/env python3
"""Times Prover.check_trace beside Prover.prove on G1ExpStark(128) (2^16 rows) and Fq12ExpStark(512) (2^18 rows), in one process
on the GPU box.  The witness is generated on the device from seeded instances; after a warm-up of each, check_trace() and
prove() alternate for --calls calls, each timed on the host clock around the whole call.  Reported per table: median (min-max)
of both, the stage split of the median check by HIP events (permutation Z, constraint kernels, reduction, download), and
check_trace(flags=True), which also downloads the N flag bytes.  Every report must be clean.  Writes the JSON file and prints
one row per table for DESIGN.md section 7.

    python tools/check_trace_time.py [--out profiles/check_trace_time.json] [--calls 20] [--tables g1,fq12]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES = {"g1": ("G1ExpStark", 128, 16), "fq12": ("Fq12ExpStark", 512, 18)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_trace_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--tables", default="g1,fq12")
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    import starky_bn254_amd as S
    from bench import synthetic_ios, synthetic_ios_fq12
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("check_trace_time.py needs a GPU")
    results = {}
    for key in args.tables.split(","):
        cls, num_io, bits = TABLES[key]
        stark = getattr(S, cls)(num_io)
        prover = S.Prover(stark, stark.config(), bits)
        prover.generate_trace(synthetic_ios_fq12(num_io, args.seed) if key == "fq12" else synthetic_ios(num_io, args.seed, key))
        assert prover.check_trace().ok and prover.check_trace(flags=True).ok   # warm-up: code objects, first touch
        prover.prove()
        t = {"check": [], "check_flags": [], "prove": []}
        stages = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            rep = prover.check_trace(seed=args.seed)
            t["check"].append((time.perf_counter() - t0) * 1e3)
            stages.append(prover.check_times())
            assert rep.ok, str(rep)
            t0 = time.perf_counter()
            rep = prover.check_trace(seed=args.seed, flags=True)
            t["check_flags"].append((time.perf_counter() - t0) * 1e3)
            assert rep.ok and not rep.row_flags.any()
            t0 = time.perf_counter()
            prover.prove()
            t["prove"].append((time.perf_counter() - t0) * 1e3)
        prover.close()
        entry = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls_ms": v} for k, v in t.items()}
        mid = sorted(range(args.calls), key=lambda i: t["check"][i])[args.calls // 2]
        entry["check"]["stage_ms_of_median_call"] = stages[mid]
        entry["check_over_prove"] = entry["check"]["median_ms"] / entry["prove"]["median_ms"]
        results[f"{cls}({num_io})"] = dict(entry, rows=1 << bits, columns=stark.num_columns, num_zs=stark.num_permutation_zs())
        print(f"{cls}({num_io})", {k: round(v["median_ms"], 3) for k, v in entry.items() if isinstance(v, dict)}, stages[mid], flush=True)
    out = {"workload": f"device witness of seed {args.seed}; check_trace() and prove() alternate, {args.calls} calls each after a warm-up",
           "clock": "host perf_counter around the whole call; stage_ms: HIP events on the prover's stream",
           "forms": {"check": "Prover.check_trace(): report only", "check_flags": "Prover.check_trace(flags=True): report and N flag bytes",
                     "prove": "Prover.prove()"},
           "tables": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")

    def cell(e):
        return f"{e['median_ms']:.2f} ({e['min_ms']:.2f}-{e['max_ms']:.2f})"
    for name, e in results.items():
        st = e["check"]["stage_ms_of_median_call"]
        print(f"| {name} | {cell(e['prove'])} | {cell(e['check'])} | {cell(e['check_flags'])} | "
              f"{st['perm_z']:.2f} / {st['constraints']:.2f} / {st['reduction']:.3f} / {st['download']:.3f} |")


if __name__ == "__main__":
    main()
