#!/usr/bin/env python3
"""Times Prover.explain_trace and Prover.explain_rows (16 rows) beside Prover.check_trace on G1ExpStark(128) (2^16 rows) and
Fq12ExpStark(16) (2^13 rows), device and host forms, in one process on the GPU box.  The witness is generated on the device
from seeded instances and read back for the host forms; after a warm-up the three device calls alternate for --calls calls,
each timed on the host clock around the whole call, the host forms for --host-calls calls.  Reported per table: median
(min-max) of each, and the stage split of the median explain_trace by HIP events (permutation Z, explain kernels, download).
Every result must be clean.  --prove-ab LIB[,LIB..] adds a prove-time A/B of G1ExpStark(128): tools/ab_lib_prove_time.py is run
three times per library (SBN_LIB), each in a fresh process, and both sets of runs go into the file.

    python tools/explain_time.py [--out profiles/explain_time.json] [--calls 20] [--host-calls 3] [--tables g1,fq12]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES = {"g1": ("G1ExpStark", 128, 16), "fq12": ("Fq12ExpStark", 16, 13)}


def timed(f, *a, **k):
    t0 = time.perf_counter()
    r = f(*a, **k)
    return (time.perf_counter() - t0) * 1e3, r


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls_ms": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--tables", default="g1,fq12")
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--prove-ab", default="", help="name=path of libraries for the prove-time A/B, comma separated")
    args = ap.parse_args()
    import numpy as np
    import starky_bn254_amd as S
    from bench import synthetic_ios, synthetic_ios_fq12
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("explain_time.py needs a GPU")
    results = {}
    for key in args.tables.split(","):
        cls, num_io, bits = TABLES[key]
        stark = getattr(S, cls)(num_io)
        n = 1 << bits
        rows = np.arange(16, dtype=np.uint64) * (n // 16) + 5
        prover = S.Prover(stark, stark.config(), bits)
        pi = prover.generate_trace(synthetic_ios_fq12(num_io, args.seed) if key == "fq12" else synthetic_ios(num_io, args.seed, key))
        assert prover.check_trace().ok and prover.explain_trace().ok and all(r.ok for r in prover.explain_rows(rows))   # warm-up
        t = {"check_trace": [], "explain_trace": [], "explain_rows_16": [], "check_trace_host": [], "explain_trace_host": [], "explain_rows_16_host": []}
        stages = []
        for _ in range(args.calls):
            ms, rep = timed(prover.check_trace, seed=args.seed)
            t["check_trace"].append(ms)
            assert rep.ok
            ms, e = timed(prover.explain_trace, seed=args.seed)
            t["explain_trace"].append(ms)
            stages.append(prover.explain_times())
            assert e.ok
            ms, r = timed(prover.explain_rows, rows, seed=args.seed)
            t["explain_rows_16"].append(ms)
            assert all(x.ok for x in r)
        trace = prover.read_trace()
        prover.close()
        for _ in range(args.host_calls):
            ms, rep = timed(S.check_trace_host, stark, trace, pi, seed=args.seed)
            t["check_trace_host"].append(ms)
            ms, e = timed(S.explain_trace_host, stark, trace, pi, seed=args.seed)
            t["explain_trace_host"].append(ms)
            ms, r = timed(S.explain_rows_host, stark, trace, pi, rows, seed=args.seed)
            t["explain_rows_16_host"].append(ms)
            assert rep.ok and e.ok and all(x.ok for x in r)
        del trace
        entry = {k: summary(v) for k, v in t.items()}
        mid = sorted(range(args.calls), key=lambda i: t["explain_trace"][i])[args.calls // 2]
        entry["explain_trace"]["stage_ms_of_median_call"] = stages[mid]
        results[f"{cls}({num_io})"] = dict(entry, rows=n, columns=stark.num_columns, blocks=len(stark.constraint_blocks()), num_zs=stark.num_permutation_zs())
        print(f"{cls}({num_io})", {k: round(v["median_ms"], 3) for k, v in entry.items()}, stages[mid], flush=True)
    out = {"workload": f"device witness of seed {args.seed}; check_trace(), explain_trace() and explain_rows(16 rows) alternate, {args.calls} calls each "
                       f"after a warm-up; the host forms on the trace read back, {args.host_calls} calls each",
           "clock": "host perf_counter around the whole call; stage_ms: HIP events on the prover's stream",
           "tables": results}
    if args.prove_ab:
        libs = [item.split("=", 1) for item in args.prove_ab.split(",")]
        ab = {name: [] for name, _ in libs}
        for _ in range(3):   # the libraries alternate; a fresh process per run: SBN_LIB is read when the package loads the library
            for name, path in libs:
                p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_lib_prove_time.py"), "20"], env=dict(os.environ, SBN_LIB=path),
                                   capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    raise SystemExit(f"ab_lib_prove_time.py failed for {name}: {p.stderr[-2000:]}")
                line = p.stdout.strip().splitlines()[-1]
                ab[name].append({"ms_per_proof": float(line.split("ms_per_proof ")[1].split()[0]), "line": line})
                print(name, ab[name][-1]["ms_per_proof"], flush=True)
        out["prove_time_ab_G1ExpStark(128)"] = ab
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")

    def cell(e):
        return f"{e['median_ms']:.2f} ({e['min_ms']:.2f}-{e['max_ms']:.2f})"
    for name, e in results.items():
        st = e["explain_trace"]["stage_ms_of_median_call"]
        print(f"| {name} | {cell(e['check_trace'])} | {cell(e['explain_trace'])} | {cell(e['explain_rows_16'])} | "
              f"{st['perm_z']:.2f} / {st['explain']:.2f} / {st['download']:.3f} | {cell(e['check_trace_host'])} | {cell(e['explain_trace_host'])} | {cell(e['explain_rows_16_host'])} |")


if __name__ == "__main__":
    main()
