#!/usr/bin/env python3
"""Times the device witness of the u16-range-check tables above 2^18 rows beside the host path it replaces, on the GPU box:
G1ExpStark(1024), G2ExpStark(1024), FqExpStark(1024) (2^19 rows) and FqExpStark(2048) (2^20 rows), seeded instances of bench.py.
Per table
  device     Prover.generate_trace(ios): median of --calls calls of the device_tracegen_ms entry of stage_times() (HIP events) and
             of the host clock around the call, and the SBN_TRACE_TIMING spans of one more call (the library prints them to stderr);
  host       the host clock around stark.generate_trace_and_public_inputs(ios) and around Prover.load_trace(trace, pi), once each:
             what a caller paid for the same resident trace before (7 .. 28 GB over PCIe).
--ab PARENT_LIB adds the A/B of the heights the older forms serve: generate_trace() on G1ExpStark(128) and G1ExpStark(512), this
build against the library PARENT_LIB (a build of the parent commit, through SBN_LIB), --runs fresh processes each, alternating;
every run is the median device_tracegen_ms of --calls calls.  Recorded: the runs, both medians over the runs, and the parent's own
run-to-run spread (largest minus smallest of its runs); "within_parent_spread" says whether this build's median exceeds the
parent's by no more than that spread.  Writes the JSON file and prints one row per case.

    python tools/tall_witness_time.py [--out profiles/tall_witness_time.json] [--calls 5] [--ab PARENT_LIB --runs 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TALL = [("g1", "G1ExpStark", 1024), ("g2", "G2ExpStark", 1024), ("fq", "FqExpStark", 1024), ("fq", "FqExpStark", 2048)]
AB = [("g1", "G1ExpStark", 128), ("g1", "G1ExpStark", 512)]


def seeded_ios(key, num_io, seed):
    from bench import synthetic_ios
    if key in ("g1", "g2"):
        return synthetic_ios(num_io, seed, key)
    rng = np.random.default_rng(seed)                     # FqExpStark: x, offset below p (top limb < 2^28), a 256-bit exponent
    ios = rng.integers(0, 1 << 32, size=(num_io, 24), dtype=np.uint64).astype(np.uint32)
    ios[:, 7] &= 0x0FFFFFFF
    ios[:, 15] &= 0x0FFFFFFF
    return ios


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


def device_calls(prover, ios, calls):
    wall, dev = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        prover.generate_trace(ios)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(prover.stage_times()["device_tracegen_ms"])
    return {"device_tracegen_ms": statistics.median(dev), "host_clock_ms": statistics.median(wall), "device_calls_ms": dev}


def tall_row(S, key, cls, num_io, calls, seed):
    stark = getattr(S, cls)(num_io)
    bits = (512 * num_io).bit_length() - 1
    ios = seeded_ios(key, num_io, seed)
    os.environ["SBN_TRACE_TIMING"] = "1"
    try:
        timed = S.Prover(stark, stark.config(), bits)
    finally:
        del os.environ["SBN_TRACE_TIMING"]
    spans = {}
    for line in stderr_of(lambda: timed.generate_trace(ios)).splitlines():
        if line.startswith("[device tracegen]"):
            name, ms = line[len("[device tracegen]"):].rsplit("ms", 1)[0].rsplit(None, 1)
            spans[name.strip()] = float(ms)
    timed.close()
    prover = S.Prover(stark, stark.config(), bits)
    pi = prover.generate_trace(ios)                          # warm-up: code objects, pinned staging
    dev = device_calls(prover, ios, calls)
    t0 = time.perf_counter()
    trace, pi_host = stark.generate_trace_and_public_inputs(ios)
    host_gen = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(pi, pi_host)
    t0 = time.perf_counter()
    prover.load_trace(trace, pi_host)
    load = (time.perf_counter() - t0) * 1e3
    prover.close()
    return {"rows": 1 << bits, "columns": int(stark.num_columns), "trace_bytes": int(trace.nbytes), "device": dev, "device_spans_ms": spans,
            "host_generator_ms": host_gen, "load_trace_ms": load, "host_path_over_device_host_clock": (host_gen + load) / dev["host_clock_ms"]}


def ab_run(key, cls, num_io, calls, seed):
    """One run of the A/B in this process (whose library SBN_LIB chose): prints the median device_tracegen_ms."""
    import starky_bn254_amd as S
    stark = getattr(S, cls)(num_io)
    prover = S.Prover(stark, stark.config(), (512 * num_io).bit_length() - 1)
    ios = seeded_ios(key, num_io, seed)
    prover.generate_trace(ios)
    print(json.dumps(device_calls(prover, ios, calls)["device_tracegen_ms"]))
    prover.close()


def ab_row(key, cls, num_io, calls, seed, runs, parent_lib):
    got = {"this": [], "parent": []}
    for _ in range(runs):
        for side in ("parent", "this"):
            env = dict(os.environ)
            env.pop("SBN_LIB", None)
            if side == "parent":
                env["SBN_LIB"] = os.path.abspath(parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-run", f"{key}:{cls}:{num_io}", "--calls", str(calls), "--seed", str(seed)],
                                 env=env, check=True, capture_output=True, text=True, timeout=300).stdout
            got[side].append(float(out.strip().splitlines()[-1]))
    spread = max(got["parent"]) - min(got["parent"])
    med = {k: statistics.median(v) for k, v in got.items()}
    return {"runs_ms": got, "median_ms": med, "parent_run_to_run_spread_ms": spread, "within_parent_spread": med["this"] <= med["parent"] + spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tall_witness_time.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--tables", default=",".join(f"{c}:{n}" for _, c, n in TALL))
    ap.add_argument("--ab", default=None, help="libsbn254.so of the parent commit")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab-run", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.ab_run:
        key, cls, num_io = args.ab_run.split(":")
        return ab_run(key, cls, int(num_io), args.calls, args.seed)
    import starky_bn254_amd as S
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("tall_witness_time.py needs a GPU")
    out = {"workload": f"seeded instances (seed {args.seed}); device: medians of {args.calls} generate_trace() calls after a warm-up; host generator and load_trace once each",
           "clock": "device_tracegen_ms and the spans: HIP events on the prover's stream; everything else: perf_counter around the call",
           "tall": {}, "ab_generate_trace": {}}
    wanted = args.tables.split(",") if args.tables else []
    for key, cls, num_io in TALL:
        if f"{cls}:{num_io}" not in wanted:
            continue
        r = tall_row(S, key, cls, num_io, args.calls, args.seed)
        out["tall"][f"{cls}({num_io})"] = r
        print(f"| {cls}({num_io}) | {r['device']['device_tracegen_ms']:.1f} | {r['device']['host_clock_ms']:.1f} | {r['host_generator_ms']:.0f} | {r['load_trace_ms']:.0f} | "
              f"{r['host_path_over_device_host_clock']:.1f} |", flush=True)
    if args.ab:
        for key, cls, num_io in AB:
            r = ab_row(key, cls, num_io, max(args.calls, 20), args.seed, args.runs, args.ab)
            out["ab_generate_trace"][f"{cls}({num_io})"] = r
            print(f"| A/B {cls}({num_io}) | this {r['median_ms']['this']:.3f} | parent {r['median_ms']['parent']:.3f} | parent spread {r['parent_run_to_run_spread_ms']:.3f} | "
                  f"{'within' if r['within_parent_spread'] else 'OUTSIDE'} |", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
