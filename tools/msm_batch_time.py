#!/usr/bin/env python3
"""Times a batch of short MSMs in one process on the GPU box.  On G1ExpStark(128), --segments sums of --terms terms each (the
seeded points and exponents of bench.py, the generator as the start of every segment), the host clock around
  prove_msms   BatchProver.prove_msms(terms, lengths): the segmented list is derived once on the host pool, the segments share
               units (1,000 sums of 10 terms: 79 units);
  prove_ios    BatchProver.prove_ios on the same units already at hand (no derivation): the yardstick;
  prove_msm    --single of the same segments through one BatchProver.prove_msm call each: every call pads its sum to a whole unit
               (what the segmented call replaces; 1,000 such calls would be 1,000 unit proofs).
Medians and min-max of --calls calls each, after a warm-up of every form.  Writes the JSON file and prints one row per form.

    python tools/msm_batch_time.py [--out profiles/msm_batch_time.json] [--calls 20] [--segments 1000] [--terms 10] [--single 16]
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


def timed(calls, f):
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        wall.append((time.perf_counter() - t0) * 1e3)
    return {"host_clock_ms": {"median": statistics.median(wall), "min": min(wall), "max": max(wall)}, "calls": len(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_batch_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--segments", type=int, default=1000)
    ap.add_argument("--terms", type=int, default=10)
    ap.add_argument("--single", type=int, default=16)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    if args.calls < 20:
        raise SystemExit("at least 20 calls per form")
    import starky_bn254_amd as S
    from bench import synthetic_ios
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("msm_batch_time.py needs a GPU")
    num_io = 128
    stark = S.G1ExpStark(num_io)
    M = args.segments * args.terms
    seeded = synthetic_ios(M, args.seed, "g1")
    terms = np.ascontiguousarray(np.concatenate([seeded[:, :16], seeded[:, 32:]], axis=1))
    lengths = [args.terms] * args.segments
    start = S.generator(stark)
    units, finals, sums, infinity = S.msm_batch_instances(stark, terms, lengths)
    bp = S.BatchProver(stark, stark.config(), 16, inflight=args.inflight)
    proofs, fin, sm, inf, ios = bp.prove_msms(terms, lengths)              # warm-up of every form
    want = bp.prove_ios(units)
    assert np.array_equal(ios, units) and np.array_equal(fin, finals) and np.array_equal(sm, sums) and np.array_equal(inf, infinity)
    assert all(np.array_equal(a.words, b.words) for a, b in zip(proofs, want))
    S.verify_msms(stark, stark.config(), proofs, lengths, terms=terms)
    single = min(args.single, args.segments)

    def one_call_per_sum():
        for s in range(single):
            bp.prove_msm(terms[s * args.terms:(s + 1) * args.terms], start)
    one_call_per_sum()
    rows = {"prove_msms": timed(args.calls, lambda: bp.prove_msms(terms, lengths)), "prove_ios": timed(args.calls, lambda: bp.prove_ios(units)),
            "prove_msm": timed(args.calls, one_call_per_sum)}
    bp.close()
    rows["prove_msms"]["unit_proofs"] = rows["prove_ios"]["unit_proofs"] = len(units)
    rows["prove_msm"]["unit_proofs"] = rows["prove_msm"]["segments"] = single
    for name, r in rows.items():
        h = r["host_clock_ms"]
        print(f"| {name} | {r['unit_proofs']} unit proofs | {h['median']:.1f} ({h['min']:.1f}-{h['max']:.1f}) ms |", flush=True)
    out = {"workload": f"G1ExpStark({num_io}), {args.segments} segments of {args.terms} terms: seeded points and exponents of bench.py (seed {args.seed}), "
                       f"start = the generator; {len(units)} units beside {args.segments} for one prove_msm call per segment; inflight {args.inflight}; "
                       f"{args.calls} calls per form after a warm-up of every form; prove_msm: {single} of the segments, one call each",
           "clock": "host_clock_ms: perf_counter around the whole call (prove_msm: around the loop of calls)",
           "columns": "| form | unit proofs | host clock median (min-max) |", "forms": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
