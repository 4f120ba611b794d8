#!/usr/bin/env python3
"""What verified proving costs (include/sbn.h sbn_prover_set_guard) on G1ExpStark(128), 2^16 rows, in one process on the GPU box.
Two workloads, three arms each -- no guard, the device guard, the host guard -- on ONE context (one batch prover) whose mode is
switched between calls, so the arms alternate call by call and share every buffer:

    single   Prover.prove() on a resident trace (witness generated on the device once)
    batch    BatchProver.prove_ios of 24 units at inflight 2

Each call is timed on the host clock around the whole call (a proof comes back assembled on the host, so the call ends behind its
last device wait).  Per arm: 3 warm-up calls, then 20 timed calls; reported: median (min-max) ms per call, the arm's median minus
the unguarded median, the guard's own account of itself (sbn_prover_guard_stats: proofs checked and rejected, mean ms per check,
device bytes) and, for the batch, proofs per second.  A guarded call that fails (a unit its verifier rejects) is counted under
failed_calls and its message kept; it is not retried and its time is not used.

    python tools/guarded_prove_time.py [--out profiles/guarded_prove_time.json] [--calls 20] [--warmup 3] [--units 24] [--inflight 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NUM_IO, DEGREE_BITS = 128, 16
ARMS = [("unguarded", None), ("device", "device"), ("host", "host")]


def run_arms(obj, call, calls, warmup, S):
    """Alternates the arms on `obj` (set_guard, then `call`); -> per arm: times of the timed calls (ms), failures, stats delta."""
    times = {a: [] for a, _ in ARMS}
    failed = {a: [] for a, _ in ARMS}
    checked = {a: [0, 0, 0] for a, _ in ARMS}
    for k in range(warmup + calls):
        for arm, mode in ARMS:
            obj.set_guard(mode)
            before = obj.guard_stats()
            t0 = time.perf_counter()
            try:
                call()
                ms = (time.perf_counter() - t0) * 1e3
                if k >= warmup:
                    times[arm].append(ms)
            except S.SbnError as e:
                if e.code != -6:
                    raise
                failed[arm].append(e.reason)
            after = obj.guard_stats()
            if k >= warmup:
                for i, f in enumerate(("checked", "rejected", "ns")):
                    checked[arm][i] += getattr(after, f) - getattr(before, f)
    return times, failed, checked, obj.guard_stats().device_bytes


def summarize(times, failed, checked, device_bytes, proofs_per_call):
    out = {}
    base = statistics.median(times["unguarded"])
    for arm, _ in ARMS:
        t = times[arm]
        med = statistics.median(t)
        n_checked, n_rejected, ns = checked[arm]
        out[arm] = {
            "calls": len(t), "median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
            "minus_unguarded_ms": round(med - base, 3),
            "proofs_per_s": round(proofs_per_call / med * 1e3, 2),
            "guard_checked": n_checked, "guard_rejected": n_rejected,
            "guard_ms_per_check": round(ns / n_checked / 1e6, 3) if n_checked else None,
            "failed_calls": len(failed[arm]), "failures": failed[arm][:4],
        }
    out["guard_device_bytes"] = device_bytes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guarded_prove_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--units", type=int, default=24)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    from starky_bn254_amd import sharding
    os.environ.setdefault("SBN_HOST_THREADS", str(max(1, min(64, sharding.effective_cpus()))))
    import numpy as np
    import starky_bn254_amd as S
    from bench import synthetic_ios
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("guarded_prove_time.py needs a GPU")
    stark = S.G1ExpStark(NUM_IO)
    cfg = stark.config()
    result = {"table": f"G1ExpStark({NUM_IO})", "degree_bits": DEGREE_BITS, "calls": args.calls, "warmup": args.warmup,
              "arms_alternate": "call by call on one context", "clock": "host clock around the whole call"}

    p = S.Prover(stark, cfg, DEGREE_BITS)
    p.generate_trace(synthetic_ios(NUM_IO, args.seed, "g1"))
    want = p.prove().words
    single = run_arms(p, p.prove, args.calls, args.warmup, S)
    assert np.array_equal(p.prove().words, want)          # the words did not move under any arm
    result["single"] = summarize(*single, proofs_per_call=1)
    result["single"]["describe"] = {k: v for k, v in p.describe().items() if k.startswith("guard") or k == "dev_bytes"}
    p.close()
    print("single", json.dumps(result["single"]), flush=True)

    ios = np.stack([synthetic_ios(NUM_IO, args.seed + u, "g1") for u in range(args.units)])
    bp = S.BatchProver(stark, cfg, DEGREE_BITS, inflight=args.inflight)
    batch = run_arms(bp, lambda: bp.prove_ios(ios), args.calls, args.warmup, S)
    result["batch"] = summarize(*batch, proofs_per_call=args.units)
    result["batch"].update({"units": args.units, "inflight": args.inflight})
    bp.close()
    print("batch", json.dumps(result["batch"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
