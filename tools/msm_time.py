#!/usr/bin/env python3
"""Times a long chained list (count = 16 num_io: sixteen units) proved as units of one table, in one process on one GPU with
BatchProver(inflight=3): G1ExpStark(128) and Fq12ExpStark(16).  The terms are the seeded instances of bench.py without their
offsets, start is the offset of instance 0.  Per table two batch provers, one per placement of the table's chains
  host    the chains on the host (G1: SBN_TRACEGEN_DEVICE_CHAIN=0; Fq12: SBN_FQ12_HOST_CHAIN=1),
  device  the chains on the device (G1: SBN_TRACEGEN_DEVICE_CHAIN=2; Fq12: the default),
and per placement three forms, host clock (perf_counter) around calls that return with every proof on the host:
  a_user   what a caller could do before prove_msm existed: chain_instances() over the whole list on the host pool (the count is a
           multiple of num_io, so there is nothing to pad), then BatchProver.prove_ios on the units;
  msm      BatchProver.prove_msm: the list derived on the host pool inside the call, then the same units;
  ceiling  BatchProver.prove_ios on the explicit units already at hand: no derivation at all.
a_list is the chain_instances() share of a_user alone: the most any form that derives the offsets elsewhere could save.  The
repetitions alternate over every form of both placements after a warm-up of each; every form must return the same proof words.  For
each the JSON holds the repetitions, their median and their spread (max - min).

    python tools/msm_time.py [--out profiles/msm_time.json] [--reps 7]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# class, instances, degree bits, {placement: switches}
TABLES = {"g1": ("G1ExpStark", 128, 16, {"host": {"SBN_TRACEGEN_DEVICE_CHAIN": "0"}, "device": {"SBN_TRACEGEN_DEVICE_CHAIN": "2"}}),
          "fq12": ("Fq12ExpStark", 16, 13, {"host": {"SBN_EXPERIMENTAL": "1", "SBN_FQ12_HOST_CHAIN": "1"}, "device": {}})}
UNITS = 16


def summary(ms):
    return {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "reps_ms": ms}


def create(S, stark, bits, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return S.BatchProver(stark, stark.config(), bits, inflight=3)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_time.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tables", default="g1,fq12")
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    import starky_bn254_amd as S
    from chained_trace_time import seeded_terms
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("msm_time.py needs a GPU")
    results = {}
    for key in args.tables.split(","):
        cls, num_io, bits, placements = TABLES[key]
        stark = getattr(S, cls)(num_io)
        count = UNITS * num_io
        terms, start = seeded_terms(key, count, args.seed)
        units, _ = S.msm_instances(stark, terms, start)
        forms, provers, want = {"a_list": lambda: S.chain_instances(stark, terms, start)}, [], None
        for pl, env in placements.items():
            bp = create(S, stark, bits, env)
            provers.append(bp)
            forms[pl + ".a_user"] = lambda bp=bp: bp.prove_ios(S.chain_instances(stark, terms, start)[0].reshape(UNITS, num_io, -1))
            forms[pl + ".msm"] = lambda bp=bp: bp.prove_msm(terms, start)[0]
            forms[pl + ".ceiling"] = lambda bp=bp: bp.prove_ios(units)
        for k, f in forms.items():                               # warm-up of every form; all must give the same words
            got = f()
            if k == "a_list":
                continue
            want = want or [p.words for p in got]
            assert len(got) == UNITS and all(np.array_equal(p.words, w) for p, w in zip(got, want)), k
        ms = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, f in forms.items():
                t0 = time.perf_counter()
                f()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for bp in provers:
            bp.close()
        name = f"{cls}({num_io}) count={count}"
        r = {k: summary(v) for k, v in ms.items()}
        results[name] = r
        print(f"| {name} | " + " | ".join(f"{k} {v['median_ms']:.1f} (spread {v['spread_ms']:.1f})" for k, v in r.items()) + " |", flush=True)
    out = {"workload": f"seeded instances of bench.py (seed {args.seed}) without their offsets, start = the offset of instance 0; "
                       f"{UNITS} units per list, BatchProver(inflight=3) per placement, {args.reps} alternating repetitions after a warm-up of every form",
           "clock": "perf_counter around the whole call (every proof is on the host when it returns); spread = max - min of the repetitions",
           "cases": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
