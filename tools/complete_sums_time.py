#!/usr/bin/env python3
"""Times the complete sums (include/sbn.h, "Complete sums") in one process on the GPU box.  On G1ExpStark(128) and
G2ExpStark(128), per placement of the curve chains (SBN_TRACEGEN_DEVICE_CHAIN 0, 1, 2, set before the prover is created), one
unit of 12 segments of 10 seeded terms (bench.py's points and exponents), the host clock around
  explicit        Prover.generate_trace_msms on the list with explicit starts (candidate 0 for every segment): the yardstick;
  complete        Prover.generate_trace_msms_complete on the same terms: every choice is 0, so on the device placements this is
                  the explicit call plus the status kernel and one readback of the status words;
  complete_moved  the same list with the head of segment 5 replaced by candidate 0 with an odd scalar: that segment moves to
                  candidate 1.  complete_moved - complete is the cost of one more round (on the device placements: start, scan,
                  rebase, status and the readback; in placement 0 one more pass of the host derivation over that segment);
and, on G1ExpStark(128) with the batch prover, 100 such segments through prove_msms (explicit starts) and prove_msms_complete.
All forms of one table and placement are measured in the same run, alternating, medians and min-max of --calls calls each after
a warm-up of every form.  Writes the JSON file and prints one row per form.

    python tools/complete_sums_time.py [--out profiles/complete_sums_time.json] [--calls 20]
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


def timed_together(calls, forms):
    """{name: stats}: the forms run one after the other inside every round, so that a drift of the box hits all of them alike."""
    wall = {name: [] for name in forms}
    for _ in range(calls):
        for name, f in forms.items():
            t0 = time.perf_counter()
            f()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"host_clock_ms": {"median": statistics.median(w), "min": min(w), "max": max(w)}, "calls": len(w)} for name, w in wall.items()}


def seeded_terms(S, table, count, seed):
    from bench import synthetic_ios
    w = 16 if table == "g1" else 32
    ios = synthetic_ios(count, seed, table)
    return np.ascontiguousarray(np.concatenate([ios[:, :w], ios[:, 2 * w:]], axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complete_sums_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--inflight", type=int, default=3)
    args = ap.parse_args()
    if args.calls < 20:
        raise SystemExit("at least 20 calls per form")
    import starky_bn254_amd as S
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("complete_sums_time.py needs a GPU")
    rows = {}
    lengths = [10] * 12
    for table, cls in (("g1", S.G1ExpStark), ("g2", S.G2ExpStark)):
        stark = cls(128)
        w = 16 if table == "g1" else 32
        terms = seeded_terms(S, table, 120, args.seed)
        moved = terms.copy()
        moved[50, :w] = S.start_candidate(stark, 0)
        moved[50, w] |= 1
        _, eff, starts, choice, _, _, _ = S.msm_batch_instances_complete(stark, terms, lengths)
        assert not choice.any() and np.array_equal(eff, terms)
        assert S.msm_batch_instances_complete(stark, moved, lengths)[3].tolist() == [0] * 5 + [1] + [0] * 6
        for chain in ("0", "1", "2"):
            os.environ["SBN_TRACEGEN_DEVICE_CHAIN"] = chain
            pr = S.Prover(stark, stark.config(), 16)
            del os.environ["SBN_TRACEGEN_DEVICE_CHAIN"]
            forms = {"explicit": lambda: pr.generate_trace_msms(terms, lengths, starts),
                     "complete": lambda: pr.generate_trace_msms_complete(terms, lengths),
                     "complete_moved": lambda: pr.generate_trace_msms_complete(moved, lengths)}
            want = pr.generate_trace_msms(terms, lengths, starts)
            got = pr.generate_trace_msms_complete(terms, lengths)
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[4], got[7])       # the same public inputs and list
            for f in forms.values():
                f()
            for name, r in timed_together(args.calls, forms).items():
                rows[f"{table} chain={chain} {name}"] = r
            pr.close()
    stark = S.G1ExpStark(128)
    terms = seeded_terms(S, "g1", 1000, args.seed)
    lengths = [10] * 100
    _, eff, starts, choice, _, _, _ = S.msm_batch_instances_complete(stark, terms, lengths)
    assert not choice.any()
    bp = S.BatchProver(stark, stark.config(), 16, inflight=args.inflight)
    forms = {"prove_msms": lambda: bp.prove_msms(terms, lengths, starts), "prove_msms_complete": lambda: bp.prove_msms_complete(terms, lengths)}
    a, b = forms["prove_msms"](), forms["prove_msms_complete"]()
    assert all(np.array_equal(p.words, q.words) for p, q in zip(a[0], b[0])) and len(a[0]) == 8
    for name, r in timed_together(args.calls, forms).items():
        rows[f"g1 batch {name}"] = r
    bp.close()
    for name, r in rows.items():
        h = r["host_clock_ms"]
        print(f"| {name} | {h['median']:.2f} ({h['min']:.2f}-{h['max']:.2f}) ms |", flush=True)
    out = {"workload": f"G1ExpStark(128) / G2ExpStark(128): one unit of 12 segments of 10 terms (seeded points and exponents of bench.py, seed {args.seed}), "
                       "starts = candidate 0; complete_moved: the head of segment 5 is candidate 0 with an odd scalar, so that segment takes candidate 1; "
                       f"batch: 100 segments of 10 terms = 8 units, inflight {args.inflight}; {args.calls} calls per form, the forms of one table and "
                       "placement alternating inside every round, after a warm-up of every form",
           "clock": "host_clock_ms: perf_counter around the whole call",
           "columns": "| table, placement (SBN_TRACEGEN_DEVICE_CHAIN), form | host clock median (min-max) |", "forms": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
