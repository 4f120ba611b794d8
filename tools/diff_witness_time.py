#!/usr/bin/env python3
"""Times Prover.diff_witness on G1ExpStark(128) (2^16 rows x 1,676 columns) and Fq12ExpStark(16) (2^13 x 9,802), in one process on the
GPU box, beside Prover.generate_trace, Prover.check_trace and Prover.explain_rows on the same context: the diff of the clean
device witness, of a copy with ONE wrong cell, of a copy in which EVERY main cell from row n / 2 on is wrong, and the host twin
(diff_witness_host on the clean trace, SBN_HOST_THREADS=16 unless set).  Every case: --warmups calls, then the median of --calls
calls timed on the host clock around the whole call; the split of the median device call is the library's own (device witness and
compare kernel by HIP events, listing + downloads by the host clock).  The device result must equal the host twin's, and be clean
/ differing as built.

    python tools/diff_witness_time.py [--out profiles/diff_witness_time.json] [--calls 20] [--warmups 3]
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
P = 0xFFFFFFFF00000001


def timed(f, *a, **k):
    t0 = time.perf_counter()
    r = f(*a, **k)
    return (time.perf_counter() - t0) * 1e3, r


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls_ms": v}


def series(calls, warmups, f, *a, **k):
    for _ in range(warmups):
        f(*a, **k)
    return [timed(f, *a, **k)[0] for _ in range(calls)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diff_witness_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    import numpy as np
    import starky_bn254_amd as S
    from bench import synthetic_ios, synthetic_ios_fq12
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("diff_witness_time.py needs a GPU")
    tables = {}
    for name, stark, bits, table in (("G1ExpStark(128)", S.G1ExpStark(128), 16, "g1"), ("Fq12ExpStark(16)", S.Fq12ExpStark(16), 13, "fq12")):
        n, C_, num_main = 1 << bits, stark.num_columns, stark.num_main_columns
        ios = synthetic_ios(stark.num_io, args.seed) if table == "g1" else synthetic_ios_fq12(stark.num_io, args.seed)
        prover = S.Prover(stark, stark.config(), bits)
        pi = prover.generate_trace(ios)
        clean = prover.read_trace()
        one = clean.copy()
        one[217, 513] = (int(one[217, 513]) + 1) % P
        half = clean.copy()
        v = half[:num_main, n // 2:] + np.uint64(1)
        half[:num_main, n // 2:] = np.where(v == np.uint64(P), np.uint64(0), v)
        entry = {"generate_trace": summary(series(args.calls, args.warmups, prover.generate_trace, ios))}
        want = {"clean": 0, "one_wrong_cell": 1, "every_main_cell_from_row_n_2": num_main * (n // 2)}
        for case, trace in (("clean", clean), ("one_wrong_cell", one), ("every_main_cell_from_row_n_2", half)):
            prover.load_trace(trace, pi)
            for _ in range(args.warmups):
                dev = prover.diff_witness()
            assert dev.main_cells == want[case] and dev.ok == (case == "clean") and dev == S.diff_witness_host(stark, trace, pi)
            t, split = [], []
            for _ in range(args.calls):
                ms, d = timed(prover.diff_witness)
                t.append(ms)
                split.append(prover.diff_times())
                assert d == dev
            e = summary(t)
            mid = sorted(range(args.calls), key=lambda i: t[i])[args.calls // 2]
            e["split_ms_of_median_call"] = split[mid]
            e["cells"], e["main_cells"], e["rows"], e["columns"], e["listed"] = dev.cells, dev.main_cells, dev.rows, dev.columns, len(dev.raw_cells)
            entry["diff_witness " + case] = e
            if case == "one_wrong_cell":
                entry["check_trace"] = summary(series(args.calls, args.warmups, prover.check_trace, seed=args.seed))
                entry["explain_rows"] = summary(series(args.calls, args.warmups, prover.explain_rows, [513], seed=args.seed))
                entry["first_listed_cell"] = str(dev).split("; ")[1]
        entry["diff_witness_host clean"] = summary(series(args.calls, args.warmups, S.diff_witness_host, stark, clean, pi))
        entry["bytes_of_both_matrices"] = 2 * 8 * C_ * n
        prover.close()
        tables[name] = entry
        print(name, {k: round(x["median_ms"], 3) for k, x in entry.items() if isinstance(x, dict)}, flush=True)
    out = {"workload": f"device witness of bench.synthetic_ios / synthetic_ios_fq12 (seed {args.seed}); 'one_wrong_cell' = (v + 1) mod p in row 513 of column 217; 'every_main_cell_from_row_n_2' = the same "
                       f"in every main column from row n / 2 on; cells = 16 listed; every case {args.warmups} warm-ups, then {args.calls} calls; the host twin on "
                       f"{os.environ['SBN_HOST_THREADS']} threads",
           "clock": "host perf_counter around the whole call; split_ms: device witness and compare kernel by HIP events on the prover's stream, listing + downloads by the host clock",
           "tables": tables}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
