#!/usr/bin/env python3
"""Times the batch verifier against the host verifier on G1ExpStark(128) proofs (2^16 rows, ~1.9 MB each), in one process on the
GPU box.  BatchProver makes the proofs from seeds; for batch sizes 1, 16 and 256 three forms alternate for --rounds rounds:

    host_1    the sbn_verify loop on one host thread
    host_16   the same loop on 16 host threads
    device    Verifier.verify (one call for the whole batch)

each timed on the host clock around the whole call.  Reported: median (min-max) per form and size, the device stage split by HIP
events (upload, kernels, download) of the median device round, and whether the slowest device round beats the fastest round of
the one-thread loop at batch 256 (the acceptance bar).  Every verdict must be 0.  Writes the JSON file and prints one row for the
table of DESIGN.md section 7.

    python tools/verify_time.py [--out profiles/verify_batch_time.json] [--rounds 5] [--sizes 1,16,256]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NUM_IO, DEGREE_BITS, HOST_THREADS = 128, 16, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch_time.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    if args.rounds < 5:
        raise SystemExit("at least five rounds")
    from starky_bn254_amd import sharding
    os.environ.setdefault("SBN_HOST_THREADS", str(max(1, min(64, sharding.effective_cpus()))))
    import numpy as np
    import starky_bn254_amd as S
    from bench import synthetic_ios
    L = S.lib()
    if L.sbn_device_count() < 1:
        raise SystemExit("verify_time.py needs a GPU")
    stark = S.G1ExpStark(NUM_IO)
    cfg = stark.config()
    nmax = max(sizes)
    t0 = time.perf_counter()
    ios = np.stack([synthetic_ios(NUM_IO, args.seed + u, "g1") for u in range(nmax)])
    bp = S.BatchProver(stark, cfg, DEGREE_BITS, 3)
    proofs = bp.prove_ios(ios)
    bp.close()
    blobs = [p.to_bytes() for p in proofs]
    print(f"{nmax} proofs of {len(blobs[0])} bytes in {time.perf_counter() - t0:.1f} s", flush=True)

    def host_one(b):
        return L.sbn_verify(C.byref(stark._d), C.byref(cfg._c), b, len(b))

    def host_1(batch):
        return [host_one(b) for b in batch]

    pool = ThreadPoolExecutor(HOST_THREADS)

    def host_16(batch):
        return list(pool.map(host_one, batch))

    verifier = S.Verifier(stark, cfg, DEGREE_BITS, max_batch=nmax)

    def device(batch):
        return [code for code, _ in verifier.verify(batch)]

    forms = [("host_1", host_1), ("host_16", host_16), ("device", device)]
    device(blobs[:1])   # warm-up: the kernel's code object, the pinned ring's first touch
    host_16(blobs[:HOST_THREADS])
    results = {}
    for n in sizes:
        batch = blobs[:n]
        times = {name: [] for name, _ in forms}
        stages = []
        for _ in range(args.rounds):
            for name, f in forms:
                t0 = time.perf_counter()
                codes = f(batch)
                dt = time.perf_counter() - t0
                assert codes == [0] * n, (name, n, codes)
                times[name].append(dt * 1e3)
                if name == "device":
                    stages.append(verifier.stage_times())
        entry = {}
        for name, ts in times.items():
            entry[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "rounds_ms": ts,
                           "median_ms_per_proof": statistics.median(ts) / n}
        mid = sorted(range(args.rounds), key=lambda i: times["device"][i])[args.rounds // 2]
        entry["device"]["stage_ms_of_median_round"] = stages[mid]
        entry["device_slowest_vs_host_1_fastest"] = entry["host_1"]["min_ms"] / entry["device"]["max_ms"]
        entry["device_median_vs_host_16_median"] = entry["host_16"]["median_ms"] / entry["device"]["median_ms"]
        results[str(n)] = entry
        print(n, {k: (round(v["median_ms"], 2), round(v["min_ms"], 2), round(v["max_ms"], 2)) for k, v in entry.items() if isinstance(v, dict)},
              entry["device"]["stage_ms_of_median_round"], flush=True)
    verifier.close()
    pool.shutdown()
    big = results[str(nmax)]
    bar = big["device"]["max_ms"] < big["host_1"]["min_ms"]
    out = {"workload": f"G1ExpStark({NUM_IO}) proofs, 2^{DEGREE_BITS} rows, {len(blobs[0])} bytes each, seeds {args.seed}..{args.seed + nmax - 1}, all accepted",
           "forms": {"host_1": "sbn_verify loop, one host thread", "host_16": f"sbn_verify loop, {HOST_THREADS} host threads",
                     "device": "Verifier.verify, one call per batch"},
           "clock": "host perf_counter around the whole call; stage_ms: HIP events on the verifier's stream",
           "rounds": args.rounds, "host_pool_threads": int(os.environ["SBN_HOST_THREADS"]), "batch": results,
           "acceptance": {"rule": f"batch {nmax}: slowest device round faster than the fastest host_1 round", "met": bool(bar)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")

    def cell(e):
        return f"{e['median_ms']:.1f} ({e['min_ms']:.1f}-{e['max_ms']:.1f})"
    for n in sizes:
        e = results[str(n)]
        st = e["device"]["stage_ms_of_median_round"]
        print(f"| {n} | {cell(e['host_1'])} | {cell(e['host_16'])} | {cell(e['device'])} | "
              f"{st.get('upload', 0):.1f} / {st.get('kernels', 0):.1f} / {st.get('download', 0):.2f} |")
    if not bar:
        raise SystemExit("acceptance bar missed: the slowest device round is not faster than the fastest one-thread host round")


if __name__ == "__main__":
    main()
