#!/usr/bin/env python3
"""What rate_bits 3 (28 queries) costs against rate_bits 1 (84 queries) at the same conjectured security, in one process on the GPU
box.  For G1ExpStark(128) (2^16 rows) and Fq12ExpU64Stark(16) (2^11 rows): one prover per rate, the witness generated on the
device once, then --warmup prove() calls each and --calls timed prove() calls ALTERNATING between the two rates, so that both see
the same clocks and the same neighbours.  Recorded per rate: median / min / max of the host clock around prove(), the mean of
stage_times(), the proof's bytes, dev_bytes of describe(), and the host sbn_verify time (median of 5).  Recorded per table: the ratio
of the two medians, and beside it the rate-1 time the parent commit recorded for the same table where profiles/ has one.

Expectation written down before the first run: a ratio BELOW 4 -- hashing, the LDE's writes and the FRI combination grow by 4, the
transforms by 4 x 19/17, witness, Z, quotient evaluation and openings do not grow.  If it is above 4 the stage means say where.

    python tools/rate_time.py [--out profiles/rate_time.json] [--calls 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TABLES = [("G1ExpStark", 128, 16, "g1exp_inputs", 1), ("Fq12ExpU64Stark", 16, 11, "fq12expu64_inputs", 5)]   # class, instances, degree bits, inputs, seed


def parent_rate1_ms(name):
    """(file, ms per proof) the parent commit recorded at rate 1, or None."""
    if name == "G1ExpStark(128)":
        f = os.path.join("profiles", "r4_v5_bench.json")
        try:
            return f, json.load(open(os.path.join(ROOT, f)))["ms_per_step"]
        except (OSError, KeyError, ValueError):
            return None
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import starky_bn254_amd as S
    import oracle_lib as O   # seeded input generators only
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("rate_time.py needs a GPU")
    out = {"calls": args.calls, "warmup": args.warmup, "rates": {"1": 84, "3": 28}, "tables": {}}
    for cls, num_io, bits, inputs, seed in TABLES:
        stark = getattr(S, cls)(num_io)
        name = f"{cls}({num_io})"
        ios = getattr(O, inputs)(num_io, seed)[0]
        ctx = {}
        for r in (1, 3):
            cfg = S.StarkConfig.for_rate(r)
            p = S.Prover(stark, cfg, bits)
            p.generate_trace(ios)
            for _ in range(args.warmup):
                proof = p.prove()
            ctx[r] = {"cfg": cfg, "prover": p, "proof": proof, "wall": [], "stages": {}}
        for _ in range(args.calls):
            for r in (1, 3):
                c = ctx[r]
                t0 = time.perf_counter()
                c["proof"] = c["prover"].prove()
                c["wall"].append((time.perf_counter() - t0) * 1e3)
                for k, v in c["prover"].stage_times().items():
                    c["stages"][k] = c["stages"].get(k, 0.0) + v / args.calls
        rec = {}
        for r in (1, 3):
            c = ctx[r]
            vt = []
            for _ in range(5):
                t0 = time.perf_counter()
                S.verify_stark_proof(stark, c["proof"], c["cfg"])
                vt.append((time.perf_counter() - t0) * 1e3)
            d = c["prover"].describe()
            rec[str(r)] = {"num_query_rounds": int(c["cfg"].num_query_rounds),
                           "prove_ms": {"median": statistics.median(c["wall"]), "min": min(c["wall"]), "max": max(c["wall"])},
                           "stage_ms_mean": {k: round(v, 4) for k, v in c["stages"].items()},
                           "proof_bytes": len(c["proof"].to_bytes()), "dev_bytes": int(d["dev_bytes"]),
                           "host_verify_ms_median": statistics.median(vt),
                           "switches": {k: d[k] for k in ("ntt_chunk", "ntt_fused", "ntt_streams", "ntt_split1024", "ntt_lde_zero_aware")}}
            c["prover"].close()
        rec["ratio_rate3_over_rate1"] = rec["3"]["prove_ms"]["median"] / rec["1"]["prove_ms"]["median"]
        par = parent_rate1_ms(name)
        rec["parent_rate1"] = {"file": par[0], "ms_per_proof": par[1]} if par else None
        out["tables"][name] = rec
        print(f"{name}: rate 1 {rec['1']['prove_ms']['median']:.2f} ms ({rec['1']['proof_bytes']} B), rate 3 {rec['3']['prove_ms']['median']:.2f} ms "
              f"({rec['3']['proof_bytes']} B), ratio {rec['ratio_rate3_over_rate1']:.2f}, parent rate 1 {par[1] if par else 'not recorded'}", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
