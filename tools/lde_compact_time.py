#!/usr/bin/env python3
"""What compact LDE storage (Prover(..., lde="compact")) costs and saves at rate_bits 3, in one process on the GPU box.

For G1ExpStark(128) (2^16 rows) and Fq12ExpU64Stark(16) (2^11 rows) under StarkConfig.for_rate(3): one full and one compact context,
the witness generated on the device once, then --warmup prove() calls each and --calls timed prove() calls ALTERNATING between the
two, so that both see the same clocks and the same neighbours.  Recorded per mode: median / min / max of the host clock around
prove(), the mean of stage_times(), dev_bytes of describe() and prover_memory_plan(); per table the ratio of the two medians and
whether the two proofs are the same words.  When compact is more than 10 % slower on G1ExpStark(128), the stage that carries the
difference is named and the query stage's rate is set against its multiply-add count.

For Fq12ExpStark(512) (2^18 rows, config[4]) compact only, and only if the device's free memory covers the plan: device witness time,
three prove() calls, the proof's bytes, dev_bytes, and the host verifier's verdict; otherwise "skipped" with both figures.

    python tools/lde_compact_time.py [--out profiles/lde_compact_time.json] [--calls 20] [--warmup 3] [--no-large]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TABLES = [("G1ExpStark", 128, 16, "g1exp_inputs", 1), ("Fq12ExpU64Stark", 16, 11, "fq12expu64_inputs", 5)]   # class, instances, degree bits, inputs, seed
LARGE = ("Fq12ExpStark", 512, 18, "fq12exp_inputs", 3)


def free_device_bytes():
    """(free, total) of the current device as HIP reports them."""
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    rc = hip.hipMemGetInfo(C.byref(free), C.byref(total))
    if rc != 0:
        raise SystemExit(f"hipMemGetInfo failed ({rc})")
    return int(free.value), int(total.value)


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lde_compact_time.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-large", action="store_true", help="leave Fq12ExpStark(512) out")
    args = ap.parse_args()
    import starky_bn254_amd as S
    import oracle_lib as O   # seeded input generators only
    if S.lib().sbn_device_count() < 1:
        raise SystemExit("lde_compact_time.py needs a GPU")
    S.lib().sbn_set_device(0)
    cfg = S.StarkConfig.for_rate(3)
    out = {"calls": args.calls, "warmup": args.warmup, "rate_bits": 3, "num_query_rounds": int(cfg.num_query_rounds), "tables": {}}
    for cls, num_io, bits, inputs, seed in TABLES:
        stark = getattr(S, cls)(num_io)
        name = f"{cls}({num_io})"
        ios = getattr(O, inputs)(num_io, seed)[0]
        ctx = {}
        for mode in ("full", "compact"):
            p = S.Prover(stark, cfg, bits, lde=mode)
            p.generate_trace(ios)
            for _ in range(args.warmup):
                proof = p.prove()
            ctx[mode] = {"prover": p, "proof": proof, "wall": [], "stages": {}}
        for _ in range(args.calls):
            for mode in ("full", "compact"):
                c = ctx[mode]
                t0 = time.perf_counter()
                c["proof"] = c["prover"].prove()
                c["wall"].append((time.perf_counter() - t0) * 1e3)
                for k, v in c["prover"].stage_times().items():
                    c["stages"][k] = c["stages"].get(k, 0.0) + v / args.calls
        rec = {}
        for mode in ("full", "compact"):
            c = ctx[mode]
            d = c["prover"].describe()
            rec[mode] = {"prove_ms": summary(c["wall"]), "stage_ms_mean": {k: round(v, 4) for k, v in c["stages"].items()},
                         "dev_bytes": int(d["dev_bytes"]), "memory_plan": S.prover_memory_plan(stark, cfg, bits, lde=mode),
                         "lde_ring": int(d["lde_ring"]), "lde_ring_bytes": int(d["lde_ring_bytes"]), "ntt_chunk": int(d["ntt_chunk"]),
                         "ntt_streams": int(d["ntt_streams"])}
            c["prover"].close()
        rec["same_proof_words"] = bool((ctx["full"]["proof"].words == ctx["compact"]["proof"].words).all())
        S.verify_stark_proof(stark, ctx["compact"]["proof"], cfg)
        rec["ratio_compact_over_full"] = rec["compact"]["prove_ms"]["median"] / rec["full"]["prove_ms"]["median"]
        if rec["ratio_compact_over_full"] > 1.10:
            fs, cs = rec["full"]["stage_ms_mean"], rec["compact"]["stage_ms_mean"]
            stages = [k for k in fs if not k.endswith("_launches") and not k.endswith("kernels_ms") and k not in ("device_tracegen_ms", "split_exchange_ms")]
            worst = max(stages, key=lambda k: cs[k] - fs[k])
            macs = (stark.num_columns + stark.num_permutation_zs(cfg)) * int(cfg.num_query_rounds) * (1 << bits)
            rec["slower_than_10_percent"] = {
                "stage_with_largest_difference": worst, "difference_ms": {k: round(cs[k] - fs[k], 4) for k in stages},
                "query_rows_multiply_adds": macs,
                # 8 VALU instructions per multiply-add (Acc<F>::macv: 4 v_mad_u64_u32 + 4 v_addc), the rest of the loop aside
                "query_rows_valu_instructions": 8 * macs,
                "queries_stage_ms": cs["queries"],
                "achieved_multiply_adds_per_s": macs / (cs["queries"] * 1e-3) if cs["queries"] > 0 else None}
        out["tables"][name] = rec
        print(f"{name}: full {rec['full']['prove_ms']['median']:.2f} ms / {rec['full']['dev_bytes'] / 1e9:.2f} GB, compact "
              f"{rec['compact']['prove_ms']['median']:.2f} ms / {rec['compact']['dev_bytes'] / 1e9:.2f} GB, ratio {rec['ratio_compact_over_full']:.3f}, "
              f"same words {rec['same_proof_words']}", flush=True)
    if not args.no_large:
        cls, num_io, bits, inputs, seed = LARGE
        stark = getattr(S, cls)(num_io)
        name = f"{cls}({num_io})"
        plan = S.prover_memory_plan(stark, cfg, bits, lde="compact")
        free, total = free_device_bytes()
        rec = {"memory_plan_compact": plan, "memory_plan_full": S.prover_memory_plan(stark, cfg, bits, lde="full"), "device_free_bytes": free,
               "device_total_bytes": total}
        if free < plan + (2 << 30):   # 2 GiB of headroom for the runtime's own allocations
            rec["status"] = "skipped"
        else:
            ios = getattr(O, inputs)(num_io, seed)[0]
            p = S.Prover(stark, cfg, bits, lde="compact")
            try:
                t0 = time.perf_counter()
                p.generate_trace(ios)
                rec["device_witness_ms"] = (time.perf_counter() - t0) * 1e3
                wall = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    proof = p.prove()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    print(f"{name}: prove() {wall[-1]:.1f} ms", flush=True)
                rec["prove_ms"] = wall
                rec["stage_ms_last"] = {k: round(v, 3) for k, v in p.stage_times().items()}
                rec["proof_bytes"] = len(proof.to_bytes())
                rec["dev_bytes"] = int(p.describe()["dev_bytes"])
            finally:
                p.close()
            t0 = time.perf_counter()
            S.verify_stark_proof(stark, proof, cfg)   # raises unless the proof is accepted
            rec["host_verify_ms"] = (time.perf_counter() - t0) * 1e3
            rec["status"] = "proved and verified"
        out["tables"][name] = rec
        print(f"{name}: {rec['status']}, plan {plan / 1e9:.1f} GB, free {free / 1e9:.1f} GB", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
