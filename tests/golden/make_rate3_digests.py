#!/usr/bin/env python3
"""Writes tests/golden/rate3_digests.json: the sha256 of the CPU oracle's proof words (little-endian u64) and of the public inputs,
at rate_bits 3 under StarkConfig.for_rate(3) (cap 4, 16 grinding bits, arity 4, final 5, 28 queries), of the parity kit's inputs:
G1ExpStark(128) seed 1, FqExpStark(128) seed 4, Fq12ExpU64Stark(16) seed 5.  CPU only; the G1 proof takes the oracle a minute or more, which is why tests/test_rate_gpu.py compares digests and never runs the oracle on these tables.

usage: python tests/golden/make_rate3_digests.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O          # noqa: E402
import rate_oracle as R         # noqa: E402
from parity_kit import sha      # noqa: E402

ROW = (4, 16, 4, 5, 28)
CASES = [("g1exp", O.AIR_G1_EXP, 128, 1, O.g1exp_inputs, O.g1exp_trace),
         ("fqexp", O.AIR_FQ_EXP, 128, 4, O.fqexp_inputs, O.fqexp_trace),
         ("fq12expu64", O.AIR_FQ12_EXP_U64, 16, 5, O.fq12expu64_inputs, O.fq12expu64_trace)]


def main():
    out = {"rate_bits": 3, "config": list(ROW), "cases": {}}
    for name, kind, num_io, seed, inputs, trace_of in CASES:
        ios, _ = inputs(num_io, seed)
        trace, pi = trace_of(ios)
        words, secs = R.prove(kind, num_io, trace, pi, 3, ROW)
        assert R.verify(kind, num_io, words, 3, ROW) == (0, "")
        out["cases"][name] = {"num_io": num_io, "seed": seed, "proof_words": int(len(words)), "proof_sha256": sha(words), "public_inputs_sha256": sha(pi)}
        print(name, out["cases"][name], f"oracle prove {secs:.1f} s", flush=True)
    with open(os.path.join(HERE, "rate3_digests.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
