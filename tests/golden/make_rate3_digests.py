#!/usr/bin/env python3
"""Writes tests/golden/rate3_digests.json: the word count and sha256 of the CPU oracle's proof words (little-endian u64) and, for the
tables with public inputs, the sha256 of those, at rate_bits 3 under StarkConfig.for_rate(3) (cap 4, 16 grinding bits, arity 4,
final 5, 28 queries).  The Exp tables take the parity kit's inputs: G1ExpStark(128) seed 1, FqExpStark(128) seed 4,
Fq12ExpU64Stark(16) seed 5, G2ExpStark(128) seed 2, Fq12ExpStark(16) seed 3; lookup18 / lookup19 / lookup20 are LookupStark at 2^18,
2^19 and 2^20 rows on O.lookup_inputs(1 << bits, 200 + bits).  Every proof is accepted by the oracle's verifier before it is written.

CPU only.  tests/test_rate_gpu.py compares digests and never runs the oracle on these tables, because of what the oracle takes
(orc_prove_rate's own seconds when the entries were written, on a CPU that other builds shared):
  fq12expu64 13.1 s, fqexp 35.6 s, fq12exp 61.4 s, g1exp 85.8 s, g2exp 210.1 s; lookup18 10.7 s, lookup19 20.3 s, lookup20 42.2 s
All eight take eight minutes of wall time, G2ExpStark(128) alone three and a half; traces and verification add a few seconds each.

usage: python tests/golden/make_rate3_digests.py [--only NAME...] [--out PATH]
  --only NAME...  recompute these entries alone; every other entry is copied from the committed file
  --out PATH      write there instead of tests/golden/rate3_digests.json"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np              # noqa: E402
import oracle_lib as O          # noqa: E402
import rate_oracle as R         # noqa: E402
from parity_kit import sha      # noqa: E402

ROW = (4, 16, 4, 5, 28)
JSON = os.path.join(HERE, "rate3_digests.json")
# name -> (oracle kind, num_io, seed, inputs, trace)
EXP = {"g1exp": (O.AIR_G1_EXP, 128, 1, O.g1exp_inputs, O.g1exp_trace),
       "fqexp": (O.AIR_FQ_EXP, 128, 4, O.fqexp_inputs, O.fqexp_trace),
       "fq12expu64": (O.AIR_FQ12_EXP_U64, 16, 5, O.fq12expu64_inputs, O.fq12expu64_trace),
       "g2exp": (O.AIR_G2_EXP, 128, 2, O.g2exp_inputs, O.g2exp_trace),
       "fq12exp": (O.AIR_FQ12_EXP, 16, 3, O.fq12exp_inputs, O.fq12exp_trace)}
LOOKUP = {"lookup18": 18, "lookup19": 19, "lookup20": 20}   # name -> degree_bits; seed 200 + degree_bits
NAMES = list(EXP) + list(LOOKUP)


def entry(name):
    """-> (the JSON entry of one case, the oracle's seconds for the proof)"""
    if name in EXP:
        kind, num_io, seed, inputs, trace_of = EXP[name]
        trace, pi = trace_of(inputs(num_io, seed)[0])
        e = {"num_io": num_io, "seed": seed}
    else:
        bits = LOOKUP[name]
        kind, num_io, seed, pi = O.AIR_LOOKUP, 0, 200 + bits, np.zeros(0, dtype=np.uint64)
        trace = O.lookup_trace(*O.lookup_inputs(1 << bits, seed))
        e = {"degree_bits": bits, "seed": seed}
    words, secs = R.prove(kind, num_io, trace, pi, 3, ROW)
    assert R.verify(kind, num_io, words, 3, ROW) == (0, "")
    e.update(proof_words=int(len(words)), proof_sha256=sha(words))
    if name in EXP:
        e["public_inputs_sha256"] = sha(pi)
    return e, secs


def main(argv=None):
    ap = argparse.ArgumentParser(description="the oracle's rate-3 proof digests")
    ap.add_argument("--only", nargs="+", choices=NAMES, metavar="NAME", help="recompute these entries alone: " + " ".join(NAMES))
    ap.add_argument("--out", default=JSON)
    args = ap.parse_args(argv)
    out = {"rate_bits": 3, "config": list(ROW), "cases": {}}
    if args.only:
        with open(JSON) as f:
            old = json.load(f)
        assert (old["rate_bits"], old["config"]) == (out["rate_bits"], out["config"])
        out["cases"] = old["cases"]
    for name in args.only or NAMES:
        out["cases"][name], secs = entry(name)
        print(name, out["cases"][name], f"oracle prove {secs:.1f} s", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
