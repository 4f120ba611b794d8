"""Host A/B of the instance-list derivations (no device): wall time of six host calls on two builds of the library.

usage: instance_lists_host_ab.py <other libsbn254.so> [runs]   -> profiles/instance_lists_host_ab.txt

The two libraries alternate, a fresh process per run (SBN_LIB is read when the package loads the library), SBN_HOST_THREADS=16,
`runs` (default 5) runs each.  Per call: the median and the max - min spread of either library.  The inputs are made once (seeded)
and handed to the runs in a file; every call must return SBN_OK."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "profiles", "instance_lists_host_ab.txt")
CALLS = ["msm_instances G1 4096 terms", "msm_instances FQ_EXP 65536 terms", "msm_instances FQ12_EXP 512 terms", "msm_batch_instances G1 4096 terms, segments of 4",
         "scalar_mul_instances G2 1024 points", "power_instances FQ12_EXP_U64 256 towers of depth 3"]


def make_inputs(path):
    import chained_lists as CL
    import oracle_lib as O
    rng = np.random.default_rng(101)

    def below_p(rows, values):      # `values` field elements of eight u32 limbs per row, each below 2^252 < p
        a = rng.integers(0, 1 << 32, size=(rows, 8 * values), dtype=np.uint64).astype(np.uint32)
        a[:, 7::8] &= 0x0FFFFFFF
        return a

    def exps256(rows):
        return rng.integers(0, 1 << 32, size=(rows, 8), dtype=np.uint64).astype(np.uint32)

    g1 = np.array([CL.value_words("g1", O.g1_random(rng)) for _ in range(4096)], dtype=np.uint32)
    g2 = np.array([CL.value_words("g2", O.g2_random(rng)) for _ in range(1024)], dtype=np.uint32)
    u64 = np.stack([rng.integers(0, 1 << 32, size=256, dtype=np.uint64), rng.integers(0, 0xFFFFFFFF, size=256, dtype=np.uint64)], axis=1).astype(np.uint32)
    np.savez(path, g1_terms=np.concatenate([g1, exps256(4096)], axis=1), fq_terms=np.concatenate([below_p(65536, 1), exps256(65536)], axis=1),
             fq12_terms=np.concatenate([below_p(512, 12), exps256(512)], axis=1), g2_points=g2, g2_scalars=exps256(1024), u64_bases=below_p(256, 12), u64_exps=u64,
             fq_start=below_p(1, 1)[0], fq12_start=below_p(1, 12)[0])


def one_run(path):
    """The six calls on the library SBN_LIB names, one JSON line of seconds."""
    import starky_bn254_amd as S
    import tracegen_edges as T
    with np.load(path) as z:
        d = {k: np.ascontiguousarray(z[k]) for k in z.files}
    L = S.lib()
    p = lambda a: a.ctypes.data   # noqa: E731
    g1_start, num_io = S.generator(S.G1ExpStark(128)), 128
    lengths = np.full(1024, 4, dtype=np.uint64)
    out = np.zeros(1 << 22, dtype=np.uint32)      # room for the largest list (FQ_EXP: 65536 x 24 words)
    fin = np.zeros(1024 * 96, dtype=np.uint32)
    inf = np.zeros(4096, dtype=np.uint8)
    calls = [
        lambda: L.sbn_msm_instances(T.AIR["g1"], p(d["g1_terms"]), 4096, num_io, p(g1_start), p(out), p(fin)),
        lambda: L.sbn_msm_instances(T.AIR["fq"], p(d["fq_terms"]), 65536, num_io, p(d["fq_start"]), p(out), p(fin)),
        lambda: L.sbn_msm_instances(T.AIR["fq12"], p(d["fq12_terms"]), 512, 16, p(d["fq12_start"]), p(out), p(fin)),
        lambda: L.sbn_msm_batch_instances(T.AIR["g1"], p(d["g1_terms"]), p(lengths), 1024, None, 1, num_io, p(out), p(fin), p(fin), p(inf)),
        lambda: L.sbn_scalar_mul_instances(T.AIR["g2"], p(d["g2_points"]), p(d["g2_scalars"]), 1024, 1024, num_io, None, p(out), p(fin), p(inf)),
        lambda: L.sbn_power_instances(T.AIR["fq12u64"], p(d["u64_bases"]), p(d["u64_exps"]), 256, 256, 3, 16, p(out), p(fin)),
    ]
    assert L.sbn_msm_instances(T.AIR["fq"], p(d["fq_terms"]), 64, num_io, p(d["fq_start"]), p(out), p(fin)) == 0    # (starts the host pool)
    secs = []
    for call in calls:
        t0 = time.perf_counter()
        rc = call()
        secs.append(time.perf_counter() - t0)
        assert rc == 0, (rc, L.sbn_last_error().decode())
    print(json.dumps(secs))


def main():
    other, runs = os.path.abspath(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 5
    libs = {"parent": other, "new": os.path.join(ROOT, "starky_bn254_amd", "libsbn254.so")}
    times = {k: [] for k in libs}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "inputs.npz")
        make_inputs(path)
        for _ in range(runs):
            for name, lib in libs.items():
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--run", path], env=dict(os.environ, SBN_LIB=lib, SBN_HOST_THREADS="16"),
                                   capture_output=True, text=True, check=True)
                times[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    lines = [f"# host wall time in ms, SBN_HOST_THREADS=16, {runs} alternating runs per library, a fresh process per run: median (max - min)",
             "# slower = the new median exceeds the parent's median plus the parent's own spread"]
    for i, call in enumerate(CALLS):
        col = {k: [1e3 * run[i] for run in v] for k, v in times.items()}
        med = {k: statistics.median(v) for k, v in col.items()}
        spread = {k: max(v) - min(v) for k, v in col.items()}
        verdict = "slower" if med["new"] > med["parent"] + spread["parent"] else "not slower"
        lines.append(f"{call}: parent {med['parent']:.2f} ({spread['parent']:.2f})  new {med['new']:.2f} ({spread['new']:.2f})  {verdict}")
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if sys.argv[1] == "--run":
        one_run(sys.argv[2])
    else:
        main()
