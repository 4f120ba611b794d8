"""Shared by tests/test_explain_host.py and tests/test_explain_gpu.py: the corrupted traces the explain tests look at (the cells of
tests/check_trace_cases.py) and the independent, exact reference for "which constraints are non-zero on a row".

The reference is the oracle's constraint-by-constraint evaluator.  orc_eval_constraints returns acc_j = sum_t c_t alpha_j^(n-1-t)
for any number of alphas; with alpha_j = w^j, w a K-th root of unity, K a power of two >= n, the returned vector is the DFT of
e -> c_(n-1-e), and an inverse NTT recovers every c_t exactly, selectors included.  No challenge of the library enters it."""
import functools

import numpy as np

import check_trace_cases as K
import oracle_lib as O

P = O.GL_P
ROOT_2_32 = 1753635133440165772        # of order 2^32
SEED = 0x9E3779B97F4A7C15
FQ12 = ("fq12exp", "fq12exp_u64")      # 10,047 and 11,744 constraints: rows 0, 255, n - 1 only, one trace copy


def _inverse_ntt(vals, w):
    """c with vals[j] = sum_e c[e] w^(j e), w of order len(vals) (a power of two)."""
    k = len(vals)
    lg = k.bit_length() - 1
    a = [0] * k
    for i, v in enumerate(vals):
        a[int(format(i, f"0{lg}b")[::-1], 2) if lg else 0] = v
    w_inv = pow(w, P - 2, P)
    size = 2
    while size <= k:
        step = pow(w_inv, k // size, P)
        half = size // 2
        tw = [1] * half
        for i in range(1, half):
            tw[i] = tw[i - 1] * step % P
        for s in range(0, k, size):
            for i in range(half):
                u, v = a[s + i], a[s + i + half] * tw[i] % P
                a[s + i], a[s + i + half] = (u + v) % P, (u - v) % P
        size *= 2
    k_inv = pow(k, P - 2, P)
    return [x * k_inv % P for x in a]


def oracle_constraints(c, trace, i):
    """[c_0, .., c_(n-1)]: the value of every constraint of the table on row i of `trace` (against row i + 1 mod N), in emission
    order, from the oracle."""
    stark, rows = c["stark"], c["n"]
    n = stark.num_constraints
    k = 1 << max(n - 1, 1).bit_length()
    w = pow(ROOT_2_32, (1 << 32) // k, P)
    alphas, a = [], 1
    for _ in range(k):
        alphas.append(a)
        a = a * w % P
    g = pow(ROOT_2_32, 1 << (32 - (rows.bit_length() - 1)), P)
    z_last = (pow(g, i, P) - pow(g, rows - 1, P)) % P
    lv, nv = np.ascontiguousarray(trace[:, i]), np.ascontiguousarray(trace[:, (i + 1) % rows])
    acc = O.eval_constraints(stark.kind, stark.num_io, lv, nv, c["pi"], alphas, z_last, int(i == 0), int(i == rows - 1))
    d = _inverse_ntt(acc, w)           # d[e] = the constraint with alpha-exponent e = c_(n-1-e)
    assert not any(d[n:]), "the oracle emitted more constraints than sbn_air_num_constraints"
    return d[:n][::-1]


def block_firsts(stark):
    return np.array([b.first for b in stark.constraint_blocks()], dtype=np.int64)


def oracle_blocks(c, trace, i):
    """The blocks of the table that contain a constraint the oracle finds non-zero on row i."""
    ct = oracle_constraints(c, trace, i)
    nz = np.array([t for t, v in enumerate(ct) if v], dtype=np.int64)
    return set(int(b) for b in np.searchsorted(block_firsts(c["stark"]), nz, side="right") - 1)


def flagged(row_explanation):
    return {b.index for b in row_explanation.blocks}


@functools.lru_cache(maxsize=None)
def corrupted(name):
    """[(cells, trace copy with those cells changed, rows to look at)]: one entry per cell of K.corruptions(name) with rows
    {r - 1, r}; for the two Fq12 tables ONE entry with the cells of rows 0, 255, n - 1 in one copy."""
    c = K.case(name)
    n = c["n"]
    out = []
    if name in FQ12:
        cells = [(r, col) for r in (0, 255, n - 1) for col in c["cols"]]
        rows = sorted({(r + d) % n for r, _ in cells for d in (-1, 0)})
        out.append((tuple(cells), K.corrupt(c["trace"], cells), rows))
    else:
        for r, col in K.corruptions(name):
            out.append((((r, col),), K.corrupt(c["trace"], [(r, col)]), sorted({(r - 1) % n, r})))
    for _, t, _ in out:
        t.setflags(write=False)
    return out


def gpu_rows(name):
    """The rows the device tests list: those of check_trace_cases (0, 1, 255 | 256 = the workgroup boundary, n - 1, the instance
    boundary) and their predecessors."""
    c = K.case(name)
    return sorted({(r + d) % c["n"] for r in c["rows"] for d in (-1, 0)})
