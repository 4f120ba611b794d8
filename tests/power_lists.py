"""Field powers and power towers over Python integers, for tests/test_powers_host.py and tests/test_powers_gpu.py: Fq by pow(),
Fq12 by a schoolbook product written here (flat basis of the field tables: the coefficient of w^k is c[k] + c[k+6] i, i^2 = -1,
w^6 = 9 + i, as csrc/bn254w.cuh states it), the word shapes of `ios`, and the explicit padded list a tower call stands for."""
import random

import numpy as np

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
BN_X = 4965661367192848881
GLP = (1 << 64) - (1 << 32) + 1
WORDS = {"fq": (8, 8), "fq12": (96, 8), "fq12u64": (96, 2)}     # u32 words of an element, of the exponent


def limbs(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def from_limbs(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


# ---------------------------------------------------------------- Fq12 = Fq2[w] / (w^6 - (9 + i)), Fq2 = Fq[i] / (i^2 + 1)
def _f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def fq12_mul(x, y):
    """x, y: twelve ints in the flat basis -> their product, schoolbook: the degree-10 polynomial in w, then w^6 = 9 + i."""
    xs = [(x[k], x[k + 6]) for k in range(6)]
    ys = [(y[k], y[k + 6]) for k in range(6)]
    prod = [(0, 0)] * 11
    for i in range(6):
        for j in range(6):
            t = _f2mul(xs[i], ys[j])
            prod[i + j] = ((prod[i + j][0] + t[0]) % P, (prod[i + j][1] + t[1]) % P)
    for k in range(10, 5, -1):
        t = _f2mul(prod[k], (9, 1))
        prod[k - 6] = ((prod[k - 6][0] + t[0]) % P, (prod[k - 6][1] + t[1]) % P)
    return [prod[k][0] for k in range(6)] + [prod[k][1] for k in range(6)]


FQ12_ONE = [1] + [0] * 11


def fq12_pow(x, e):
    """Square-and-multiply, most significant bit first (the table walks the other way: the result is the same element)."""
    acc = list(FQ12_ONE)
    for t in range(e.bit_length() - 1, -1, -1):
        acc = fq12_mul(acc, acc)
        if (e >> t) & 1:
            acc = fq12_mul(acc, x)
    return acc


def power(table, x, e):
    return pow(x, e, P) if table == "fq" else fq12_pow(x, e)


def elem_words(table, v):
    return limbs(v, 8) if table == "fq" else [w for c in v for w in limbs(c, 8)]


def elem_from_words(table, ws):
    return from_limbs(ws) if table == "fq" else [from_limbs(ws[8 * c:8 * c + 8]) for c in range(12)]


def random_elem(table, rng):
    return rng.randrange(P) if table == "fq" else [rng.randrange(P) for _ in range(12)]


def base_words(table, bases):
    return np.array([elem_words(table, b) for b in bases], dtype=np.uint32)


def exp_words(table, exps):
    return np.array([limbs(e, WORDS[table][1]) for e in exps], dtype=np.uint32)


def towers(table, bases, exps, depth):
    """powers[k][l] = bases[k]^(e_k^(l+1)) as Python values, level by level; exps: one per tower, or a single shared one."""
    out = []
    for k, b in enumerate(bases):
        e = exps[0] if len(exps) == 1 else exps[k]
        x, levels = b, []
        for _ in range(depth):
            x = power(table, x, e)
            levels.append(x)
        out.append(levels)
    return out


def explicit_units(table, bases, exps, depth, num_io):
    """(units, powers) in words: the list a tower call stands for -- x of its level, offset one, the tower's exponent, tower-major,
    the last unit padded with copies of the last row -- and the outputs (count, depth, W)."""
    w, ew = WORDS[table]
    pw = towers(table, bases, exps, depth)
    one = [1] + [0] * (w - 1)
    rows = []
    for k, b in enumerate(bases):
        e = exps[0] if len(exps) == 1 else exps[k]
        for l in range(depth):
            rows.append(elem_words(table, b if l == 0 else pw[k][l - 1]) + one + limbs(e, ew))
    while len(rows) % num_io:
        rows.append(rows[-1])
    units = np.array(rows, dtype=np.uint32).reshape(-1, num_io, 2 * w + ew)
    powers = np.array([[elem_words(table, v) for v in lv] for lv in pw], dtype=np.uint32)
    return units, powers


def pi_outputs(table, num_io, pi):
    """The outputs among the public inputs of one unit, as (num_io, W) u32 words: u32 limbs in Fq, 16-bit limbs in Fq12."""
    w, ew = WORDS[table]
    pw, pe = (8, 8) if table == "fq" else (192, 8 if table == "fq12" else 1)
    per = 3 * pw + pe
    pi = np.asarray(pi, dtype=np.uint64).reshape(num_io, per)
    out = pi[:, 2 * pw + pe:]
    if table == "fq":
        return out.astype(np.uint32)
    return (out[:, 0::2] | (out[:, 1::2] << np.uint64(16))).astype(np.uint32)


def rng(seed):
    return random.Random(seed)
