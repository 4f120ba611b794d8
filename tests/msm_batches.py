"""Batches of short MSMs: SEGMENTED chained lists (segment s holds lengths[s] consecutive instances; its head starts from the
start of the segment, every other instance from the output before it) for the five Exp tables, derived in plain Python integers
through chained_lists.derive, one segment at a time.  Shared by test_msm_batch_host.py and test_msm_batch_gpu.py.

Python integers (oracle_lib's group and field operations through tracegen_edges) are the reference for every offset, final and
sum, never the code under test.  Every recipe asserts here, on the CPU, that its list walks clean and that the special cases it
is meant to hold are really present, so a changed recipe cannot silently drop a case."""
import functools

import numpy as np

import chained_lists as CL
import msm_lists as ML
import oracle_lib as O
import tracegen_edges as T

P, R, U256 = T.P, T.R, T.U256
CURVE_LENGTHS = [1, 1, 2, 59, 1, 33, 3, 21]          # heads 0, 1, 2, 4, 63, 64, 97, 100; M = 121 in a unit of 128: 7 pads
# M = 300 over units of 128: segment 12 is instances 120 .. 134 (straddles 127|128), segment 24 is 245 .. 264 (straddles 255|256),
# the last unit holds 44 real instances and 84 pads; the same idea over units of 16: M = 37, 15 .. 17 and 30 .. 33 straddle
BATCH_LENGTHS = {"g1": (128, [10] * 12 + [15] + [10] * 11 + [20, 35]), "fq12": (16, [5, 5, 5, 3, 6, 6, 4, 3])}


def heads(lengths):
    return [int(h) for h in np.cumsum([0] + list(lengths))[:-1]]


def derive(table, xs, es, lengths, starts):
    """(insts, finals): the explicit list of the M real instances and the last output of every segment, segment by segment
    through chained_lists.derive; starts: one Python value per segment."""
    insts, finals = [], []
    for s, (h, n) in enumerate(zip(heads(lengths), lengths)):
        seg, fin = CL.derive(table, xs[h:h + n], es[h:h + n], starts[s])
        insts += seg
        finals.append(fin)
    return insts, finals


def sums_of(curve, finals, starts):
    """final_s + (-start_s) by Python's complete addition: None is the point at infinity."""
    add, neg, _ = T._ops(curve)
    return [add(f, neg(st)) for f, st in zip(finals, starts)]


def lengths_words(lengths):
    return np.array(lengths, dtype=np.uint64)


def starts_words(table, starts):
    return np.array([list(CL.value_words(table, st)) for st in starts], dtype=np.uint32)


def point_words(curve, pts):
    """[n][16E] u32; None (the point at infinity) as zero words."""
    w = {"g1": 16, "g2": 32}[curve]
    return np.array([list(CL.value_words(curve, p)) if p is not None else [0] * w for p in pts], dtype=np.uint32)


def flags(pts):
    return np.array([1 if p is None else 0 for p in pts], dtype=np.uint8)


def _rand_exp(rng):
    return int.from_bytes(rng.bytes(32), "little") % R


@functools.lru_cache(maxsize=None)
def curve_unit(curve, shared):
    """The one-unit recipe of the curve tables (np.random.default_rng(7), exponents mod r, CURVE_LENGTHS): e = 0 at the head of
    segment 3; segment 2 = (x, e), (-x, e), whose sum is the point at infinity and whose final equals its start; e = r and
    e = 2^256 - 1 inside segment 3; starts (s + 1) * generator per segment, or (shared) the generator for all.
    Returns (xs, es, starts, insts, finals, sums)."""
    rng = np.random.default_rng(7)
    add, neg, mul = T._ops(curve)
    rnd = O.g1_random if curve == "g1" else O.g2_random
    gen = CL.START[curve]
    M = sum(CURVE_LENGTHS)
    xs = [rnd(rng) for _ in range(M)]
    es = [_rand_exp(rng) for _ in range(M)]
    es[4] = 0
    xs[3], es[3] = neg(xs[2]), es[2]
    es[10], es[11] = R, U256
    starts = [gen if shared else mul(gen, s + 1) for s in range(len(CURVE_LENGTHS))]
    insts, finals = derive(curve, xs, es, CURVE_LENGTHS, starts)
    sums = sums_of(curve, finals, starts)
    assert heads(CURVE_LENGTHS) == [0, 1, 2, 4, 63, 64, 97, 100] and M == 121
    assert all(f is not None for f in finals) and CL.walk_all(curve, insts) is None
    assert insts[5][1] == insts[4][1] == starts[3]                         # e = 0 at a head: the start passes through
    assert sums[2] is None and finals[2] == starts[2] and [s for s in range(8) if sums[s] is None] == [2]
    assert es[10] == R and es[11] == U256 and (curve != "g1" or insts[11][1] == insts[10][1])   # r x = O on G1
    for s, h in enumerate(heads(CURVE_LENGTHS)):
        assert insts[h][1] == starts[s]
    return xs, es, starts, insts, finals, sums


def field_lengths(num_io):
    """Length 1, a segment with a zero base (4), the segment behind it (3), then 5 and segments of 7 up to num_io - 3: 3 pads."""
    lengths = [1, 4, 3, 5]
    while sum(lengths) + 7 <= num_io - 3:
        lengths.append(7)
    if sum(lengths) < num_io - 3:
        lengths.append(num_io - 3 - sum(lengths))
    return lengths


@functools.lru_cache(maxsize=None)
def field_unit(table, num_io, shared):
    """The one-unit recipe of the field tables (np.random.default_rng(13)): field_lengths(num_io); random bases, the table's edge
    exponents and random ones; instance 2 (inside segment 1) is a zero base with exponent 3, so the final of segment 1 is zero
    and the final of segment 2, which starts afresh, must not be; 0^0 at instance 6.  starts: random per segment, or (shared) one.
    Returns (xs, es, starts, insts, finals)."""
    rng = np.random.default_rng(13)
    rand = lambda: int.from_bytes(rng.bytes(32), "little") % P   # noqa: E731
    u64 = table == "fq12u64"
    edge = T.EXPONENTS_U64 if u64 else T.EXPONENTS
    zero = 0 if table == "fq" else [0] * 12
    one = 1 if table == "fq" else CL.ONE12
    base = rand if table == "fq" else (lambda: [rand() for _ in range(12)])
    lengths = field_lengths(num_io)
    M = sum(lengths)
    xs = [base() for _ in range(M)]
    es = [edge[k % len(edge)] if k % 3 else (rand() % (T.GLP if u64 else 1 << 256)) for k in range(M)]
    xs[2], es[2] = zero, 3
    xs[6], es[6] = zero, 0
    starts = [one if shared else base() for _ in lengths]
    insts, finals = derive(table, xs, es, lengths, starts)
    assert lengths[0] == 1 and M == num_io - 3
    assert finals[1] == zero and insts[3][1] == zero and finals[2] != zero and insts[5][1] == starts[2]
    assert insts[7][1] == insts[6][1]
    return xs, es, starts, insts, finals


@functools.lru_cache(maxsize=None)
def batch_list(table):
    """The recipe of the batch prover (np.random.default_rng(17), BATCH_LENGTHS): more than two units, a segment across each unit
    boundary, the last unit padded; per-segment starts ((s + 1) * generator on G1, random in Fq12).  On G1 segment 1 is a pair
    (x, e), (-x, e) followed by eight more terms.  Returns (num_io, lengths, xs, es, starts, insts, finals, sums); sums is None
    on the field table."""
    num_io, lengths = BATCH_LENGTHS[table]
    rng = np.random.default_rng(17)
    M = sum(lengths)
    hs = heads(lengths)
    straddle = [s for s, (h, n) in enumerate(zip(hs, lengths)) if h // num_io != (h + n - 1) // num_io]
    assert len(straddle) == 2 and M > 2 * num_io and M % num_io
    assert [hs[s] // num_io for s in straddle] == [0, 1]
    if table == "g1":
        add, neg, mul = T._ops("g1")
        xs = [O.g1_random(rng) for _ in range(M)]
        es = [_rand_exp(rng) for _ in range(M)]
        xs[11], es[11] = neg(xs[10]), es[10]
        starts = [mul(T.G1_GEN, s + 1) for s in range(len(lengths))]
        insts, finals = derive("g1", xs, es, lengths, starts)
        assert all(f is not None for f in finals) and CL.walk_all("g1", insts) is None
        assert insts[12][1] == insts[10][1]
        return num_io, lengths, xs, es, starts, insts, finals, sums_of("g1", finals, starts)
    rand = lambda: [int.from_bytes(rng.bytes(32), "little") % P for _ in range(12)]   # noqa: E731
    xs = [rand() for _ in range(M)]
    es = [T.EXPONENTS[k % len(T.EXPONENTS)] if k % 2 else int.from_bytes(rng.bytes(32), "little") for k in range(M)]
    starts = [rand() for _ in lengths]
    insts, finals = derive(table, xs, es, lengths, starts)
    return num_io, lengths, xs, es, starts, insts, finals, None


def padded(table, insts, num_io):
    """(units, num_io, words): the explicit list padded with copies of its last row (the reference's resize rule)."""
    return ML.padded_units(table, insts, num_io)


@functools.lru_cache(maxsize=None)
def refusal_lists(curve):
    """Lists of the curve unit recipe (per-segment starts) the derivation must refuse with SBN_ERR_WITNESS, and an accepted twin:
      'infinity'  the head of segment 5 (instance 64) takes x = -start_5, e = 1: offset[65] is the point at infinity, in segment 5
                  only -- every other segment is untouched;
      'collide'   the head of segment 6 (instance 97) takes x = start_6 and an odd exponent: the table's first addition meets
                  B = A, a degenerate walk at step 0;
      'twin'      the same with bit 0 of that exponent cleared: walked clean, accepted.
    Returns {name: (xs, es)} and the starts."""
    xs, es, starts, _, _, _ = curve_unit(curve, False)
    add, neg, _ = T._ops(curve)
    out = {}
    ix, ie = list(xs), list(es)
    ix[64], ie[64] = neg(starts[5]), 1
    bad, _ = derive(curve, ix, ie, CURVE_LENGTHS, starts)
    assert bad[65][1] is None and all(i[1] is not None for k, i in enumerate(bad) if not 65 <= k < 97)
    out["infinity"] = (ix, ie)
    cx, ce, te = list(xs), list(es), list(es)
    cx[97] = starts[6]
    ce[97], te[97] = es[97] | 1, (es[97] | 1) & ~1
    bad, _ = derive(curve, cx, ce, CURVE_LENGTHS, starts)
    assert CL.walk_all(curve, bad) == (97, 0)
    twin, finals = derive(curve, cx, te, CURVE_LENGTHS, starts)
    assert CL.walk_all(curve, twin) is None and all(f is not None for f in finals)
    out["collide"] = (cx, ce)
    out["twin"] = (cx, te)
    return out, starts
