"""Independent scalar multiplications (every instance carries the same offset, the caller wants e_k x_k: the call shape of the
reference's g2_mul_by_cofactor_circuit, src/curves/g2/circuit.rs:335-367) for the two curve tables, derived in plain Python
integers.  Shared by test_scalar_mul_host.py and test_scalar_mul_gpu.py.

num_io = 128 is the smallest curve table (2^16 rows); count = 133 gives one full unit and a unit of 5 real rows + 123 pads.
Python integers (oracle_lib's g1_* / g2_* through tracegen_edges) are the reference for every product and output, never the code
under test; scalars are 256-bit and never reduced mod r."""
import functools

import numpy as np

import chained_lists as CL
import msm_lists as ML
import oracle_lib as O
import tracegen_edges as T

P, R, U256 = T.P, T.R, T.U256
NUM_IO, COUNT = 128, 133
G2_COFACTOR = 2 * P - R
GEN = {"g1": T.G1_GEN, "g2": T.G2_GEN}
ZERO = {"g1": 16, "g2": 32}   # u32 words of a point


def point_words(curve, pts):
    """[count][16E] u32; None (the point at infinity) as zero words."""
    return np.array([list(CL.value_words(curve, p)) if p is not None else [0] * ZERO[curve] for p in pts], dtype=np.uint32)


def scalar_words(es):
    return np.array([T.limbs(e, 8, 32) for e in es], dtype=np.uint32)


def flags(pts):
    return np.array([1 if p is None else 0 for p in pts], dtype=np.uint8)


def explicit(curve, xs, es, offset):
    """[(x, offset, e)]: the explicit list of the real instances."""
    return [(x, offset, e) for x, e in zip(xs, es)]


@functools.lru_cache(maxsize=None)
def seeded_list(curve):
    """133 instances (np.random.default_rng(31)): random points (on the twist: NOT cofactor-cleared) and random 256-bit scalars from
    the generator as offset, with the fixed instances of the issue, each asserted here so a changed recipe cannot drop a case.
    Returns (xs, es, offset, products, outputs): Python points, None = the point at infinity."""
    rng = np.random.default_rng(31)
    add, neg, mul = T._ops(curve)
    rnd = O.g1_random if curve == "g1" else O.g2_random
    off = GEN[curve]
    xs = [rnd(rng) for _ in range(COUNT)]
    es = [int.from_bytes(rng.bytes(32), "little") for _ in range(COUNT)]
    es[3] = 0
    es[5] = 1
    es[6] = U256
    xs[7], es[7] = xs[5], es[5]
    xs[9], es[9] = neg(add(off, off)), 1
    xs[11], es[11] = (xs[11] if curve == "g1" else mul(xs[11], G2_COFACTOR)), R
    xs[130], es[130] = off, 2
    es[132] = 0
    products = [mul(x, e) for x, e in zip(xs, es)]
    outputs = [add(off, q) for q in products]
    assert all(o is not None for o in outputs)
    assert products[3] is None and products[132] is None and products[11] is None and xs[11] is not None
    assert products[5] == xs[5] and products[7] == products[5]
    assert es[6] == (1 << 256) - 1 and (curve == "g1" or products[6] != mul(xs[6], U256 % R))   # not reduced: off the subgroup it matters
    assert outputs[9] == neg(off) and products[9] == neg(add(off, off))       # output = -offset: the doubling branch of the un-offset
    assert products[130] == add(off, off) and outputs[130] == add(off, add(off, off))
    assert [k for k in range(COUNT) if products[k] is None] == [3, 11, 132]
    assert CL.walk_all(curve, explicit(curve, xs, es, off)) is None            # the table walks every instance
    for k in range(COUNT):                                                      # and reaches Python's outputs
        if k in (3, 5, 6, 9, 11, 130, 132):
            assert T.curve_walk(curve, xs[k], off, es[k])[0] == outputs[k], k
    return xs, es, off, products, outputs


def case(curve):
    """(points, scalars, offset_words, ios_units, product_words, infinity, public-input outputs per instance) of the seeded list."""
    xs, es, off, products, outputs = seeded_list(curve)
    units = ML.padded_units(curve, explicit(curve, xs, es, off), NUM_IO)
    return point_words(curve, xs), scalar_words(es), CL.value_words(curve, off), units, point_words(curve, products), flags(products), outputs


@functools.lru_cache(maxsize=None)
def cofactor_list():
    """The shared-scalar variant: G2_COFACTOR on 133 random twist points (np.random.default_rng(37)).  r * cleared is the point at
    infinity for every instance (asserted): the cleared points are in the prime-order subgroup.  Returns (xs, cleared)."""
    rng = np.random.default_rng(37)
    xs = [O.g2_random(rng) for _ in range(COUNT)]
    cleared = [O.g2_mul(x, G2_COFACTOR) for x in xs]
    assert all(c is not None and O.g2_mul(c, R) is None for c in cleared)
    assert any(O.g2_mul(x, R) is not None for x in xs)                         # the inputs are off the subgroup
    assert CL.walk_all("g2", explicit("g2", xs, [G2_COFACTOR] * COUNT, T.G2_GEN)) is None
    return xs, cleared


def cofactor_case():
    """(points, ios_units, cleared_words) of the cofactor list."""
    xs, cleared = cofactor_list()
    units = ML.padded_units("g2", explicit("g2", xs, [G2_COFACTOR] * COUNT, T.G2_GEN), NUM_IO)
    return point_words("g2", xs), units, point_words("g2", cleared)


def public_inputs(S, curve, units):
    """The public inputs of every unit from the host generators (generate_public_inputs per unit)."""
    stark = T.stark_class(S, curve)(NUM_IO)
    return [stark.generate_public_inputs(u) for u in units]
